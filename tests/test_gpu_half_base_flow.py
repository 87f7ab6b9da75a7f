"""The base flow of an exactly doubled pyramid level kept at the previous level's size.

At such a level the up-sampled flow is a replication -- every 2 x 2 block of pixels holds one value of the previous level after the
resample's multiplications -- so the warp stores it once per block (flow2d_upsample_registration_half_2d) and its readers index it
with (y >> 1, x >> 1): the strip solver (flow2d_solve_params.base_flow_shift = 1) and the median with addend
(flow2d_add_median_2d_pair_half).  The contract is bit identity (uint32 views: NaN payloads, signed zeros, denormals count) with
the full-size entries fed the replicated planes -- those are held to the oracle and to the reference kernels elsewhere -- and whole
pyramids that equal the CPU oracle in every pixel on whichever path their levels select.
"""
import numpy as np
import pytest

from conftest import level_fields

pytestmark = pytest.mark.gpu

U32, F32 = np.uint32, np.float32
POISON = 0x7F7F7F7F
UNSUPPORTED = 5
GREY, GRADIENT, GRADIENT_UNTILED, LOG_DERIVATIVES = 0, 1, 2, 3
FUSED, PER_SWEEP = 2, 1


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def replicate(half, w, h):
    return np.repeat(np.repeat(half, 2, axis=0), 2, axis=1)[:h, :w]


def special_flow(w, h, seed, scale=3.0):
    """A flow plane with what arithmetic treats specially: -0 (the resample's chain turns it into +0), NaNs with payloads, both
    infinities, denormals (they round in the chain), and vectors that leave any frame of this size."""
    a = (np.random.default_rng(seed).normal(0, 1, (h, w)) * scale).astype(F32)
    a[0, 0:6] = -0.0
    a[1, 1:5] = np.array([1e-40, -3e-41, 1.4e-45, -1e-39], F32)
    a[2, 3] = np.inf
    a[3, 2] = -np.inf
    a.view(U32)[4, 7] = 0x7FC12345
    a.view(U32)[h - 1, w - 1] = 0xFFC00001
    a[h // 2, :] = 1000.0
    a[:, w // 2] = -1000.0
    a[h - 2, 0] = -0.0
    return a


# ---- the warp ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pw,ph", [(32, 16), (33, 17), (100, 60)])
def test_half_warp_equals_the_full_size_warp(ctx, pw, ph):
    w, h = 2 * pw, 2 * ph
    rng = np.random.default_rng(pw)
    f0, f1 = rng.uniform(0, 255, (h, w)).astype(F32), rng.uniform(0, 255, (h, w)).astype(F32)
    u, v = special_flow(pw, ph, 1), special_flow(pw, ph, 2)
    d = [ctx.plane(w, h, a) for a in (u, v, f0, f1)]
    for hx, hy in ((1.0, 1.0), (2.0, 4.0), (1.37, 0.9)):
        full_u, full_v, full_w, half_u, half_v, half_w = (ctx.plane(w, h).fill_bytes(0x7F) for _ in range(6))
        ctx.upsample_registration(d[0], d[1], pw, ph, full_u, full_v, d[2], d[3], w, h, hx, hy, full_w)
        ctx.upsample_registration_half(d[0], d[1], pw, ph, half_u, half_v, d[2], d[3], w, h, hx, hy, half_w)
        ctx.synchronize()
        assert np.array_equal(bits(full_w.download()), bits(half_w.download())), "the warped frame"
        for full, half, name in ((full_u, half_u, "u"), (full_v, half_v, "v")):
            got = bits(half.download())
            assert np.array_equal(bits(full.download()), replicate(got[:ph, :pw], w, h)), name
            outside = np.ones(got.shape, bool)
            outside[:ph, :pw] = False
            assert (got[outside] == POISON).all(), "words outside the half-size region were written"
    # (the chain is not the identity: the -0 entries came out as +0)
    assert (bits(half_u.download())[0, 0:6] == 0).all() and (bits(u)[0, 0:6] == 0x80000000).all()


def test_half_warp_batch_of_three_with_a_padded_stride(ctx):
    pw, ph, G, pad = 33, 17, 3, 5
    w, h = 2 * pw, 2 * ph
    stride_rows = h + pad
    rng = np.random.default_rng(9)

    def stack(arrays):
        full = np.full((stride_rows * G, w), POISON, U32)
        for b, a in enumerate(arrays):
            full[b * stride_rows:b * stride_rows + a.shape[0], :a.shape[1]] = bits(a)
        return ctx.plane(w, stride_rows * G).upload(full.view(F32))

    us, vs = [special_flow(pw, ph, 10 + b) for b in range(G)], [special_flow(pw, ph, 20 + b) for b in range(G)]
    f0s, f1s = ([rng.uniform(0, 255, (h, w)).astype(F32) for _ in range(G)] for _ in range(2))
    d = [stack(x) for x in (us, vs, f0s, f1s)]
    full_u, full_v, full_w, half_u, half_v, half_w = (stack([]) for _ in range(6))
    with ctx.set_batch(G, stride_rows * d[0].pitch):
        ctx.upsample_registration(d[0], d[1], pw, ph, full_u, full_v, d[2], d[3], w, h, 1.0, 1.0, full_w)
        ctx.upsample_registration_half(d[0], d[1], pw, ph, half_u, half_v, d[2], d[3], w, h, 1.0, 1.0, half_w)
    ctx.synchronize()
    assert np.array_equal(bits(full_w.download()), bits(half_w.download()))
    for full, half in ((full_u, half_u), (full_v, half_v)):
        want, got = bits(full.download()), bits(half.download())
        outside = np.ones(got.shape, bool)
        for b in range(G):
            r = b * stride_rows
            assert np.array_equal(want[r:r + h], replicate(got[r:r + ph, :pw], w, h)), b
            outside[r:r + ph, :pw] = False
        assert (got[outside] == POISON).all()


def test_half_warp_refuses_other_ratios_and_overlaps(ctx, flow2d):
    w, h = 64, 32
    planes = [ctx.plane(w, 2 * h, np.zeros((2 * h, w), F32)) for _ in range(7)]
    u, v, ou, ov, f0, f1, out = planes
    with pytest.raises(flow2d.Flow2DError) as e:
        ctx.upsample_registration_half(u, v, 30, 16, ou, ov, f0, f1, w, h, 1.0, 1.0, out)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(flow2d.Flow2DError) as e:  # out_u starts in the last row of the flow read
        hip = flow2d.hip_lib()
        flow2d._check(hip.flow2d_upsample_registration_half_2d(ctx.handle, u.ptr, v.ptr, 32, 16, u.ptr + 15 * u.pitch, ov.ptr, f0.ptr, f1.ptr,
                                                               w, h, u.pitch, 1.0, 1.0, out.ptr), "flow2d_upsample_registration_half_2d")
    assert e.value.status == 1


# ---- the median --------------------------------------------------------------------------------------------------------------

def planted(a, seed):
    a = a.copy()
    h, w = a.shape
    rng = np.random.default_rng(seed)
    for k in range(6):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        a.view(U32)[y, x] = (0x7FC00000 + k) if k % 2 else 0x80000000
    a[0, 0] = -0.0
    a.view(U32)[h - 1, w - 1] = 0x7FC00077
    return a


@pytest.mark.parametrize("window", [3, 5, 7])
@pytest.mark.parametrize("w,h", [
    (66, 34),     # every wave an edge wave
    (200, 120),   # interior waves
    (20, 12),     # a few pixels (the streaming kernels still: they take over from 8 x 8 / 12 x 12)
    (20, 6),      # lower than the streaming kernels' minimum: the generic kernel, all three windows
    (67, 35),     # odd sizes: the last row and column of the half-size plane serve one pixel row / column
])
@pytest.mark.parametrize("special", [False, True], ids=["plain", "nan_and_negative_zero"])
def test_half_median_equals_the_median_of_the_replicated_base(ctx, w, h, window, special):
    pw, ph = (w + 1) // 2, (h + 1) // 2
    rng = np.random.default_rng(w * window)
    bases = [rng.normal(0, 2, (ph, pw)).astype(F32) for _ in range(2)]
    adds = [rng.normal(0, 0.5, (h, w)).astype(F32) for _ in range(2)]
    if special:
        bases = [planted(a, 3 + i) for i, a in enumerate(bases)]
        adds = [planted(a, 5 + i) for i, a in enumerate(adds)]
        bases[0][1, 1], adds[0][2:4, 2:4] = 0.0, -0.0  # +0 + -0 = +0 beside -0 + -0 elsewhere
        bases[1][:] = -0.0
        adds[1][::3, :] = -0.0                          # whole runs of -0 sums: the stable order of equal zeros shows
    half = [ctx.plane(w, h, a) for a in bases]
    full = [ctx.plane(w, h, replicate(a, w, h)) for a in bases]
    add = [ctx.plane(w, h, a) for a in adds]
    want_a, want_b, got_a, got_b = (ctx.plane(w, h).fill_bytes(0x7F) for _ in range(4))
    ctx.add_median(full[0], add[0], w, h, window, want_a, full[1], add[1], want_b)
    ctx.add_median_half(half[0], add[0], w, h, window, got_a, half[1], add[1], got_b)
    ctx.synchronize()
    assert np.array_equal(bits(want_a.download()), bits(got_a.download()))
    assert np.array_equal(bits(want_b.download()), bits(got_b.download()))
    # a single plane set
    one = ctx.plane(w, h).fill_bytes(0x7F)
    ctx.add_median_half(half[0], add[0], w, h, window, one)
    ctx.synchronize()
    assert np.array_equal(bits(want_a.download()), bits(one.download()))


# ---- the strip solver --------------------------------------------------------------------------------------------------------

def solve_both(ctx, f0, f1, u_half, v_half, w, h, hx, hy, outer, inner, constancy, alpha=35.0, e=0.001):
    """(du, dv) of the strips with the replicated base at full size, and with the half-size base and base_flow_shift = 1"""
    out = []
    for shift in (0, 1):
        u, v = (u_half, v_half) if shift else (replicate(u_half, w, h), replicate(v_half, w, h))
        d = [ctx.plane(w, h, a) for a in (f0, f1)] + [ctx.plane(w, h).fill_bytes(0x7F).upload(a) for a in (u, v)]
        scratch = [ctx.plane(w, h).fill_bytes(0x7F) for _ in range(6)]
        rdu, rdv = ctx.solve_level(*d, *scratch, w, h, hx, hy, alpha, e, e, outer, inner, constancy, FUSED, base_flow_shift=shift)
        out.append((bits(rdu.download(w, h)), bits(rdv.download(w, h))))
        for p in d + scratch:
            p.free()
    return out


@pytest.mark.parametrize("constancy", [GREY, GRADIENT, GRADIENT_UNTILED, LOG_DERIVATIVES])
@pytest.mark.parametrize("w,h", [(128, 96), (320, 208)])
def test_shifted_base_gives_the_bits_of_the_replicated_base(ctx, oracle, w, h, constancy):
    """Inner 1, 2, 5 and 7 (7: a continued launch of 4 + 3 sweeps), outer 3 (the first launch takes zero increments), a power-of-two
    and another spacing.  320 x 208 holds strips that touch no border, the others run the border body."""
    if (w, h) == (320, 208):
        for inner in (1, 2, 3, 4, 5):
            order = ctx.fused_block_order(w, h, inner)
            halo, valid = inner + 1, 64 - 2 * (inner + 1)
            # a wave takes the interior body when its 64 columns and its rows with their halo keep off every border: one block must
            # hold such a strip column (its four waves are strip columns 4 bx .. 4 bx + 3) AND such rows
            inside = [(bx, s, y0, y1) for bx, by, y0, y1 in order.tolist() if bx >= 0 and y0 > halo + 1 and y1 + halo + 4 < h
                      for s in range(4 * bx, 4 * bx + 4) if s * valid < w and s * valid - halo > 0 and s * valid - halo + 63 < w - 1]
            assert inside, ("no strip without a border", inner)
    f0, f1, u, v, _, _ = level_fields(oracle, w, h, 61)
    if constancy == LOG_DERIVATIVES:
        f0, f1 = np.abs(f0), np.abs(f1)
    u_half, v_half = u[:h // 2, :w // 2].copy(), v[:h // 2, :w // 2].copy()
    before = ctx.fused_fallbacks()
    for spacing in (1.0, 1.37):
        for inner in (1, 2, 5, 7):
            (a_du, a_dv), (b_du, b_dv) = solve_both(ctx, f0, f1, u_half, v_half, w, h, F32(spacing), F32(spacing), 3, inner, constancy)
            assert not (a_du == POISON).any()
            assert np.array_equal(a_du, b_du) and np.array_equal(a_dv, b_dv), (spacing, inner)
    if constancy != LOG_DERIVATIVES:
        assert ctx.fused_fallbacks() == before  # (ordinary operands: every wave took the guarded short forms)


def test_shifted_base_in_a_batch_of_three(ctx, oracle):
    w, h, G, pad = 320, 208, 3, 4
    stride_rows = h + pad
    fields = [level_fields(oracle, w, h, 70 + b) for b in range(G)]

    def stack(arrays):
        full = np.full((stride_rows * G, w), POISON, U32)
        for b, a in enumerate(arrays):
            full[b * stride_rows:b * stride_rows + a.shape[0], :a.shape[1]] = bits(a)
        return ctx.plane(w, stride_rows * G).upload(full.view(F32))

    halves = [[f[k][:h // 2, :w // 2] for f in fields] for k in (2, 3)]
    res = []
    for shift in (0, 1):
        base = halves if shift else [[replicate(a, w, h) for a in plane] for plane in halves]
        d = [stack([f[0] for f in fields]), stack([f[1] for f in fields]), stack(base[0]), stack(base[1])]
        scratch = [stack([]) for _ in range(6)]
        with ctx.set_batch(G, stride_rows * d[0].pitch):
            rdu, rdv = ctx.solve_level(*d, *scratch, w, h, 1.0, 1.0, 35.0, 0.001, 0.001, 3, 5, GRADIENT, FUSED,
                                       container_height=h, base_flow_shift=shift)
        ctx.synchronize()
        res.append((bits(rdu.download()), bits(rdv.download())))
    for b in range(G):
        r = slice(b * stride_rows, b * stride_rows + h)
        assert not (res[0][0][r] == POISON).any()
        assert np.array_equal(res[0][0][r], res[1][0][r]) and np.array_equal(res[0][1][r], res[1][1][r]), b


def test_shifted_base_with_a_negative_zero_takes_the_fallback_pass(ctx):
    """Flat frames and a base flow of -0: every numerator is a -0, the one zero the three-step division gets wrong.  The guard sees
    the -0 entries as they are read -- through the shifted loads too -- and the plain pass (the border body) repeats the strips."""
    w, h = 320, 208
    f0 = np.full((h, w), 80.0, F32)
    u_half, v_half = np.full((h // 2, w // 2), -0.0, F32), np.zeros((h // 2, w // 2), F32)
    before = ctx.fused_fallbacks()
    (a_du, a_dv), (b_du, b_dv) = solve_both(ctx, f0, f0.copy(), u_half, v_half, w, h, F32(1.0), F32(1.0), 3, 5, GREY)
    assert ctx.fused_fallbacks() >= before + 2  # both runs tripped
    assert not (a_du == POISON).any()
    assert np.array_equal(a_du, b_du) and np.array_equal(a_dv, b_dv)


@pytest.mark.parametrize("algorithm", [PER_SWEEP, 3, 4])
def test_a_shift_with_another_algorithm_is_refused_before_a_launch(ctx, flow2d, oracle, algorithm):
    w, h = 64, 32
    f0, f1, u, v, _, _ = level_fields(oracle, w, h, 3)
    d = [ctx.plane(w, h, a) for a in (f0, f1, u, v)]
    scratch = [ctx.plane(w, h).fill_bytes(0x7F) for _ in range(6)]
    with pytest.raises(flow2d.Flow2DError) as e:
        ctx.solve_level(*d, *scratch, w, h, 1.0, 1.0, 35.0, 0.001, 0.001, 2, 5, GREY, algorithm, base_flow_shift=1)
    assert e.value.status == UNSUPPORTED
    with pytest.raises(flow2d.Flow2DError) as e:
        ctx.solve_level(*d, *scratch, w, h, 1.0, 1.0, 35.0, 0.001, 0.001, 2, 5, GREY, FUSED, base_flow_shift=2)
    assert e.value.status == UNSUPPORTED
    ctx.synchronize()
    for p in scratch:
        assert (bits(p.download()) == POISON).all()


# ---- whole pyramids ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pyramid_reference(oracle):
    """The oracle's flows the pyramid tests compare with, computed once: (w, h, levels, scale, constancy, seed) -> (u, v)"""
    cache = {}

    def get(w, h, levels, scale, constancy, seed):
        key = (w, h, levels, scale, constancy, seed)
        if key not in cache:
            f0, f1 = oracle.synthetic_pair(w, h, 1.0 + 0.5 * seed, -0.5 * seed, seed=30 + seed, noise=True)
            cache[key] = (f0, f1) + tuple(oracle.compute_flow(f0, f1, levels, scale, 3, 5, 35.0, 0.001, 0.001, 5, 1.5, constancy)[:2])
        return cache[key]
    return get


@pytest.mark.parametrize("w,h,levels,scale,constancy,algorithm,eligible", [
    (256, 128, 3, 0.5, GREY, FUSED, 2),        # 64 x 32 (no previous flow), then two exactly doubled levels on the strips
    (256, 128, 3, 0.5, GRADIENT, FUSED, 2),
    (256, 128, 3, 0.5, GRADIENT, 0, 0),        # AUTO: levels of this size go to the tiles
    (200, 120, 3, 0.6, GRADIENT, FUSED, 0),    # 72 x 44, 120 x 72, 200 x 120: no level twice the previous one
])
def test_pyramids_equal_the_oracle_and_count_their_half_size_levels(flow2d, ctx, pyramid_reference, w, h, levels, scale, constancy,
                                                                    algorithm, eligible):
    f0, f1, ou, ov = pyramid_reference(w, h, levels, scale, constancy, 0)
    p = flow2d.OpticalFlow.params(levels, scale, 3, 5, 35.0, 0.001, 0.001, 5, 1.5, algorithm)
    flow = flow2d.OpticalFlow(w, h, constancy, ctx=ctx)
    try:
        planes = [ctx.plane(w, h, f0), ctx.plane(w, h, f1), ctx.plane(w, h), ctx.plane(w, h)]
        for graph, rounds in ((False, 1), (True, 2)):
            flow.use_graph(graph)
            for rnd in range(rounds):
                planes[2].fill_bytes(0x55)
                planes[3].fill_bytes(0x55)
                before = flow2d.half_base_flow_launches()
                flow.compute_flow_device(*[q.ptr for q in planes], p)
                ctx.synchronize()
                launched = flow2d.half_base_flow_launches() - before
                assert launched == (eligible if rnd == 0 else 0), (graph, rnd, launched)  # (a replayed graph calls no launcher)
                assert np.array_equal(planes[2].download(), ou) and np.array_equal(planes[3].download(), ov), (graph, rnd)
    finally:
        flow.close()


@pytest.mark.parametrize("constancy", [GREY, GRADIENT])
def test_lock_step_group_of_three_equals_the_oracle(flow2d, pyramid_reference, constancy):
    w, h, G = 256, 128, 3
    ref = [pyramid_reference(w, h, 3, 0.5, constancy, k) for k in range(G)]
    c = flow2d.Context(0)
    batch = flow2d.OpticalFlowBatch(w, h, constancy, lanes=1, group_size=G)
    try:
        planes = [c.plane(w, h * G, np.vstack([q[0] for q in ref])), c.plane(w, h * G, np.vstack([q[1] for q in ref])),
                  c.plane(w, h * G), c.plane(w, h * G)]
        params = batch.params(3, 0.5, 3, 5, 35.0, 0.001, 0.001, 5, 1.5, FUSED)
        for graph, rounds in ((False, 1), (True, 2)):
            batch.use_graph(graph)
            for rnd in range(rounds):
                planes[2].fill_bytes(0x7F)
                planes[3].fill_bytes(0x7F)
                c.synchronize()
                before = flow2d.half_base_flow_launches()
                batch.compute_flow_batch_device(*[[q.ptr] for q in planes], params)
                batch.synchronize()
                launched = flow2d.half_base_flow_launches() - before
                assert launched == (2 if rnd == 0 else 0), (graph, rnd, launched)  # one launch per eligible level for the whole group
                u, v = planes[2].download(), planes[3].download()
                for k, q in enumerate(ref):
                    assert np.array_equal(u[k * h:(k + 1) * h], q[2]) and np.array_equal(v[k * h:(k + 1) * h], q[3]), (graph, rnd, k)
    finally:
        batch.close()
        c.close()
