"""flow2d_subset_refine_2d on the device against its numpy restatement (tests/test_subset_cpu.py): states and records exactly, the
float planes within max(one fp32 ulp, 16 x the spread of the restatement's three summation orders on that input) -- the kernel
sums in the restatement's "butterfly" order, so the bytes are expected to match and each case prints whether they did.  A
one-subset frame, a dense grid with fewer pixels than lanes, subsets larger than the grid's windows, the largest subset, several
workgroups with a node count that is no multiple of the waves, non-finite and huge inputs, one and sixty-four iterations, every
optional output absent, containers larger than the data with poisoned outputs; the same bytes from repeated calls, a replayed
graph and an instance alone or in a lock-step batch; the refusals on a real context."""
import ctypes

import numpy as np
import pytest

from test_correlate_cpu import F32, U32, bits, correlate_reference, frame_range, grid, random_frames, scenes_module
from test_gpu_batch_kernels import Tall, pitch_of, stride_of
from test_gpu_multipass import POISON, padded, release
from test_subset_cpu import FLAT, NO_INPUT, STRAYED, SUBSET_DTYPE, Refined, all_orders

pytestmark = pytest.mark.gpu
F64 = np.float64


def run_subset(ctx, f0, f1, u0, v0, r, s, R, K=20, epsilon=1e-3, max_shift=2.0, max_gradient=0.5, gradients=True, score=True, state=True,
               record=True):
    """(the eight planes' bits -- None where absent --, record bytes or None) of one call into poisoned outputs, which must stay
    poisoned beyond the grid; frames and inputs lie in containers larger than the data, NaN beyond it."""
    h, w = f0.shape
    nh, nw = u0.shape
    frames = [padded(ctx, f0), padded(ctx, f1)]
    start = [padded(ctx, u0), padded(ctx, v0)]
    outs = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(8)]
    rec = ctx.subset_records().fill_bytes(0x7F)
    ctx.subset_refine(frames[0], frames[1], w, h, start[0], start[1], nw, nh, r, s, R, K, epsilon, max_shift, max_gradient, outs[0], outs[1],
                      outs[2:6] if gradients else None, outs[6] if score else None, outs[7] if state else None, rec if record else None)
    ctx.synchronize()
    present = [True, True] + [gradients] * 4 + [score, state]
    got = [q.download().view(U32) for q in outs]
    for g, there in zip(got, present):
        if there:
            assert (g[nh:] == POISON).all() and (g[:, nw:] == POISON).all(), "written beyond the grid"
        else:
            assert (g == POISON).all(), "an absent plane was written"
    raw = rec.download(16, 1).tobytes()
    assert record or set(raw) == {0x7F}
    result = [g[:nh, :nw] if there else None for g, there in zip(got, present)], (raw if record else None)
    release(ctx, frames + start + outs + [rec])
    return result


def compare(got, want, spread, what):
    """The device's planes (bits) and record against the restatement `want` (Refined); returns whether every byte matched."""
    planes, raw = got
    exact = True
    if planes[7] is not None:
        assert np.array_equal(planes[7], bits(want.state)), "%s: states %s, want %s" % (what, planes[7].view(F32), want.state)
    if raw is not None:
        assert raw == want.record.tobytes(), "%s: record %s, want %s" % (what, np.frombuffer(raw, SUBSET_DTYPE), want.record)
    live = want.state >= 0
    for g, w_plane, name in zip(planes[:7], want.planes()[:7], Refined.NAMES[:7]):
        if g is None:
            continue
        wbits = bits(w_plane)
        assert np.array_equal(g[~live], wbits[~live]), "%s: %s of a node that was not refined" % (what, name)
        same = g[live] == wbits[live]
        exact &= bool(same.all())
        tolerance = np.maximum(np.spacing(np.abs(w_plane[live])).astype(F64), 16.0 * spread)
        off = np.abs(g[live].view(F32).astype(F64) - w_plane[live].astype(F64))
        print("%s: %s: %d of %d words differ, largest difference %.3e" % (what, name, (~same).sum(), same.size, off.max() if off.size else 0.0))
        assert (off <= tolerance).all(), "%s: %s off by %.3e (allowed %.3e)" % (what, name, off.max(), tolerance[off.argmax()])
    print("%s: bytes %s" % (what, "match" if exact else "DIFFER within the tolerance"))
    return exact


def check_subset(ctx, f0, f1, u0, v0, r, s, R, what, **kw):
    want, spread = all_orders(f0, f1, u0, v0, r, s, R, **kw)
    compare(run_subset(ctx, f0, f1, u0, v0, r, s, R, **kw), want, spread, what)
    return want


def speckle_case(w, h, r, s, d=4, motion="affine", seed=0):
    """A speckle pair of any size and the node field flow2d_correlate_2d's restatement finds on it."""
    sc = scenes_module().make_speckle_scene(motion, w, h, seed=seed)
    lo, scale = frame_range(sc.frame_0, sc.frame_1)
    u0, v0, _, _, _ = correlate_reference(sc.frame_0, sc.frame_1, lo, scale, r, d, s)
    return sc.frame_0, sc.frame_1, u0, v0


def counts(want):
    return {k: int(want.record[k][0]) for k in SUBSET_DTYPE.names[:7]}


# ---- shapes -------------------------------------------------------------------------------------------------------------------------
def test_one_subset_frame(flow2d, ctx):
    f0, _ = random_frames(7, 7, seed=2, shift=(0, 0))
    zero = np.zeros((1, 1), F32)
    want = check_subset(ctx, f0, f0, zero, zero, 3, 3, 3, "7x7, f1 = f0")
    assert counts(want) == dict(nodes=1, converged=1, unconverged=0, strayed=0, flat=0, no_input=0, iterations=1)
    assert want.state[0, 0] == 1 and want.u[0, 0] == 0 and want.v[0, 0] == 0 and want.score[0, 0] == 1
    want = check_subset(ctx, f0, f0, np.ones((1, 1), F32), zero, 3, 3, 3, "7x7, u0 = 1")
    assert want.state[0, 0] == STRAYED and counts(want)["iterations"] == 1 and want.u[0, 0] == 1


def test_tiny_dense_grid(flow2d, ctx):
    f0, f1 = random_frames(9, 7, seed=5, shift=(0, 0), noise=2.0)
    zero = np.zeros((5, 7), F32)
    want = check_subset(ctx, f0, f1, zero, zero, 1, 1, 1, "9x7 dense, N = 9")
    c = counts(want)
    assert c["nodes"] == 35 and c["iterations"] > 35 and min(c["converged"], c["unconverged"], c["strayed"]) >= 1  # (nine pixels for six unknowns: every outcome)


@pytest.mark.parametrize("R", [3, 6])
def test_subsets_at_and_beyond_the_grid_radius(flow2d, ctx, R):
    """50 x 41 with the grid (3, s 5): nine nodes per row, no multiple of the waves.  R = 6: the subsets of the first row and
    column leave frame 0, and more border nodes leave frame 1 on the way."""
    f0, f1, u0, v0 = speckle_case(50, 41, 3, 5)
    assert u0.shape == (7, 9)
    want = check_subset(ctx, f0, f1, u0, v0, 3, 5, R, "50x41, R = %d" % R)
    c = counts(want)
    assert c["converged"] >= 15 and (c["strayed"] >= 15 if R == 6 else True)


def test_largest_subset(flow2d, ctx):
    f0, f1, u0, v0 = speckle_case(97, 99, 15, 33, d=3)
    assert u0.shape == (3, 3)
    want = check_subset(ctx, f0, f1, u0, v0, 15, 33, 15, "97x99, R = 15, N = 961")
    assert counts(want)["converged"] >= 1


_small_specimen = []


def small_specimen():
    """40 x 36, grid (3, s 4), 9 x 8 nodes: the stretched specimen's frames at that size and the truth rounded to whole pixels as the
    start -- the case of test_gpu_subset_masked.py's large radii, made once."""
    if not _small_specimen:
        scene, _ = scenes_module().make_speckle_specimen("stretch", 40, 36, seed=0)
        nw, nh = grid(40, 36, 3, 4)
        cy, cx = 3 + np.arange(nh) * 4, 3 + np.arange(nw) * 4
        _small_specimen.append((scene.frame_0, scene.frame_1, np.rint(scene.gt_u[np.ix_(cy, cx)]).astype(F32),
                                np.rint(scene.gt_v[np.ix_(cy, cx)]).astype(F32)))
    return _small_specimen[0]


@pytest.mark.parametrize("R", [10, 11, 12, 13, 15])
def test_the_large_radii(flow2d, ctx, R):
    """The radii around every change of the waves per workgroup: four at R = 10, three at 11 and 12 (node = blockIdx.x * 3 + wave),
    two from 13.  40 x 36: only the inner nodes' subsets lie inside frame 0, the others stray."""
    f0, f1, u0, v0 = small_specimen()
    assert u0.shape == (8, 9) and u0.size % 3 == 0 and u0.size % 4 == 0  # (72 nodes: 18, 24 and 36 full workgroups)
    want = check_subset(ctx, f0, f1, u0, v0, 3, 4, R, "40x36 specimen, R = %d" % R)
    c = counts(want)
    assert (want.state >= 0).sum() >= 1 and c["strayed"] >= 20


def test_several_workgroups(flow2d, ctx):
    f0, f1, u0, v0 = speckle_case(130, 37, 7, 8)
    assert u0.shape == (3, 15) and u0.size % 4 != 0
    want = check_subset(ctx, f0, f1, u0, v0, 7, 8, 7, "130x37, (7, s 8)")
    assert counts(want)["converged"] >= 20


def test_wide_bounds(flow2d, ctx):
    """Bounds so wide that no node strays by them, and bounds so tight that many do."""
    f0, f1, u0, v0 = speckle_case(50, 41, 3, 5)
    want = check_subset(ctx, f0, f1, u0, v0, 3, 5, 3, "max_shift 100, max_gradient 10", max_shift=100.0, max_gradient=10.0)
    tight = check_subset(ctx, f0, f1, u0, v0, 3, 5, 3, "max_shift 0.5, max_gradient 0.05", max_shift=0.5, max_gradient=0.05)
    assert counts(tight)["strayed"] > counts(want)["strayed"]


def test_non_finite_and_huge_inputs(flow2d, ctx):
    f0, f1, u0, v0 = speckle_case(50, 41, 3, 5)
    u0, v0, f0, f1 = u0.copy(), v0.copy(), f0.copy(), f1.copy()
    u0[1, 1], v0[2, 2], u0[3, 3], v0[4, 4], u0[5, 5] = np.nan, np.inf, 1e30, -3e38, -np.inf
    f0[8, 38], f1[33, 8] = np.nan, np.inf
    want = check_subset(ctx, f0, f1, u0, v0, 3, 5, 3, "non-finite and huge")
    assert want.state[1, 1] == NO_INPUT and want.state[2, 2] == NO_INPUT and want.state[5, 5] == NO_INPUT
    assert want.state[3, 3] == STRAYED and want.state[4, 4] == STRAYED and want.state[1, 7] == FLAT and want.state[6, 1] == FLAT
    flat = np.full_like(f0, 9.0)
    want = check_subset(ctx, flat, f1, u0, v0, 3, 5, 3, "constant frame 0")
    assert counts(want)["flat"] == u0.size - counts(want)["no_input"] and counts(want)["no_input"] >= 3


def test_one_and_sixty_four_iterations(flow2d, ctx):
    f0, f1, u0, v0 = speckle_case(50, 41, 3, 5)
    want = check_subset(ctx, f0, f1, u0, v0, 3, 5, 3, "K = 1", K=1)
    assert counts(want)["iterations"] == u0.size
    want = check_subset(ctx, f0, f1, u0, v0, 3, 5, 3, "K = 64, epsilon 0", K=64, epsilon=0.0)
    c = counts(want)
    assert c["converged"] == 0 and c["unconverged"] >= 15 and c["iterations"] >= 64 * c["unconverged"]


def test_every_optional_output_absent(flow2d, ctx):
    f0, f1, u0, v0 = speckle_case(50, 41, 3, 5)
    want, spread = all_orders(f0, f1, u0, v0, 3, 5, 3)
    compare(run_subset(ctx, f0, f1, u0, v0, 3, 5, 3, gradients=False, score=False, state=False, record=False), want, spread, "u and v only")
    compare(run_subset(ctx, f0, f1, u0, v0, 3, 5, 3, gradients=True, score=False, state=True, record=False), want, spread, "no score, no record")


def test_the_wrapper_allocates_and_downloads(flow2d, ctx):
    f0, f1, u0, v0 = speckle_case(50, 41, 3, 5)
    want, spread = all_orders(f0, f1, u0, v0, 3, 5, 3)
    p0, p1, pu, pv = ctx.plane(50, 41, f0), ctx.plane(50, 41, f1), ctx.plane(9, 7, u0), ctx.plane(9, 7, v0)
    u, v, gradients, score, state, rec = ctx.subset_refine(p0, p1, 50, 41, pu, pv, 9, 7, 3, 5, 3)
    compare(([bits(q) for q in (u, v) + gradients + (score, state)], bytes(rec)), want, spread, "wrapper")
    assert rec.summary() == counts(want)


# ---- the same bytes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [3, 7])
def test_four_entries_give_the_same_bytes(flow2d, ctx, R):
    """flow2d_subset_refine_2d, flow2d_subset_refine_from_2d with four all-zero start planes and flow2d_subset_refine_masked_2d
    without a mask and with an all-zero one: the same eight planes and the same record, byte for byte, the record's eighth word 0.
    48 x 40 with the grid (7, s 8), 5 x 4 nodes: R = 3 leaves lanes idle (N = 49), R = 7 gives a lane several pixels; one node
    without input, one whose start takes its subset out of the frame, one on a flat patch of frame 0."""
    from test_gpu_subset_masked import run_masked  # (those modules import this one)
    from test_gpu_subset_sequence import run_from

    f0, f1, u0, v0 = speckle_case(48, 40, 7, 8)
    assert u0.shape == (4, 5)
    f0, u0 = f0.copy(), u0.copy()
    u0[1, 1], u0[0, 0] = np.nan, -20.0
    f0[23 - 8:23 + 9, 31 - 8:31 + 9] = 100.0  # node (3, 2), centre (31, 23): its subset and the stencil around it
    zeros = [np.zeros_like(u0) for _ in range(4)]
    got = {"plain": run_subset(ctx, f0, f1, u0, v0, 7, 8, R, max_shift=2.0),
           "from, zero start": run_from(ctx, f0, f1, [u0, v0] + zeros, 7, 8, R, max_shift=2.0),
           "masked, no mask": run_masked(ctx, f0, f1, (u0, v0), None, 0, 7, 8, R, max_shift=2.0),
           "masked, zero mask": run_masked(ctx, f0, f1, (u0, v0), np.zeros_like(f0), (2 * R + 1) ** 2, 7, 8, R, max_shift=2.0)}
    planes, raw = got["plain"]
    state = planes[7].view(F32)
    assert state[1, 1] == NO_INPUT and state[0, 0] == STRAYED and state[2, 3] == FLAT and (state >= 1).sum() >= 5
    assert np.isnan(planes[0].view(F32)[1, 1]) and planes[0].view(F32)[0, 0] == -20.0 and not planes[2][0, 0] and not planes[5][2, 3]
    record = np.frombuffer(raw, SUBSET_DTYPE)[0]
    assert record["nodes"] == 20 and record["no_input"] == 1 and record["flat"] >= 1 and record["strayed"] >= 1
    for what, (other, other_raw) in got.items():
        for name, a, b in zip(Refined.NAMES, other, planes):
            assert np.array_equal(a, b), "%s: %s" % (what, name)
        assert other_raw == raw and np.frombuffer(other_raw, SUBSET_DTYPE)["reserved"][0] == 0, what


def test_repeated_calls_and_a_replayed_graph(flow2d, ctx):
    w, h, r, s, R = 130, 37, 7, 8, 7
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    f0, f1, u0, v0 = speckle_case(w, h, r, s)
    nh, nw = u0.shape
    frames, start = [padded(ctx, f0), padded(ctx, f1)], [padded(ctx, u0), padded(ctx, v0)]
    outs = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(8)]
    rec = ctx.subset_records().fill_bytes(0x7F)

    def call():
        ctx.subset_refine(frames[0], frames[1], w, h, start[0], start[1], nw, nh, r, s, R, out_u=outs[0], out_v=outs[1], out_gradients=outs[2:6],
                          out_score=outs[6], out_state=outs[7], record=rec)

    def snapshot():
        ctx.synchronize()
        return [q.download().tobytes() for q in outs] + [rec.download(16, 1).tobytes()]

    call()
    first = snapshot()
    assert np.frombuffer(first[8], SUBSET_DTYPE)["nodes"][0] == nw * nh
    for _ in range(2):
        for q in outs + [rec]:
            q.fill_bytes(0x3C)
        call()
        again = snapshot()
        # (beyond the grid the fill differs: compare the grids and the record)
        for a, b in zip(again[:8], first[:8]):
            ga, gb = np.frombuffer(a, U32).reshape(nh + 3, -1)[:nh, :nw], np.frombuffer(b, U32).reshape(nh + 3, -1)[:nh, :nw]
            assert np.array_equal(ga, gb)
        assert again[8] == first[8]
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    try:
        call()
    finally:
        graph = vp()
        assert lib.flow2d_capture_end(ctx.handle, ctypes.byref(graph)) == 0
    try:
        for fill in (0x7F, 0x11):
            for q in outs + [rec]:
                q.fill_bytes(fill)
            assert lib.flow2d_graph_launch(ctx.handle, graph) == 0
            replayed = snapshot()
            for a, b in zip(replayed[:8], first[:8]):
                ga, gb = np.frombuffer(a, U32).reshape(nh + 3, -1), np.frombuffer(b, U32).reshape(nh + 3, -1)
                assert np.array_equal(ga[:nh, :nw], gb[:nh, :nw]) and (ga[nh:] == U32(fill * 0x01010101)).all()
            assert replayed[8] == first[8]
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)
    release(ctx, frames + start + outs + [rec])


@pytest.mark.parametrize("kind", ["contiguous", "rows"])
def test_lock_step_batch(flow2d, ctx, kind):
    """Three instances `stride` apart with different frames and starts: planes and record of instance b are the bytes of that
    instance alone, and every other word of the output allocations is what it was."""
    w, h, cw, ch, count, r, s, R = 130, 37, 140, 40, 3, 5, 6, 5
    stride = stride_of(kind, pitch_of(cw), ch)
    cases = [speckle_case(w, h, r, s, motion=m, seed=b) for b, m in enumerate(("affine", "translation", "affine"))]
    cases[1][2][1, 3] = np.nan  # a node without input in one instance only
    nh, nw = cases[0][2].shape
    new = lambda: Tall(ctx, cw, ch, count, stride)  # noqa: E731
    t0, t1 = new().fill([c[0] for c in cases]), new().fill([c[1] for c in cases])
    tu, tv = new().fill([c[2] for c in cases]), new().fill([c[3] for c in cases])
    outs = [new() for _ in range(8)]
    rec = ctx.subset_records(count).fill_bytes(0x7F)
    with ctx.set_batch(count, stride):
        ctx.subset_refine(t0, t1, w, h, tu, tv, nw, nh, r, s, R, out_u=outs[0], out_v=outs[1], out_gradients=outs[2:6], out_score=outs[6],
                          out_state=outs[7], record=rec, instances=count)
    ctx.synchronize()
    alone = [run_subset(ctx, c[0], c[1], c[2], c[3], r, s, R) for c in cases]
    for k, tall in enumerate(outs):
        tall.check([a[0][k].view(F32) for a in alone], "%s (%s)" % (Refined.NAMES[k], kind))
    for tall in (t0, t1, tu, tv):
        tall.check(None, "inputs")
    raw = rec.download(16 * count, 1).tobytes()
    for b in range(count):
        assert raw[64 * b:64 * b + 64] == alone[b][1], "record of instance %d" % b
    assert np.frombuffer(raw, SUBSET_DTYPE)["no_input"].tolist() == [0, 1, 0]
    # ... and against the restatement
    for b, c in enumerate(cases):
        want, spread = all_orders(c[0], c[1], c[2], c[3], r, s, R)
        compare(alone[b], want, spread, "instance %d" % b)
    # a written range must not meet a later instance of an input
    lib = flow2d.hip_lib()
    with ctx.set_batch(count, stride):
        assert lib.flow2d_subset_refine_2d(ctx.handle, t0.ptr, t1.ptr, w, h, t0.pitch, tu.ptr, tv.ptr, nw, nh, tu.pitch, r, s, R, 20, 1e-3, 2.0, 0.5,
                                           tv.ptr + 2 * stride, outs[1].ptr, None, None, None, None, None, None, None) == 1
    ctx.synchronize()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing(flow2d, ctx):
    w, h, r, s, R = 100, 40, 7, 8, 7
    lib = flow2d.hip_lib()
    f0, f1, u0, v0 = speckle_case(w, h, r, s)
    nw, nh = grid(w, h, r, s)
    p0, p1, pu, pv = ctx.plane(w, h, f0), ctx.plane(w, h, f1), ctx.plane(nw, nh, u0), ctx.plane(nw, nh, v0)
    outs = [ctx.plane(nw, nh).fill_bytes(0x7F) for _ in range(8)]
    rec = ctx.subset_records().fill_bytes(0x7F)
    span = p0.pitch * h
    nan, inf = float("nan"), float("inf")
    names = ("u", "v", "ux", "uy", "vx", "vy", "score", "state")
    base = dict(f0=p0.ptr, f1=p1.ptr, w=w, h=h, pitch=p0.pitch, u0=pu.ptr, v0=pv.ptr, nw=nw, nh=nh, npitch=pu.pitch, r=r, s=s, R=R, K=20, eps=1e-3,
                shift=2.0, grad=0.5, record=rec.ptr, **{n: q.ptr for n, q in zip(names, outs)})

    def call(**kw):
        a = dict(base, **kw)
        return lib.flow2d_subset_refine_2d(ctx.handle, a["f0"], a["f1"], a["w"], a["h"], a["pitch"], a["u0"], a["v0"], a["nw"], a["nh"], a["npitch"],
                                           a["r"], a["s"], a["R"], a["K"], a["eps"], a["shift"], a["grad"], *[a[n] for n in names], a["record"])

    bad = [dict(f0=None), dict(f1=None), dict(u0=None), dict(v0=None), dict(u=None), dict(v=None), dict(w=0), dict(h=0), dict(nw=0), dict(nh=0),
           dict(pitch=p0.pitch + 8), dict(pitch=16), dict(npitch=16), dict(npitch=pu.pitch + 4), dict(r=0), dict(r=16), dict(s=0), dict(s=65),
           dict(R=0), dict(R=16), dict(K=0), dict(K=65), dict(eps=-1.0), dict(eps=nan), dict(eps=inf), dict(shift=0.0), dict(shift=nan),
           dict(shift=inf), dict(grad=0.0), dict(grad=-0.5), dict(grad=nan), dict(nw=nw + 1), dict(nh=nh + 1), dict(w=14), dict(h=14),
           dict(ux=None), dict(vy=None), dict(uy=None, vx=None), dict(u=p0.ptr), dict(v=p1.ptr + span - p0.pitch), dict(ux=pu.ptr), dict(vy=pv.ptr),
           dict(v=outs[0].ptr), dict(state=outs[6].ptr), dict(score=outs[2].ptr), dict(record=rec.ptr + 4), dict(record=p0.ptr + 64),
           dict(record=outs[0].ptr), dict(record=pu.ptr)]
    for kw in bad:
        assert call(**kw) == 1, kw
    ctx.synchronize()
    for q in outs:
        assert (q.download().view(U32) == POISON).all()
    assert set(rec.download(16, 1).tobytes()) == {0x7F}
    # ... and the same planes are accepted
    assert call() == 0
    ctx.synchronize()
    want, spread = all_orders(f0, f1, u0, v0, r, s, R)
    compare(([q.download(nw, nh).view(U32) for q in outs], rec.download(16, 1).tobytes()), want, spread, "accepted")
