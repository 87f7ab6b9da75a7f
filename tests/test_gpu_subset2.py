"""flow2d_subset_refine2_2d on the device against its numpy restatement (tests/test_subset2_cpu.py) by test_gpu_subset.compare's
rule: states and records exactly, the float planes within max(one fp32 ulp, 16 x the spread of the restatement's three summation
orders on that input) -- the kernel sums in the restatement's "butterfly" order, so the bytes are expected to match and each case
prints whether they did.  A one-subset frame, subsets larger than the grid's windows, the largest subset (the largest LDS slice),
several workgroups with a surplus wave, a bending scene, starts with gradients and curvatures, every optional output absent in
turn with poisoned containers larger than the data, non-finite and huge starts, one and sixty-four iterations; the same bytes
from repeated calls, a replayed graph and an instance alone or in a lock-step batch; the refusals on a real context."""
import ctypes

import numpy as np
import pytest

from test_correlate_cpu import F32, U32, bits, correlate_reference, frame_range, grid, random_frames, scenes_module
from test_gpu_batch_kernels import Tall, pitch_of, stride_of
from test_gpu_multipass import POISON, padded, release
from test_gpu_subset import small_specimen, speckle_case
from test_subset2_cpu import CURVATURES, GRADIENTS, P_NAMES, Refined2, all_orders2
from test_subset_cpu import FLAT, NO_INPUT, STRAYED, SUBSET_DTYPE

pytestmark = pytest.mark.gpu
F64 = np.float64
# the fourteen planes in the entry's order: u, v, the gradients, the curvatures, score, state
OUT_NAMES = ("u", "v") + GRADIENTS + CURVATURES + ("score", "state")


def run_subset2(ctx, f0, f1, u0, v0, r, s, R, K=20, epsilon=1e-3, max_shift=2.0, max_gradient=0.5, max_curvature=0.05,
                start_gradients=None, start_curvatures=None, gradients=True, curvatures=True, score=True, state=True, record=True):
    """({name: bits, absent planes None}, record bytes or None) of one call into poisoned outputs, which must stay poisoned beyond
    the grid; frames and inputs lie in containers larger than the data, NaN beyond it."""
    h, w = f0.shape
    nh, nw = u0.shape
    frames = [padded(ctx, f0), padded(ctx, f1)]
    start = [padded(ctx, u0), padded(ctx, v0)]
    sg = [padded(ctx, q) for q in start_gradients] if start_gradients is not None else None
    sc = [padded(ctx, q) for q in start_curvatures] if start_curvatures is not None else None
    outs = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(14)]
    rec = ctx.subset_records().fill_bytes(0x7F)
    ctx.subset_refine2(frames[0], frames[1], w, h, start[0], start[1], nw, nh, r, s, R, K, epsilon, max_shift, max_gradient, max_curvature,
                       sg, sc, outs[0], outs[1], outs[2:6] if gradients else None, outs[6:12] if curvatures else None,
                       outs[12] if score else None, outs[13] if state else None, rec if record else None)
    ctx.synchronize()
    present = [True, True] + [gradients] * 4 + [curvatures] * 6 + [score, state]
    got = [q.download().view(U32) for q in outs]
    for g, there in zip(got, present):
        if there:
            assert (g[nh:] == POISON).all() and (g[:, nw:] == POISON).all(), "written beyond the grid"
        else:
            assert (g == POISON).all(), "an absent plane was written"
    raw = rec.download(16, 1).tobytes()
    assert record or set(raw) == {0x7F}
    result = {name: (g[:nh, :nw] if there else None) for name, g, there in zip(OUT_NAMES, got, present)}, (raw if record else None)
    release(ctx, frames + start + (sg or []) + (sc or []) + outs + [rec])
    return result


def compare2(got, want, spread, what):
    """The device's planes (bits by name) and record against the restatement `want` (Refined2); returns whether every byte matched."""
    planes, raw = got
    exact = True
    if planes["state"] is not None:
        assert np.array_equal(planes["state"], bits(want.state)), "%s: states %s, want %s" % (what, planes["state"].view(F32), want.state)
    if raw is not None:
        assert raw == want.record.tobytes(), "%s: record %s, want %s" % (what, np.frombuffer(raw, SUBSET_DTYPE), want.record)
    live = want.state >= 0
    worst = 0.0
    for name in P_NAMES + ("score",):
        g, w_plane = planes[name], getattr(want, name)
        if g is None:
            continue
        wbits = bits(w_plane)
        assert np.array_equal(g[~live], wbits[~live]), "%s: %s of a node that was not refined" % (what, name)
        same = g[live] == wbits[live]
        exact &= bool(same.all())
        tolerance = np.maximum(np.spacing(np.abs(w_plane[live])).astype(F64), 16.0 * spread)
        off = np.abs(g[live].view(F32).astype(F64) - w_plane[live].astype(F64))
        if not same.all():
            print("%s: %s: %d of %d words differ, largest difference %.3e" % (what, name, (~same).sum(), same.size, off.max()))
        worst = max(worst, float(off.max()) if off.size else 0.0)
        assert (off <= tolerance).all(), "%s: %s off by %.3e (allowed %.3e)" % (what, name, off.max(), tolerance[off.argmax()])
    print("%s: bytes %s (largest difference %.3e, spread %.3e)" % (what, "match" if exact else "DIFFER within the tolerance", worst, spread))
    return exact


def check_subset2(ctx, f0, f1, u0, v0, r, s, R, what, **kw):
    want, spread = all_orders2(f0, f1, u0, v0, r, s, R, **kw)
    compare2(run_subset2(ctx, f0, f1, u0, v0, r, s, R, **kw), want, spread, what)
    return want


def counts(want):
    return {k: int(want.record[k][0]) for k in SUBSET_DTYPE.names[:7]}


_shared = {}


def small_reference():
    """The 50 x 41 case at R = 3 and its restatement, made once and shared (read-only)."""
    if "small" not in _shared:
        f0, f1, u0, v0 = speckle_case(50, 41, 3, 5)
        _shared["small"] = (f0, f1, u0, v0) + all_orders2(f0, f1, u0, v0, 3, 5, 3)
    return _shared["small"]


# ---- shapes -------------------------------------------------------------------------------------------------------------------------
def test_one_subset_frame(flow2d, ctx):
    f0, _ = random_frames(5, 5, seed=2, shift=(0, 0))
    zero = np.zeros((1, 1), F32)
    want = check_subset2(ctx, f0, f0, zero, zero, 2, 2, 2, "5x5, f1 = f0")
    assert counts(want) == dict(nodes=1, converged=1, unconverged=0, strayed=0, flat=0, no_input=0, iterations=1)
    assert want.state[0, 0] == 1 and want.u[0, 0] == 0 and want.v[0, 0] == 0 and want.score[0, 0] == 1
    want = check_subset2(ctx, f0, f0, np.ones((1, 1), F32), zero, 2, 2, 2, "5x5, u0 = 1")
    assert want.state[0, 0] == STRAYED and counts(want)["iterations"] == 1 and want.u[0, 0] == 1


@pytest.mark.parametrize("R", [3, 6])
def test_subsets_at_and_beyond_the_grid_radius(flow2d, ctx, R):
    """50 x 41 with the grid (3, s 5): nine nodes per row, no multiple of the waves.  R = 6: the subsets of the first row and
    column leave frame 0."""
    f0, f1, u0, v0 = speckle_case(50, 41, 3, 5)
    assert u0.shape == (7, 9)
    want = check_subset2(ctx, f0, f1, u0, v0, 3, 5, R, "50x41, R = %d" % R)
    c = counts(want)
    assert c["converged"] >= 10 and (c["strayed"] >= 15 if R == 6 else True)


def test_largest_subset(flow2d, ctx):
    f0, f1, u0, v0 = speckle_case(97, 99, 15, 33, d=3)
    assert u0.shape == (3, 3)
    want = check_subset2(ctx, f0, f1, u0, v0, 15, 33, 15, "97x99, R = 15, N = 961")
    assert counts(want)["converged"] >= 1


@pytest.mark.parametrize("R", [10, 11, 12, 13, 15])
def test_the_large_radii(flow2d, ctx, R):
    """The radii around every change of the waves per workgroup: four at R = 10, three at 11 and 12 (node = blockIdx.x * 3 + wave),
    two from 13.  40 x 36: only the inner nodes' subsets lie inside frame 0, the others stray."""
    f0, f1, u0, v0 = small_specimen()
    assert u0.shape == (8, 9)
    want = check_subset2(ctx, f0, f1, u0, v0, 3, 4, R, "40x36 specimen, R = %d" % R)
    assert (want.state >= 0).sum() >= 1 and counts(want)["strayed"] >= 20


def test_several_workgroups(flow2d, ctx):
    f0, f1, u0, v0 = speckle_case(130, 37, 7, 8)
    assert u0.shape == (3, 15) and u0.size % 4 != 0
    want = check_subset2(ctx, f0, f1, u0, v0, 7, 8, 7, "130x37, (7, s 8)")
    assert counts(want)["converged"] >= 20


def test_a_bending_scene(flow2d, ctx):
    """The 4 x 3 corner of the grid (7, s 8) of the 96 x 80 "bend" scene at R = 7; the border nodes' samples leave frame 1."""
    scene = scenes_module().make_speckle_bending("bend")
    lo, scale = frame_range(scene.frame_0, scene.frame_1)
    u0, v0, _, _, _ = correlate_reference(scene.frame_0, scene.frame_1, lo, scale, 7, 6, 8)
    u0, v0 = np.ascontiguousarray(u0[:3, :4]), np.ascontiguousarray(v0[:3, :4])
    want = check_subset2(ctx, scene.frame_0, scene.frame_1, u0, v0, 7, 8, 7, "bend, 4 x 3 nodes")
    assert want.state[2, 3] >= 1 and abs(float(want.uxy[2, 3]) - 0.004) < 0.002 and abs(float(want.vxx[2, 3]) + 0.004) < 0.002


def test_starts_with_gradients_and_curvatures(flow2d, ctx):
    f0, f1, u0, v0 = speckle_case(50, 41, 3, 5)
    rng = np.random.default_rng(4)
    sg = [rng.uniform(-0.02, 0.02, u0.shape).astype(F32) for _ in range(4)]
    sc = [rng.uniform(-0.004, 0.004, u0.shape).astype(F32) for _ in range(6)]
    sc[1][2, 3] = 0.2  # beyond max_curvature: strays and comes back bit for bit
    with_gradients = check_subset2(ctx, f0, f1, u0, v0, 3, 5, 3, "start gradients", start_gradients=sg)
    assert counts(with_gradients)["converged"] >= 10
    want = check_subset2(ctx, f0, f1, u0, v0, 3, 5, 3, "start gradients and curvatures", start_gradients=sg, start_curvatures=sc)
    assert want.state[2, 3] == STRAYED and want.uxy[2, 3] == F32(0.2) and want.ux[2, 3] == sg[0][2, 3] and counts(want)["converged"] >= 10


def test_every_optional_output_absent_in_turn(flow2d, ctx):
    f0, f1, u0, v0, want, spread = small_reference()
    for absent in ("gradients", "curvatures", "score", "state", "record"):
        compare2(run_subset2(ctx, f0, f1, u0, v0, 3, 5, 3, **{absent: False}), want, spread, "without " + absent)
    compare2(run_subset2(ctx, f0, f1, u0, v0, 3, 5, 3, gradients=False, curvatures=False, score=False, state=False, record=False), want,
             spread, "u and v only")


def test_non_finite_and_huge_starts(flow2d, ctx):
    f0, f1, u0, v0 = speckle_case(50, 41, 3, 5)
    u0, v0, f0, f1 = u0.copy(), v0.copy(), f0.copy(), f1.copy()
    zero = np.zeros_like(u0)
    sg, sc = [zero.copy() for _ in range(4)], [zero.copy() for _ in range(6)]
    u0[1, 1], v0[2, 2], u0[3, 3], v0[4, 4], u0[5, 5] = np.nan, np.inf, 1e30, -3e38, -np.inf
    sg[2][1, 4], sc[5][2, 5], sc[0][3, 6], sg[1][4, 1] = np.nan, -np.inf, 1e30, 1e30
    f0[8, 38], f1[33, 8] = np.nan, np.inf
    want = check_subset2(ctx, f0, f1, u0, v0, 3, 5, 3, "non-finite and huge", start_gradients=sg, start_curvatures=sc)
    for node in ((1, 1), (2, 2), (5, 5), (1, 4), (2, 5)):
        assert want.state[node] == NO_INPUT
    for node in ((3, 3), (4, 4), (3, 6), (4, 1)):
        assert want.state[node] == STRAYED
    assert want.uxx[3, 6] == F32(1e30) and want.state[1, 7] == FLAT and want.state[6, 1] == FLAT
    want = check_subset2(ctx, np.full_like(f0, 9.0), f1, u0, v0, 3, 5, 3, "constant frame 0")
    assert counts(want)["flat"] == u0.size - counts(want)["no_input"] and counts(want)["no_input"] == 3


def test_one_and_sixty_four_iterations(flow2d, ctx):
    f0, f1, u0, v0 = speckle_case(50, 41, 3, 5)
    want = check_subset2(ctx, f0, f1, u0, v0, 3, 5, 3, "K = 1", K=1)
    assert counts(want)["iterations"] == u0.size
    u0, v0 = np.ascontiguousarray(u0[:4, :5]), np.ascontiguousarray(v0[:4, :5])  # (a corner: twenty nodes' 64 iterations restated)
    want = check_subset2(ctx, f0, f1, u0, v0, 3, 5, 3, "K = 64, epsilon 0", K=64, epsilon=0.0)
    c = counts(want)
    assert c["converged"] == 0 and c["unconverged"] >= 6 and c["iterations"] >= 64 * c["unconverged"]


def test_the_wrapper_allocates_and_downloads(flow2d, ctx):
    f0, f1, u0, v0, want, spread = small_reference()
    p0, p1, pu, pv = ctx.plane(50, 41, f0), ctx.plane(50, 41, f1), ctx.plane(9, 7, u0), ctx.plane(9, 7, v0)
    u, v, gradients, curvatures, score, state, rec = ctx.subset_refine2(p0, p1, 50, 41, pu, pv, 9, 7, 3, 5, 3)
    planes = dict(zip(OUT_NAMES, [bits(q) for q in (u, v) + gradients + curvatures + (score, state)]))
    compare2((planes, bytes(rec)), want, spread, "wrapper")
    assert rec.summary() == counts(want)


# ---- the same bytes -------------------------------------------------------------------------------------------------------------------
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
    outs = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(14)]
    rec = ctx.subset_records().fill_bytes(0x7F)

    def call():
        ctx.subset_refine2(frames[0], frames[1], w, h, start[0], start[1], nw, nh, r, s, R, out_u=outs[0], out_v=outs[1],
                           out_gradients=outs[2:6], out_curvatures=outs[6:12], out_score=outs[12], out_state=outs[13], record=rec)

    def snapshot():
        ctx.synchronize()
        return [q.download().view(U32) for q in outs] + [rec.download(16, 1).tobytes()]

    call()
    first = snapshot()
    assert np.frombuffer(first[14], SUBSET_DTYPE)["nodes"][0] == nw * nh
    for q in outs + [rec]:
        q.fill_bytes(0x3C)
    call()
    again = snapshot()
    for a, b in zip(again[:14], first[:14]):  # (beyond the grid the fill differs: compare the grids and the record)
        assert np.array_equal(a[:nh, :nw], b[:nh, :nw])
    assert again[14] == first[14]
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
            for a, b in zip(replayed[:14], first[:14]):
                assert np.array_equal(a[:nh, :nw], b[:nh, :nw]) and (a[nh:] == U32(fill * 0x01010101)).all()
            assert replayed[14] == first[14]
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)
    release(ctx, frames + start + outs + [rec])


def test_lock_step_batch(flow2d, ctx):
    """Three instances `stride` apart with different frames and starts: planes and record of instance b are the bytes of that
    instance alone, and every other word of the output allocations is what it was."""
    w, h, cw, ch, count, r, s, R = 130, 37, 140, 40, 3, 5, 6, 5
    stride = stride_of("rows", pitch_of(cw), ch)
    cases = [speckle_case(w, h, r, s, motion=m, seed=b) for b, m in enumerate(("affine", "translation", "affine"))]
    cases[1][2][1, 3] = np.nan  # a node without input in one instance only
    nh, nw = cases[0][2].shape
    new = lambda: Tall(ctx, cw, ch, count, stride)  # noqa: E731
    t0, t1 = new().fill([c[0] for c in cases]), new().fill([c[1] for c in cases])
    tu, tv = new().fill([c[2] for c in cases]), new().fill([c[3] for c in cases])
    outs = [new() for _ in range(14)]
    rec = ctx.subset_records(count).fill_bytes(0x7F)
    with ctx.set_batch(count, stride):
        ctx.subset_refine2(t0, t1, w, h, tu, tv, nw, nh, r, s, R, out_u=outs[0], out_v=outs[1], out_gradients=outs[2:6],
                           out_curvatures=outs[6:12], out_score=outs[12], out_state=outs[13], record=rec, instances=count)
    ctx.synchronize()
    alone = [run_subset2(ctx, c[0], c[1], c[2], c[3], r, s, R) for c in cases]
    for name, tall in zip(OUT_NAMES, outs):
        tall.check([a[0][name].view(F32) for a in alone], name)
    for tall in (t0, t1, tu, tv):
        tall.check(None, "inputs")
    raw = rec.download(16 * count, 1).tobytes()
    for b in range(count):
        assert raw[64 * b:64 * b + 64] == alone[b][1], "record of instance %d" % b
    assert np.frombuffer(raw, SUBSET_DTYPE)["no_input"].tolist() == [0, 1, 0]
    # a written range must not meet a later instance of an input
    lib = flow2d.hip_lib()
    with ctx.set_batch(count, stride):
        assert lib.flow2d_subset_refine2_2d(ctx.handle, t0.ptr, t1.ptr, w, h, t0.pitch, tu.ptr, tv.ptr, None, None, nw, nh, tu.pitch, r, s, R, 20,
                                            1e-3, 2.0, 0.5, 0.05, tv.ptr + 2 * stride, outs[1].ptr, None, None, None, None, None) == 1
    ctx.synchronize()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing(flow2d, ctx):
    w, h, r, s, R = 100, 40, 7, 8, 7
    lib = flow2d.hip_lib()
    f0, f1, u0, v0 = speckle_case(w, h, r, s)
    nw, nh = grid(w, h, r, s)
    p0, p1, pu, pv = ctx.plane(w, h, f0), ctx.plane(w, h, f1), ctx.plane(nw, nh, u0), ctx.plane(nw, nh, v0)
    zero = np.zeros_like(u0)
    sg, sc = [ctx.plane(nw, nh, zero).ptr for _ in range(4)], [ctx.plane(nw, nh, zero).ptr for _ in range(6)]
    outs = [ctx.plane(nw, nh).fill_bytes(0x7F) for _ in range(14)]
    rec = ctx.subset_records().fill_bytes(0x7F)
    nan, inf = float("nan"), float("inf")
    base = dict(f0=p0.ptr, f1=p1.ptr, w=w, h=h, pitch=p0.pitch, u0=pu.ptr, v0=pv.ptr, sg=sg, sc=sc, nw=nw, nh=nh, npitch=pu.pitch, r=r, s=s, R=R,
                K=20, eps=1e-3, shift=2.0, grad=0.5, curv=0.05, u=outs[0].ptr, v=outs[1].ptr, g=[q.ptr for q in outs[2:6]],
                c=[q.ptr for q in outs[6:12]], score=outs[12].ptr, state=outs[13].ptr, record=rec.ptr)

    def group(planes):
        return None if planes is None else (ctypes.c_void_p * len(planes))(*planes)

    def call(**kw):
        a = dict(base, **kw)
        return lib.flow2d_subset_refine2_2d(ctx.handle, a["f0"], a["f1"], a["w"], a["h"], a["pitch"], a["u0"], a["v0"], group(a["sg"]),
                                            group(a["sc"]), a["nw"], a["nh"], a["npitch"], a["r"], a["s"], a["R"], a["K"], a["eps"], a["shift"],
                                            a["grad"], a["curv"], a["u"], a["v"], group(a["g"]), group(a["c"]), a["score"], a["state"], a["record"])

    def without(planes, k, value=None):
        return planes[:k] + [value] + planes[k + 1:]

    bad = [dict(f0=None), dict(u0=None), dict(v=None), dict(w=0), dict(nh=0), dict(pitch=16), dict(npitch=16), dict(r=0), dict(s=65), dict(R=1),
           dict(R=16), dict(K=0), dict(K=65), dict(eps=nan), dict(shift=0.0), dict(grad=inf), dict(curv=0.0), dict(curv=nan), dict(curv=inf),
           dict(nw=nw + 1), dict(h=14), dict(g=without(base["g"], 2)), dict(c=without(base["c"], 5)), dict(sg=without(sg, 0)),
           dict(sc=without(sc, 3)), dict(sg=None), dict(u=p0.ptr), dict(c=without(base["c"], 1, p1.ptr)), dict(c=without(base["c"], 4, sc[4])),
           dict(g=without(base["g"], 0, sg[3])), dict(u=sc[0]), dict(score=outs[7].ptr), dict(c=without(base["c"], 0, outs[0].ptr)),
           dict(record=rec.ptr + 4), dict(record=outs[9].ptr), dict(record=sc[2])]
    for kw in bad:
        assert call(**kw) == 1, kw
    ctx.synchronize()
    for q in outs:
        assert (q.download().view(U32) == POISON).all()
    assert set(rec.download(16, 1).tobytes()) == {0x7F}
    # ... and the same planes are accepted
    assert call() == 0
    ctx.synchronize()
    want, spread = all_orders2(f0, f1, u0, v0, r, s, R, start_gradients=[zero] * 4, start_curvatures=[zero] * 6)
    compare2((dict(zip(OUT_NAMES, [q.download(nw, nh).view(U32) for q in outs])), rec.download(16, 1).tobytes()), want, spread, "accepted")
