"""flow2d_subset_refine_from_2d and flow2d_predict_nodes_2d on the device against their numpy restatements
(tests/test_subset_sequence_cpu.py); the layers above them are in tests/test_gpu_subset_sequence_host.py.
The refinement: states and records exactly, the float planes within max(one fp32 ulp, 16 x the spread of the restatement's three
summation orders on that input) -- the tolerance of tests/test_gpu_subset.py; each case prints what it found.  The prediction:
every byte.  Starts that come from a previous step, starts with NaN and with a gradient beyond max_gradient, no start planes at
all; a subset larger than the grid's windows; containers larger than the data with poisoned outputs; a lock-step batch of three
and a replayed graph for both entries."""
import ctypes

import numpy as np
import pytest

from test_correlate_cpu import F32, U32, bits, correlate_reference, frame_range, grid, scenes_module
from test_gpu_batch_kernels import Tall, pitch_of, stride_of
from test_gpu_multipass import POISON, padded, release
from test_gpu_subset import compare, run_subset
from test_subset_cpu import FLAT, NO_INPUT, STRAYED, SUBSET_DTYPE, Refined, subset_refine_reference
from test_subset_sequence_cpu import (PLANES, PREDICT_DTYPE, ROTATION, all_orders_from, first4, predict_passes, predict_reference,
                                      rotation_scenes)

pytestmark = pytest.mark.gpu
F64 = np.float64


# ---- the calls ------------------------------------------------------------------------------------------------------------------------
def run_from(ctx, f0, f1, start, r, s, R, K=20, epsilon=1e-3, max_shift=4.0, max_gradient=0.5, gradients=True, record=True):
    """(the eight planes' bits, record bytes) of one flow2d_subset_refine_from_2d call into poisoned outputs, which must stay
    poisoned beyond the grid; start = (u0, v0, ux0, uy0, vx0, vy0) or (u0, v0): no start planes.  Every plane lies in a container
    larger than its data (a padded node pitch), NaN beyond it."""
    h, w = f0.shape
    nh, nw = start[0].shape
    frames = [padded(ctx, f0), padded(ctx, f1)]
    held = [padded(ctx, q) for q in start]
    outs = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(8)]
    rec = ctx.subset_records().fill_bytes(0x7F)
    ctx.subset_refine_from(frames[0], frames[1], w, h, held[0], held[1], held[2:] if len(held) == 6 else None, nw, nh, r, s, R, K, epsilon,
                           max_shift, max_gradient, outs[0], outs[1], outs[2:6] if gradients else None, outs[6], outs[7], rec if record else None)
    ctx.synchronize()
    got = [q.download().view(U32) for q in outs]
    for k, g in enumerate(got):
        if gradients or not 2 <= k < 6:
            assert (g[nh:] == POISON).all() and (g[:, nw:] == POISON).all(), "written beyond the grid"
        else:
            assert (g == POISON).all(), "an absent plane was written"
    raw = rec.download(16, 1).tobytes()
    assert record or set(raw) == {0x7F}
    result = [g[:nh, :nw] if (gradients or not 2 <= k < 6) else None for k, g in enumerate(got)], (raw if record else None)
    release(ctx, frames + held + outs + [rec])
    return result


def check_from(ctx, f0, f1, start, r, s, R, what, **kw):
    want, spread = all_orders_from(f0, f1, start[0], start[1], start[2:], r, s, R, **kw)
    compare(run_from(ctx, f0, f1, start, r, s, R, **kw), want, spread, what)
    return want


def run_predict(ctx, nodes, state, s, min_state=1, min_neighbours=1, with_state=True, record=True):
    """(the six planes' bits and the state's -- None when absent --, record bytes) of one flow2d_predict_nodes_2d call."""
    nh, nw = state.shape
    held = [padded(ctx, q) for q in list(nodes) + [state]]
    outs = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(7)]
    rec = ctx.predict_records().fill_bytes(0x7F)
    ctx.predict_nodes(held[:6], held[6], nw, nh, s, min_state, min_neighbours, outs[:6], outs[6] if with_state else None, rec if record else None)
    ctx.synchronize()
    got = [q.download().view(U32) for q in outs]
    for g in got[:6]:
        assert (g[nh:] == POISON).all() and (g[:, nw:] == POISON).all(), "written beyond the grid"
    assert (got[6][nh:] == POISON).all() and (got[6][:, nw:] == POISON).all() if with_state else (got[6] == POISON).all()
    raw = rec.download(16, 1).tobytes()
    assert record or set(raw) == {0x7F}
    result = [g[:nh, :nw] for g in got[:6]] + [got[6][:nh, :nw] if with_state else None], (raw if record else None)
    release(ctx, held + outs + [rec])
    return result


def check_predict(ctx, nodes, state, s, what, **kw):
    want, want_state, record = predict_reference(nodes, state, s, kw.get("min_state", 1), kw.get("min_neighbours", 1))
    got, raw = run_predict(ctx, nodes, state, s, **kw)
    for name, g, w_plane in zip(PLANES, got, want):
        assert np.array_equal(g, bits(w_plane)), "%s: %s" % (what, name)
    if got[6] is not None:
        assert np.array_equal(got[6], bits(want_state)), "%s: state %s, want %s" % (what, got[6].view(F32), want_state)
    if raw is not None:
        assert raw == record.tobytes(), "%s: record %s, want %s" % (what, np.frombuffer(raw, PREDICT_DTYPE), record)
    return want, want_state, record


# ---- inputs: a previous step's result, restated once and shared ---------------------------------------------------------------------
_cases = {}


def affine_steps(w, h, r, s, R, d=4):
    """Frames 0, 1, 2 of the affine speckle sequence and step 1 restated: the search's nodes refined from zero gradients."""
    key = (w, h, r, s, R)
    if key not in _cases:
        seq = scenes_module().make_speckle_sequence("affine", 3, w, h, seed=0)
        f0, f1, f2 = seq.frames[0], seq.frames[1], seq.frames[2]
        lo, scale = frame_range(f0, f1)
        u0, v0, _, _, _ = correlate_reference(f0, f1, lo, scale, r, d, s)
        _cases[key] = (f0, f1, f2, subset_refine_reference(f0, f1, u0, v0, r, s, R))
    return _cases[key]


def start_of(step, s, fill=2):
    """The six start planes the sequence builds from a step's Refined."""
    nodes, _, _ = predict_passes([getattr(step, n) for n in PLANES], step.state, s, fill)
    return nodes


def counts(want):
    return {k: int(want.record[k][0]) for k in SUBSET_DTYPE.names[:7]}


# ---- flow2d_subset_refine_from_2d -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [3, 6])
def test_refine_from_a_previous_step_small(flow2d, ctx, R):
    """50 x 41 with the grid (3, s 5): nine nodes per row, no multiple of the waves; R = 6 > r: the border nodes' subsets leave
    frame 0, and the prediction refills them from inside."""
    f0, _, f2, first = affine_steps(50, 41, 3, 5, R)
    start = start_of(first, 5)
    assert start[0].shape == (7, 9) and np.abs(start[2]).max() > 0
    want = check_from(ctx, f0, f2, start, 3, 5, R, "50x41, R = %d, step 2" % R)
    assert counts(want)["converged"] >= 12 and (counts(want)["strayed"] >= 15 if R == 6 else True)


def test_refine_from_a_previous_step_of_the_rotation(flow2d, ctx):
    """96 x 80, r = R = 7, s = 8: step 2 of the rotation sequence (8 degrees against frame 0) from step 1 restated."""
    from test_subset_sequence_cpu import rotation_rows
    c = ROTATION
    _, steps = rotation_rows()
    scenes = rotation_scenes()
    start = start_of(steps[0], c["s"])
    want = check_from(ctx, scenes[1].frame_0, scenes[1].frame_1, start, c["r"], c["s"], c["R"], "96x80 rotation, step 2")
    assert counts(want)["converged"] >= 60


def test_refine_from_with_the_largest_subset(flow2d, ctx):
    """R = 15 > r = 7: two waves per workgroup, sixteen pixels per lane; only the inner nodes' subsets lie inside frame 0."""
    f0, _, f2, first = affine_steps(96, 80, 7, 8, 7)
    start = start_of(first, 8)
    want = check_from(ctx, f0, f2, start, 7, 8, 15, "96x80, R = 15 > r = 7")
    assert counts(want)["converged"] >= 20 and counts(want)["strayed"] >= 30


def test_refine_from_with_three_waves_per_workgroup(flow2d, ctx):
    """R = 11 > r = 7: 16 960 bytes of LDS per wave, so three waves per workgroup (node = blockIdx.x * 3 + wave); 99 nodes are 33
    full workgroups."""
    f0, _, f2, first = affine_steps(96, 80, 7, 8, 7)
    start = start_of(first, 8)
    want = check_from(ctx, f0, f2, start, 7, 8, 11, "96x80, R = 11 > r = 7")
    assert counts(want)["converged"] >= 30 and counts(want)["strayed"] >= 30


def test_starts_that_are_not_finite_or_beyond_the_bounds_come_back(flow2d, ctx):
    f0, _, f2, first = affine_steps(50, 41, 3, 5, 3)
    start = [q.copy() for q in start_of(first, 5)]
    start[2][1, 1] = 2.0                    # ux0 far beyond max_gradient
    start[5][1, 2] = -0.9
    start[3][2, 3], start[4][2, 4], start[0][2, 5], start[5][3, 1] = np.nan, np.inf, -np.inf, np.nan
    start[0][4, 4] = 1e30                   # out of frame 1
    start[3].view(U32)[3, 3] = 0x80000000   # -0 where the node strays by its u
    start[0][3, 3] = -400.0
    g0 = f0.copy()
    g0[8, 38] = np.nan                      # flat: the nodes whose window or stencil holds it
    want = check_from(ctx, g0, f2, start, 3, 5, 3, "NaN, Inf and gradients beyond the bound in the start")
    assert want.state[1, 1] == STRAYED and want.state[1, 2] == STRAYED and want.state[4, 4] == STRAYED and want.state[3, 3] == STRAYED
    assert all(want.state[at] == NO_INPUT for at in ((2, 3), (2, 4), (2, 5), (3, 1))) and (want.state == FLAT).sum() >= 1
    # (compare held the device to these bits: the whole start of a flat or strayed node)
    back = (want.state == FLAT) | (want.state == STRAYED)
    for name, plane in zip(PLANES, start):
        assert np.array_equal(bits(getattr(want, name))[back], bits(plane)[back]), name
    assert bits(want.uy)[3, 3] == 0x80000000


def test_without_start_planes_the_bytes_are_the_plain_entrys(flow2d, ctx):
    f0, f1, _, first = affine_steps(50, 41, 3, 5, 3)
    u0, v0 = first.u.copy(), first.v.copy()
    u0[2, 2], v0[0, 0] = np.nan, 1e30
    plain = run_subset(ctx, f0, f1, u0, v0, 3, 5, 3, max_shift=4.0)
    got = run_from(ctx, f0, f1, (u0, v0), 3, 5, 3)
    for name, a, b in zip(Refined.NAMES, got[0], plain[0]):
        assert np.array_equal(a, b), name
    assert got[1] == plain[1]
    # ... and zero start gradients differ from it in no byte either (the flat and strayed nodes' gradients are zero both ways)
    zero = np.zeros_like(u0)
    zeros = run_from(ctx, f0, f1, (u0, v0, zero, zero, zero, zero), 3, 5, 3)
    assert all(np.array_equal(a, b) for a, b in zip(zeros[0], plain[0])) and zeros[1] == plain[1]
    # the optional planes
    bare = run_from(ctx, f0, f1, (u0, v0, zero, zero, zero, zero), 3, 5, 3, gradients=False, record=False)
    assert np.array_equal(bare[0][0], plain[0][0]) and np.array_equal(bare[0][7], plain[0][7]) and bare[0][2] is None


# ---- flow2d_predict_nodes_2d ------------------------------------------------------------------------------------------------------------
def holed(step, seed=3):
    """A step's planes with what the prediction treats specially: lost patches, a NaN and an Inf inside converged nodes, states
    0 and NaN, signed zeros that tie."""
    rng = np.random.default_rng(seed)
    nodes, state = [getattr(step, n).copy() for n in PLANES], step.state.copy()
    nh, nw = state.shape
    state[rng.random((nh, nw)) < 0.25] = -3
    state[0, 0] = state[nh - 1, nw - 1] = state[0, nw - 1] = -2   # corners
    state[2:5, 2:5] = -3                                          # a hole one pass cannot fill
    for q in nodes:
        q[2:5, 2:5] = np.nan
    state[1, nw - 2], state[nh - 2, 1] = 0, np.nan
    nodes[3][1, 1], nodes[0][nh - 2, nw - 2] = np.nan, np.inf
    nodes[2][0, 1:4] = (-0.0, 0.0, -0.0)
    nodes[4][1, 0:3] = 0.0
    return nodes, state


@pytest.mark.parametrize("min_state", [0, 1])
@pytest.mark.parametrize("shape", ["50x41", "96x80"])
def test_prediction_bytes(flow2d, ctx, shape, min_state):
    first = affine_steps(50, 41, 3, 5, 3)[3] if shape == "50x41" else affine_steps(96, 80, 7, 8, 7)[3]
    s = 5 if shape == "50x41" else 8
    nodes, state = holed(first)
    for k in (1, 3, 8):
        _, want_state, record = check_predict(ctx, nodes, state, s, "%s, min_state %d, min_neighbours %d" % (shape, min_state, k),
                                              min_state=min_state, min_neighbours=k)
        print(shape, min_state, k, first4(record))
        assert record["kept"][0] >= 5 and (k == 8 or record["predicted"][0] >= 5) and (k == 1 or record["empty"][0] >= 1)
    # a second pass on the first one's output, and the state plane absent
    one, one_state, _ = predict_reference(nodes, state, s, min_state, 1)
    check_predict(ctx, one, one_state, s, "second pass", min_state=min_state)
    check_predict(ctx, nodes, state, s, "no state plane, no record", min_state=min_state, with_state=False, record=False)


def test_prediction_of_a_wide_grid(flow2d, ctx):
    """More than one workgroup in x and y (64 x 4 threads): 130 x 9 nodes of a made-up smooth field with holes."""
    rng = np.random.default_rng(11)
    nh, nw = 9, 130
    nodes = [(rng.standard_normal((nh, nw)) * sc).astype(F32) for sc in (3, 3, 0.05, 0.05, 0.05, 0.05)]
    state = np.where(rng.random((nh, nw)) < 0.4, -3, 7).astype(F32)
    _, _, record = check_predict(ctx, nodes, state, 8, "130x9", min_neighbours=2)
    assert record["predicted"][0] >= 100 and record["nodes"][0] == nh * nw


# ---- the same bytes: a lock-step batch, a replayed graph ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["contiguous", "rows"])
def test_lock_step_batch_of_three(flow2d, ctx, kind):
    """Three instances `stride` apart with different frames and starts: planes and records of instance b are the bytes of that
    instance alone, for both entries, and every other word of the output allocations is what it was."""
    w, h, cw, ch, count, r, s, R = 50, 41, 60, 44, 3, 3, 5, 3
    stride = stride_of(kind, pitch_of(cw), ch)
    f0, f1, f2, first = affine_steps(w, h, r, s, R)
    starts = [start_of(first, s), [q.copy() for q in start_of(first, s, 1)], start_of(first, s)]
    starts[1][2][1, 3] = np.nan  # a node without input in one instance only
    frames1 = [f2, f1, f2]
    nh, nw = first.state.shape
    new = lambda: Tall(ctx, cw, ch, count, stride)  # noqa: E731
    t0, t1 = new().fill([f0]), new().fill(frames1)
    tin = [new().fill([st[k] for st in starts]) for k in range(6)]
    outs = [new() for _ in range(8)]
    rec = ctx.subset_records(count).fill_bytes(0x7F)
    with ctx.set_batch(count, stride):
        ctx.subset_refine_from(t0, t1, w, h, tin[0], tin[1], tin[2:], nw, nh, r, s, R, out_u=outs[0], out_v=outs[1], out_gradients=outs[2:6],
                               out_score=outs[6], out_state=outs[7], record=rec, instances=count)
    ctx.synchronize()
    alone = [run_from(ctx, f0, frames1[b], starts[b], r, s, R) for b in range(count)]
    for k, tall in enumerate(outs):
        tall.check([a[0][k].view(F32) for a in alone], "%s (%s)" % (Refined.NAMES[k], kind))
    for tall in [t0, t1] + tin:
        tall.check(None, "inputs")
    raw = rec.download(16 * count, 1).tobytes()
    for b in range(count):
        assert raw[64 * b:64 * b + 64] == alone[b][1], "record of instance %d" % b
    assert np.frombuffer(raw, SUBSET_DTYPE)["no_input"].tolist() == [0, 1, 0]
    # the prediction: three different result fields
    fields = [holed(first, seed) for seed in (3, 4, 5)]
    pin = [new().fill([f[0][k] for f in fields]) for k in range(6)] + [new().fill([f[1] for f in fields])]
    pout = [new() for _ in range(7)]
    prec = ctx.predict_records(count).fill_bytes(0x7F)
    with ctx.set_batch(count, stride):
        ctx.predict_nodes(pin[:6], pin[6], nw, nh, s, 1, 2, pout[:6], pout[6], prec, instances=count)
    ctx.synchronize()
    single = [run_predict(ctx, f[0], f[1], s, 1, 2) for f in fields]
    for k, tall in enumerate(pout):
        tall.check([a[0][k].view(F32) for a in single], "prediction plane %d (%s)" % (k, kind))
    for tall in pin:
        tall.check(None, "inputs")
    raw = prec.download(16 * count, 1).tobytes()
    for b in range(count):
        assert raw[64 * b:64 * b + 64] == single[b][1], "prediction record of instance %d" % b
    # a written range must not meet a later instance of a start plane or of an input
    lib = flow2d.hip_lib()
    with ctx.set_batch(count, stride):
        assert lib.flow2d_subset_refine_from_2d(ctx.handle, t0.ptr, t1.ptr, w, h, t0.pitch, tin[0].ptr, tin[1].ptr, tin[2].ptr, tin[3].ptr,
                                                tin[4].ptr, tin[5].ptr, nw, nh, tin[0].pitch, r, s, R, 20, 1e-3, 4.0, 0.5, tin[4].ptr + 2 * stride,
                                                outs[1].ptr, None, None, None, None, None, None, None) == 1
        assert lib.flow2d_predict_nodes_2d(ctx.handle, *[q.ptr for q in pin], nw, nh, pin[0].pitch, s, 1, 2, *[q.ptr for q in pout[:5]],
                                           pin[6].ptr + 2 * stride, None, None) == 1
    ctx.synchronize()


def test_a_replayed_graph_gives_the_direct_calls_bytes(flow2d, ctx):
    """The prediction's two passes and the refinement from them captured as one graph: replayed into refilled outputs it gives
    the bytes of the direct calls, records included."""
    w, h, r, s, R = 50, 41, 3, 5, 3
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    f0, _, f2, first = affine_steps(w, h, r, s, R)
    nodes, state = holed(first)
    nh, nw = state.shape
    frames = [padded(ctx, f0), padded(ctx, f2)]
    held = [padded(ctx, q) for q in nodes + [state]]
    ping = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(7)]
    pong = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(7)]
    outs = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(8)]
    precs = [ctx.predict_records().fill_bytes(0x7F) for _ in range(2)]
    rec = ctx.subset_records().fill_bytes(0x7F)
    written = ping + pong + outs + precs + [rec]

    def call():
        ctx.predict_nodes(held[:6], held[6], nw, nh, s, 1, 1, ping[:6], ping[6], precs[0])
        ctx.predict_nodes(ping[:6], ping[6], nw, nh, s, 1, 1, pong[:6], pong[6], precs[1])
        ctx.subset_refine_from(frames[0], frames[1], w, h, pong[0], pong[1], pong[2:6], nw, nh, r, s, R, out_u=outs[0], out_v=outs[1],
                               out_gradients=outs[2:6], out_score=outs[6], out_state=outs[7], record=rec)

    def snapshot():
        ctx.synchronize()
        return [q.download().view(U32)[:nh, :nw].copy() for q in ping + pong + outs] + [q.download(16, 1).tobytes() for q in precs + [rec]]

    call()
    first_bytes = snapshot()
    assert np.frombuffer(first_bytes[-1], SUBSET_DTYPE)["nodes"][0] == nw * nh
    assert np.frombuffer(first_bytes[-3], PREDICT_DTYPE)["predicted"][0] >= 5
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    try:
        call()
    finally:
        graph = vp()
        assert lib.flow2d_capture_end(ctx.handle, ctypes.byref(graph)) == 0
    try:
        for fill in (0x7F, 0x11):
            for q in written:
                q.fill_bytes(fill)
            assert lib.flow2d_graph_launch(ctx.handle, graph) == 0
            replayed = snapshot()
            for a, b in zip(replayed, first_bytes):
                assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
            assert (outs[0].download().view(U32)[nh:] == U32(fill * 0x01010101)).all()
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)
    release(ctx, frames + held + written)


# ---- refusals on a real context -----------------------------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing(flow2d, ctx):
    w, h, r, s, R = 50, 41, 3, 5, 3
    lib = flow2d.hip_lib()
    f0, _, f2, first = affine_steps(w, h, r, s, R)
    start = start_of(first, s)
    nw, nh = grid(w, h, r, s)
    p0, p1 = ctx.plane(w, h, f0), ctx.plane(w, h, f2)
    pin = [ctx.plane(nw, nh, q) for q in start]
    outs = [ctx.plane(nw, nh).fill_bytes(0x7F) for _ in range(8)]
    rec = ctx.subset_records().fill_bytes(0x7F)
    ins = ("u0", "v0", "ux0", "uy0", "vx0", "vy0")
    names = ("u", "v", "ux", "uy", "vx", "vy", "score", "state")
    base = dict(record=rec.ptr, **{n: q.ptr for n, q in zip(ins, pin)}, **{n: q.ptr for n, q in zip(names, outs)})

    def call(**kw):
        a = dict(base, **kw)
        return lib.flow2d_subset_refine_from_2d(ctx.handle, p0.ptr, p1.ptr, w, h, p0.pitch, *[a[n] for n in ins], nw, nh, pin[0].pitch, r, s, R, 20,
                                                1e-3, 4.0, 0.5, *[a[n] for n in names], a["record"])

    bad = [dict(ux0=None), dict(vy0=None), dict(uy0=None, vx0=None), dict(ux0=None, uy0=None, vx0=None), dict(ux0=pin[2].ptr + 4),
           dict(u=pin[2].ptr), dict(vy=pin[5].ptr), dict(state=pin[3].ptr), dict(score=pin[4].ptr), dict(record=pin[2].ptr),
           dict(u=pin[0].ptr), dict(u0=None), dict(ux=None), dict(v=outs[0].ptr)]
    for kw in bad:
        assert call(**kw) == 1, kw
    ctx.synchronize()
    for q in outs:
        assert (q.download().view(U32) == POISON).all()
    assert set(rec.download(16, 1).tobytes()) == {0x7F}
    assert call() == 0  # ... and the same planes are accepted
    ctx.synchronize()
    want, spread = all_orders_from(f0, f2, start[0], start[1], start[2:], r, s, R)
    compare(([q.download(nw, nh).view(U32) for q in outs], rec.download(16, 1).tobytes()), want, spread, "accepted")
    # the prediction: in place is refused, nothing is written
    state = ctx.plane(nw, nh, first.state)
    pouts = [ctx.plane(nw, nh).fill_bytes(0x7F) for _ in range(7)]
    prec = ctx.predict_records().fill_bytes(0x7F)

    def predict(o=None, st=state.ptr, os_=pouts[6].ptr, record=prec.ptr, s_=s, low=1, k=1):
        o = o or [q.ptr for q in pouts[:6]]
        return lib.flow2d_predict_nodes_2d(ctx.handle, *[q.ptr for q in pin], st, nw, nh, pin[0].pitch, s_, low, k, *o, os_, record)

    in_place = [q.ptr for q in pin]
    twice = [q.ptr for q in pouts[:6]]
    twice[3] = twice[2]
    for kw in (dict(o=in_place), dict(o=twice), dict(os_=state.ptr), dict(os_=pouts[0].ptr), dict(st=None), dict(s_=0), dict(low=2), dict(k=0),
               dict(k=9), dict(record=prec.ptr + 4), dict(record=pin[0].ptr)):
        assert predict(**kw) == 1, kw
    ctx.synchronize()
    for q in pouts:
        assert (q.download().view(U32) == POISON).all()
    assert set(prec.download(16, 1).tobytes()) == {0x7F}
    assert predict() == 0
    ctx.synchronize()
