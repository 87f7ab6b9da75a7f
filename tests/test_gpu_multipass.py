"""flow2d_correlate_offset_2d and flow2d_validate_nodes_2d on the device against their numpy restatement
(tests/test_multipass_cpu.py), bit for bit: a one-window frame whose offset leaves no candidate, a tiny dense grid, a predictor
with a step inside a workgroup's nodes and search areas partly outside frame 1 at each border, the limits of radius and range,
several workgroups with a node count that is no multiple of the waves, non-finite and huge predictor values, a NULL predictor
against Context.correlate, a minimum score; validation grids of one row, one column, one node, 2 x 2 and several workgroups, with
spikes and holes in both modes; containers larger than the data with poisoned outputs; the same bytes from a replayed graph and
from an instance alone or in a lock-step batch; the refusals on a real context; OpticalFlow.correlate_multipass_device against
its parts and the restatement's chain; the CLI."""
import ctypes
import json
import subprocess

import numpy as np
import pytest

from test_correlate_cpu import F32, NAN_BITS, U32, bits, correlate_reference, expand_reference, frame_range, grid, random_frames, scenes_module
from test_gpu_batch_kernels import Tall, pitch_of, stride_of
from test_multipass_cpu import (FLAG, PASS_DTYPE, REPLACE, VALIDATION_DTYPE, correlate_offset_reference, multipass_reference,
                                validate_reference)

pytestmark = pytest.mark.gpu
POISON = U32(0x7F7F7F7F)
WAVES = 4  # nodes per workgroup of correlate_offset_kernel (csrc/correlate_offset.hip, kOffsetWaves)


def padded(ctx, a, dw=5, dh=3, fill=np.nan):
    """`a` in a container dw columns wider and dh rows taller, the padding `fill`."""
    h, w = a.shape
    full = np.full((h + dh, w + dw), fill, F32)
    full[:h, :w] = a
    return ctx.plane(w + dw, h + dh, full)


def release(ctx, planes):
    for q in planes:
        q.free()
        ctx._planes.remove(q)


def run_offset(ctx, f0, f1, pred, r, d, s, lo=0.0, scale=1.0, cut=-1.0, score=True):
    """(u bits, v bits, score bits, record bytes) of one call into poisoned outputs, which must stay poisoned beyond the grid."""
    h, w = f0.shape
    nw, nh = grid(w, h, r, s)
    frames = [padded(ctx, f0), padded(ctx, f1)]
    predictor = [padded(ctx, p) for p in pred] if pred is not None else None
    nodes = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(3)]
    record = ctx.pass_records().fill_bytes(0x7F)
    ctx.correlate_offset(frames[0], frames[1], w, h, lo, scale, r, d, s, cut, predictor, nodes[0], nodes[1], nodes[2] if score else None, record)
    got = [q.download().view(U32) for q in nodes]
    for g in got[:3 if score else 2]:
        assert (g[nh:] == POISON).all() and (g[:, nw:] == POISON).all(), "written beyond the grid"
    if not score:
        assert (got[2] == POISON).all()
    result = [g[:nh, :nw] for g in got] + [record.download(16, 1).tobytes()]
    release(ctx, frames + (predictor or []) + nodes + [record])
    return result


def check_offset(ctx, f0, f1, pred, r, d, s, what, lo=0.0, scale=1.0, cut=-1.0):
    """One case against the restatement; returns the restatement's (u, v, score, record)."""
    wu, wv, ws, record = correlate_offset_reference(f0, f1, lo, scale, r, d, s, cut, *(pred if pred is not None else (None, None)))
    gu, gv, gs, grec = run_offset(ctx, f0, f1, pred, r, d, s, lo, scale, cut)
    for got, want, name in ((gu, wu, "u"), (gv, wv, "v"), (gs, ws, "score")):
        same = got == bits(want)
        assert same.all(), "%s: %s differs at %d places, first (y, x) = %s: %s, want %s" % (
            what, name, (~same).sum(), np.argwhere(~same)[0], got[~same][0].view(F32), bits(want)[~same][0].view(F32))
    assert grec == record.tobytes(), "%s: record %s, want %s" % (what, np.frombuffer(grec, PASS_DTYPE), record)
    return wu, wv, ws, record[0]


def constant(shape, a, b):
    return np.full(shape, a, F32), np.full(shape, b, F32)


# ---- flow2d_correlate_offset_2d ---------------------------------------------------------------------------------------------------
def test_one_window_frame_pushed_out_by_its_offset(flow2d, ctx):
    f0, f1 = random_frames(7, 7, seed=2, shift=(0, 0))
    _, _, _, rec = check_offset(ctx, f0, f1, constant((7, 7), 0.0, 0.0), 3, 2, 3, "7x7, offset 0")
    assert [int(rec[k]) for k in PASS_DTYPE.names[:6]] == [1, 0, 0, 1, 0, 1]
    for a, b in ((3.0, 0.0), (0.0, -3.0), (-2.6, 2.5), (1e30, 0.0), (40000.0, -40000.0)):
        wu, _, ws, rec = check_offset(ctx, f0, f1, constant((7, 7), a, b), 3, 2, 3, "7x7, offset (%g, %g)" % (a, b))
        assert [int(rec[k]) for k in PASS_DTYPE.names[:6]] == [1, 1, 0, 0, 0, 0] and np.isnan(wu[0, 0]) and ws[0, 0] == 0
    # an offset of one pixel with a range of two: one candidate row or column is left
    _, _, _, rec = check_offset(ctx, f0, f1, constant((7, 7), 1.0, -1.0), 3, 2, 3, "7x7, offset (1, -1)")
    assert rec["invalid"] == 0 and rec["candidates"] == 1 and rec["unrefined"] == 1


def test_tiny_dense_grid(flow2d, ctx):
    f0, f1 = random_frames(9, 7, seed=5, shift=(1, 0))
    _, _, _, rec = check_offset(ctx, f0, f1, None, 1, 1, 1, "9x7 dense, no predictor")
    assert rec["nodes"] == 7 * 5
    rng = np.random.default_rng(3)
    pred = (rng.uniform(-2.4, 2.4, (7, 9)).astype(F32), rng.uniform(-2.4, 2.4, (7, 9)).astype(F32))
    _, _, _, rec = check_offset(ctx, f0, f1, pred, 1, 1, 1, "9x7 dense, random predictor")
    assert rec["nodes"] == 35 and rec["unpredicted"] == 0


@pytest.mark.parametrize("towards", ["left", "right", "top", "bottom"])
def test_step_predictor_inside_a_workgroup(flow2d, ctx, towards):
    """50 x 41, (3, 4, 5): nine nodes per row, so a workgroup of four consecutive nodes straddles the predictor's step at x = 24
    (between node columns 4 and 5) in every row; beyond the step the offset points at a border, with part of the search area --
    and for the outermost nodes all of it -- outside frame 1."""
    w, h, r, d, s = 50, 41, 3, 4, 5
    f0, f1 = random_frames(w, h, seed=17, shift=(2, -1))
    nw, nh = grid(w, h, r, s)
    assert nw == 9 and nw % WAVES != 0
    pu, pv = np.full((h, w), 2.0, F32), np.full((h, w), -1.0, F32)
    far = {"left": (-30.0, 0.0), "right": (15.5, 1.0), "top": (0.0, -19.0), "bottom": (-1.0, 21.25)}[towards]
    if towards in ("left", "right"):
        pu[:, 24:], pv[:, 24:] = far
    else:
        pu[:, :24], pv[:, :24] = far
    wu, wv, _, rec = check_offset(ctx, f0, f1, (pu, pv), r, d, s, "step towards the %s" % towards)
    assert 0 < rec["invalid"] < rec["nodes"] and rec["unpredicted"] == 0
    found = np.isfinite(wu)
    near = found[:, :5] if towards in ("left", "right") else found[:, 5:]
    assert near.all() and not found.all()


def test_limits_of_radius_and_range(flow2d, ctx):
    w, h, r, d, s = 97, 99, 15, 32, 33
    f0, f1 = random_frames(w, h, seed=23, shift=(4, 3))
    assert grid(w, h, r, s) == (3, 3)
    pu, pv = np.zeros((h, w), F32), np.zeros((h, w), F32)
    pu[:, 40:], pv[50:, :] = 30.0, -28.0
    pu[:20, :20], pv[:20, :20] = -9.5, 6.5
    _, _, _, rec = check_offset(ctx, f0, f1, (pu, pv), r, d, s, "r 15, d 32")
    assert rec["nodes"] == 9 and rec["invalid"] == 0 and rec["candidates"] > 9 * 100


@pytest.mark.parametrize("r,d,s", [(7, 8, 8), (4, 3, 1)])
def test_several_workgroups(flow2d, ctx, r, d, s):
    w, h = 130, 37
    f0, f1 = random_frames(w, h, seed=7, shift=(3, -2))
    nw, nh = grid(w, h, r, s)
    assert nw * nh > 3 * WAVES and (nw * nh) % WAVES != 0
    y, x = np.mgrid[0:h, 0:w]
    pred = ((3 + 2.7 * np.sin(x / 9.0)).astype(F32), (-2 + 2.2 * np.cos(y / 5.0 + x / 31.0)).astype(F32))
    wu, _, _, rec = check_offset(ctx, f0, f1, pred, r, d, s, "130x37 (%d, %d, %d)" % (r, d, s))
    assert rec["nodes"] == nw * nh and np.rint(np.nanmedian(wu)) == 3


def test_non_finite_predictor(flow2d, ctx):
    w, h, r, d, s = 70, 33, 3, 4, 3
    f0, f1 = random_frames(w, h, seed=12)
    rng = np.random.default_rng(2)
    pu, pv = rng.uniform(-3, 3, (h, w)).astype(F32), rng.uniform(-3, 3, (h, w)).astype(F32)
    cx, cy = r + np.arange(0, 22) * s, r + np.arange(0, 9) * s
    for k, value in enumerate((np.nan, np.inf, -np.inf, 1e30, -1e30, 32767.4, -32768.6)):
        pu[cy[k % 9], cx[(3 * k) % 22]] = value
        pv[cy[(k + 4) % 9], cx[(5 * k + 1) % 22]] = value
    _, _, _, rec = check_offset(ctx, f0, f1, (pu, pv), r, d, s, "non-finite predictor")
    assert rec["unpredicted"] == 6 and rec["invalid"] == 8  # NaN and the infinities; the huge finite ones leave no candidate
    # a wholly NaN predictor is the search without one, with every node counted
    none = check_offset(ctx, f0, f1, None, r, d, s, "no predictor")
    wu, wv, ws, rec = check_offset(ctx, f0, f1, constant((h, w), np.nan, 1.0), r, d, s, "NaN predictor")
    assert rec["unpredicted"] == rec["nodes"] and np.array_equal(bits(wu), bits(none[0])) and np.array_equal(bits(ws), bits(none[2]))


@pytest.mark.parametrize("w,h,r,d,s", [(130, 37, 5, 4, 6), (65, 17, 2, 3, 1)])
def test_null_predictor_gives_the_single_pass_bytes(flow2d, ctx, w, h, r, d, s):
    f0, f1 = random_frames(w, h, seed=31, shift=(-1, 2))
    f0[6:24, 30:60] = 50.0
    gu, gv, gs, grec = run_offset(ctx, f0, f1, None, r, d, s, cut=0.3)
    p0, p1 = padded(ctx, f0), padded(ctx, f1)
    cu, cv, cs, crec = ctx.correlate(p0, p1, w, h, 0.0, 1.0, r, d, s, 0.3)
    assert np.array_equal(gu, bits(cu)) and np.array_equal(gv, bits(cv)) and np.array_equal(gs, bits(cs))
    assert grec[:32] == bytes(crec) and crec.invalid > 0
    wu, wv, ws, wrec, _ = correlate_reference(f0, f1, 0.0, 1.0, r, d, s, 0.3)
    assert np.array_equal(gu, bits(wu)) and np.array_equal(gs, bits(ws)) and grec[:32] == wrec.tobytes() and grec[48:] == bytes(16)


def test_min_score_rejects_some_nodes(flow2d, ctx):
    f0, f1 = random_frames(90, 50, seed=9, noise=60.0)
    pred = constant((50, 90), 1.6, -1.2)
    _, _, ws, _ = check_offset(ctx, f0, f1, pred, 3, 3, 4, "no minimum")
    cut = float(np.median(ws))
    wu, _, _, rec = check_offset(ctx, f0, f1, pred, 3, 3, 4, "minimum %g" % cut, cut=cut)
    assert 0 < rec["rejected"] < rec["nodes"] and rec["invalid"] == 0 and np.isnan(wu).sum() == rec["rejected"]
    _, _, _, rec = check_offset(ctx, f0, f1, pred, 3, 3, 4, "minimum 2", cut=2.0)
    assert rec["rejected"] == rec["nodes"] and rec["unrefined"] == 0
    a, b = run_offset(ctx, f0, f1, pred, 3, 3, 4, cut=cut), run_offset(ctx, f0, f1, pred, 3, 3, 4, cut=cut, score=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3]
    # a scale and lo that are no round numbers
    check_offset(ctx, f0, f1, pred, 3, 3, 4, "scaled", lo=-3.7, scale=0.913)


# ---- flow2d_validate_nodes_2d -------------------------------------------------------------------------------------------------------
def run_validate(ctx, nu, nv, mode, threshold=2.0, epsilon=0.1, k=3, flag=True):
    nh, nw = nu.shape
    ins = [padded(ctx, nu), padded(ctx, nv)]
    outs = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(3)]
    record = ctx.pass_records().fill_bytes(0x7F)
    ctx.validate_nodes(ins[0], ins[1], nw, nh, threshold, epsilon, k, mode, outs[0], outs[1], outs[2] if flag else None, record)
    got = [q.download().view(U32) for q in outs]
    for g in got[:3 if flag else 2]:
        assert (g[nh:] == POISON).all() and (g[:, nw:] == POISON).all(), "written beyond the grid"
    if not flag:
        assert (got[2] == POISON).all()
    result = [g[:nh, :nw] for g in got] + [record.download(16, 1).tobytes()]
    release(ctx, ins + outs + [record])
    return result


def check_validate(ctx, nu, nv, mode, what, **kw):
    wu, wv, wf, record = validate_reference(nu, nv, kw.get("threshold", 2.0), kw.get("epsilon", 0.1), kw.get("k", 3), mode)
    gu, gv, gf, grec = run_validate(ctx, nu, nv, mode, **kw)
    for got, want, name in ((gu, wu, "u"), (gv, wv, "v"), (gf, wf, "flag"))[:3 if kw.get("flag", True) else 2]:
        same = got == bits(want)
        assert same.all(), "%s: %s differs at %d places, first (y, x) = %s" % (what, name, (~same).sum(), np.argwhere(~same)[0])
    assert grec == record.tobytes(), "%s: record %s, want %s" % (what, np.frombuffer(grec, VALIDATION_DTYPE), record)
    return wu, wv, wf, record[0]


def node_field(nw, nh, seed):
    """A smooth field with spikes, holes (NaN, inf, one component only), signed zeros and a cluster of holes."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:nh, 0:nw]
    u = (1.5 + 0.05 * x - 0.03 * y + rng.normal(0, 0.02, (nh, nw))).astype(F32)
    v = (-0.5 + 0.04 * y + rng.normal(0, 0.02, (nh, nw))).astype(F32)
    n = nw * nh
    flat_u, flat_v = u.reshape(-1), v.reshape(-1)
    for k, at in enumerate(rng.choice(n, max(n // 6, 1), replace=False)):
        kind = k % 6
        if kind == 0:
            flat_u[at] += 7.0
        elif kind == 1:
            flat_v[at] -= 4.0
        elif kind == 2:
            flat_u[at] = flat_v[at] = np.nan
        elif kind == 3:
            flat_u[at] = np.inf
        elif kind == 4:
            flat_v[at] = -0.0
            flat_u[at] = 0.0
        else:
            flat_v[at] = np.nan
    if nw >= 6 and nh >= 4:
        u[1:4, 2:5] = np.nan  # a hole whose middle node has no neighbour
    return u, v


@pytest.mark.parametrize("nw,nh", [(1, 1), (9, 1), (1, 9), (2, 2), (70, 5), (13, 21)])
@pytest.mark.parametrize("mode", [FLAG, REPLACE])
def test_validation_grids(flow2d, ctx, nw, nh, mode):
    u, v = node_field(nw, nh, seed=nw + 3 * nh)
    if (nw, nh) == (2, 2):
        u[:, :], v[:, :] = 1.0, 2.0
        u[1, 1] = 60.0  # k = 3: judged, an outlier
    _, _, wf, rec = check_validate(ctx, u, v, mode, "%dx%d mode %d" % (nw, nh, mode))
    assert rec["nodes"] == nw * nh
    if min(nw, nh) == 1:
        assert rec["unjudged"] == nw * nh and wf.sum() == 0  # a row or column has at most two neighbours
    if (nw, nh) == (2, 2):
        assert rec["outliers"] == 1 and rec["judged"] == 4
    if nw * nh > 256:
        assert rec["outliers"] > 0 and (rec["filled"] > 0) == (mode == REPLACE) and rec["unjudged"] > 0
    # fewer neighbours asked for, another threshold and epsilon; without the flag plane
    check_validate(ctx, u, v, mode, "%dx%d k 1" % (nw, nh), k=1, threshold=1.25, epsilon=0.03)
    check_validate(ctx, u, v, mode, "%dx%d k 8" % (nw, nh), k=8, flag=False)


def test_validation_of_an_all_nan_grid_and_of_signed_zeros(flow2d, ctx):
    nan = np.full((6, 7), np.nan, F32)
    nan[2, 2] = -np.nan
    for mode in (FLAG, REPLACE):
        wu, _, _, rec = check_validate(ctx, nan, nan, mode, "all NaN")
        assert rec["unjudged"] == 42 and rec["remaining_invalid"] == 42 and np.array_equal(bits(wu), bits(nan))
    # medians of signed zeros: the key order decides which zero a hole gets
    z = np.zeros((3, 3), F32)
    z[0, :] = -0.0
    z[1, 0] = -0.0
    z[1, 1] = np.nan
    wu, _, _, _ = check_validate(ctx, z, -z, REPLACE, "signed zeros")
    assert bits(wu[1, 1]) == bits(F32(0.0))  # four -0, four +0: (-0 + +0) * 0.5


# ---- graph and batch ----------------------------------------------------------------------------------------------------------------
def test_a_replayed_graph_gives_the_eager_bytes(flow2d, ctx):
    w, h, r, d, s = 130, 37, 4, 5, 3
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    f0, f1 = random_frames(w, h, seed=21)
    y, x = np.mgrid[0:h, 0:w]
    pred = ((2.5 * np.sin(x / 7.0)).astype(F32), (2.5 * np.cos(y / 4.0)).astype(F32))
    pred[0][5:9, 40:60] = np.nan
    nw, nh = grid(w, h, r, s)
    wu, wv, ws, wrec = correlate_offset_reference(f0, f1, 0.0, 1.0, r, d, s, 0.2, *pred)
    vu, vv, vf, vrec = validate_reference(wu, wv, 2.0, 0.1, 3, REPLACE)
    frames, predictor = [padded(ctx, f0), padded(ctx, f1)], [padded(ctx, p) for p in pred]
    nodes = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(6)]
    records = [ctx.pass_records().fill_bytes(0x7F) for _ in range(2)]

    def both():
        ctx.correlate_offset(frames[0], frames[1], w, h, 0.0, 1.0, r, d, s, 0.2, predictor, nodes[0], nodes[1], nodes[2], records[0])
        ctx.validate_nodes(nodes[0], nodes[1], nw, nh, 2.0, 0.1, 3, REPLACE, nodes[3], nodes[4], nodes[5], records[1])

    def matches():
        got = [q.download(nw, nh).view(U32) for q in nodes]
        for g, want in zip(got, (wu, wv, ws, vu, vv, vf)):
            assert np.array_equal(g, bits(want))
        assert records[0].download(16, 1).tobytes() == wrec.tobytes() and records[1].download(16, 1).tobytes() == vrec.tobytes()

    both()
    ctx.synchronize()
    matches()
    for q in nodes + records:
        q.fill_bytes(0x7F)
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    try:
        both()
    finally:
        graph = vp()
        assert lib.flow2d_capture_end(ctx.handle, ctypes.byref(graph)) == 0
    try:
        ctx.synchronize()
        assert (nodes[0].download().view(U32) == POISON).all() and set(records[1].download(16, 1).tobytes()) == {0x7F}  # captured, not run
        for _ in range(2):
            for q in nodes + records:
                q.fill_bytes(0x3C)
            assert lib.flow2d_graph_launch(ctx.handle, graph) == 0
            ctx.synchronize()
            matches()
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)


@pytest.mark.parametrize("kind", ["contiguous", "rows"])
def test_lock_step_batch(flow2d, ctx, kind):
    """Three instances `stride` apart with different frames and predictors: node planes, validated planes and records of
    instance b are the restatement's for that instance alone, and every other word of the output allocations is what it was."""
    w, h, cw, ch, count, r, d, s = 130, 37, 140, 40, 3, 5, 4, 6
    stride = stride_of(kind, pitch_of(cw), ch)
    pairs = [random_frames(w, h, seed=30 + b, shift=(b - 1, 1)) for b in range(count)]
    pairs[1][0][6:24, 30:60] = 50.0  # invalid nodes in one instance only
    y, x = np.mgrid[0:h, 0:w]
    preds = [((b - 1 + 1.4 * np.sin(x / (5.0 + b))).astype(F32), (1 + (b - 1) * 1.3 * np.cos(y / 6.0)).astype(F32)) for b in range(count)]
    preds[2][1][10:14, 70:90] = np.inf
    nw, nh = grid(w, h, r, s)
    new = lambda: Tall(ctx, cw, ch, count, stride)  # noqa: E731
    t0, t1 = new().fill([p[0] for p in pairs]), new().fill([p[1] for p in pairs])
    tu, tv = new().fill([p[0] for p in preds]), new().fill([p[1] for p in preds])
    nu, nv, ns, ou, ov, of = (new() for _ in range(6))
    records = [ctx.pass_records(count).fill_bytes(0x7F) for _ in range(2)]
    with ctx.set_batch(count, stride):
        ctx.correlate_offset(t0, t1, w, h, 0.0, 1.0, r, d, s, 0.3, (tu, tv), nu, nv, ns, records[0], instances=count)
        ctx.validate_nodes(nu, nv, nw, nh, 2.0, 0.1, 3, REPLACE, ou, ov, of, records[1], instances=count)
    ctx.synchronize()
    refs = [correlate_offset_reference(p[0], p[1], 0.0, 1.0, r, d, s, 0.3, *q) for p, q in zip(pairs, preds)]
    vals = [validate_reference(ref[0], ref[1], 2.0, 0.1, 3, REPLACE) for ref in refs]
    for tall, k, name in ((nu, 0, "node u"), (nv, 1, "node v"), (ns, 2, "node score")):
        tall.check([ref[k] for ref in refs], "%s (%s)" % (name, kind))
    for tall, k, name in ((ou, 0, "validated u"), (ov, 1, "validated v"), (of, 2, "flag")):
        tall.check([val[k] for val in vals], "%s (%s)" % (name, kind))
    for tall in (t0, t1, tu, tv):
        tall.check(None, "inputs")
    got = [q.download(16 * count, 1).tobytes() for q in records]
    assert refs[1][3]["invalid"][0] > 0 and refs[0][3]["invalid"][0] == 0 and refs[2][3]["unpredicted"][0] > 0
    for b in range(count):
        assert got[0][64 * b:64 * b + 64] == refs[b][3].tobytes(), "pass record of instance %d" % b
        assert got[1][64 * b:64 * b + 64] == vals[b][3].tobytes(), "validation record of instance %d" % b
        alone = run_offset(ctx, pairs[b][0], pairs[b][1], preds[b], r, d, s, cut=0.3)
        assert np.array_equal(alone[0], bits(refs[b][0])) and np.array_equal(alone[2], bits(refs[b][2])) and alone[3] == got[0][64 * b:64 * b + 64]
    # a written range must not meet a later instance of a predictor, nor an output an input
    lib = flow2d.hip_lib()
    with ctx.set_batch(count, stride):
        assert lib.flow2d_correlate_offset_2d(ctx.handle, t0.ptr, t1.ptr, tu.ptr, tv.ptr, w, h, t0.pitch, 0.0, 1.0, r, d, s, -1.0,
                                              tv.ptr + 2 * stride, nv.ptr, ns.ptr, nu.pitch, records[0].ptr) == 1
        assert lib.flow2d_validate_nodes_2d(ctx.handle, nu.ptr, nv.ptr, nw, nh, nu.pitch, 2.0, 0.1, 3, REPLACE, ou.ptr, nv.ptr + stride, None,
                                            records[1].ptr) == 1
    ctx.synchronize()


def test_invalid_arguments_write_nothing(flow2d, ctx):
    w, h, r, d, s = 100, 40, 7, 8, 8
    lib = flow2d.hip_lib()
    f0, f1 = random_frames(w, h, seed=5)
    pred = constant((h, w), 1.0, -2.0)
    p0, p1, pu, pv = ctx.plane(w, h, f0), ctx.plane(w, h, f1), ctx.plane(w, h, pred[0]), ctx.plane(w, h, pred[1])
    nw, nh = grid(w, h, r, s)
    nu, nv, ns, ou, ov, of = (ctx.plane(nw, nh).fill_bytes(0x7F) for _ in range(6))
    records = [ctx.pass_records().fill_bytes(0x7F) for _ in range(2)]
    span = p0.pitch * h
    nan, inf = float("nan"), float("inf")
    base = dict(f0=p0.ptr, f1=p1.ptr, pu=pu.ptr, pv=pv.ptr, w=w, h=h, pitch=p0.pitch, lo=0.0, scale=1.0, r=r, d=d, s=s, cut=-1.0, nu=nu.ptr,
                nv=nv.ptr, ns=ns.ptr, npitch=nu.pitch, record=records[0].ptr)

    def call(**kw):
        a = dict(base, **kw)
        return lib.flow2d_correlate_offset_2d(ctx.handle, a["f0"], a["f1"], a["pu"], a["pv"], a["w"], a["h"], a["pitch"], a["lo"], a["scale"],
                                              a["r"], a["d"], a["s"], a["cut"], a["nu"], a["nv"], a["ns"], a["npitch"], a["record"])

    bad = [dict(r=0), dict(r=16), dict(d=0), dict(d=33), dict(s=0), dict(s=65), dict(scale=0.0), dict(scale=nan), dict(scale=inf), dict(lo=nan),
           dict(cut=nan), dict(f0=None), dict(f1=None), dict(nu=None), dict(nv=None), dict(w=0), dict(h=0), dict(w=14), dict(h=14),
           dict(pitch=p0.pitch + 8), dict(pitch=16), dict(npitch=16), dict(npitch=nu.pitch + 4), dict(nu=p0.ptr), dict(nv=p1.ptr + span - p0.pitch),
           dict(nv=nu.ptr), dict(ns=nv.ptr), dict(record=records[0].ptr + 4), dict(record=p0.ptr + 64), dict(record=nu.ptr),
           dict(pu=None), dict(pv=None), dict(pu=pu.ptr + 4), dict(nu=pu.ptr), dict(nv=pv.ptr + span - p0.pitch), dict(ns=pu.ptr + p0.pitch),
           dict(record=pv.ptr + 64)]
    for kw in bad:
        assert call(**kw) == 1, kw

    vbase = dict(nu=nu.ptr, nv=nv.ptr, nw=nw, nh=nh, npitch=nu.pitch, t=2.0, eps=0.1, k=3, mode=REPLACE, ou=ou.ptr, ov=ov.ptr, flag=of.ptr,
                 record=records[1].ptr)

    def validate(**kw):
        a = dict(vbase, **kw)
        return lib.flow2d_validate_nodes_2d(ctx.handle, a["nu"], a["nv"], a["nw"], a["nh"], a["npitch"], a["t"], a["eps"], a["k"], a["mode"],
                                            a["ou"], a["ov"], a["flag"], a["record"])

    for kw in [dict(nu=None), dict(nv=None), dict(ou=None), dict(ov=None), dict(nw=0), dict(nh=0), dict(npitch=16), dict(k=0), dict(k=9),
               dict(t=0.0), dict(t=nan), dict(t=inf), dict(eps=0.0), dict(eps=nan), dict(eps=-1.0), dict(mode=2), dict(mode=-1), dict(ou=nu.ptr),
               dict(ov=nv.ptr), dict(ov=ou.ptr), dict(flag=nu.ptr), dict(flag=ov.ptr), dict(record=records[1].ptr + 4), dict(record=nu.ptr),
               dict(record=ou.ptr)]:
        assert validate(**kw) == 1, kw
    ctx.synchronize()
    for q in (nu, nv, ns, ou, ov, of):
        assert (q.download().view(U32) == POISON).all()
    for q in records:
        assert set(q.download(16, 1).tobytes()) == {0x7F}
    # ... and the same planes are accepted
    assert call() == 0 and validate() == 0
    wu, wv, ws, wrec = correlate_offset_reference(f0, f1, 0.0, 1.0, r, d, s, -1.0, *pred)
    vu, vv, vf, vrec = validate_reference(wu, wv)
    assert np.array_equal(nu.download().view(U32), bits(wu)) and np.array_equal(ns.download().view(U32), bits(ws))
    assert np.array_equal(ou.download().view(U32), bits(vu)) and np.array_equal(of.download().view(U32), bits(vf))
    assert records[0].download(16, 1).tobytes() == wrec.tobytes() and records[1].download(16, 1).tobytes() == vrec.tobytes()
    # the convenience forms: arrays and the records read back; no record, no score, no flag
    gu, gv, gs, grec = ctx.correlate_offset(p0, p1, w, h, 0.0, 1.0, r, d, s, predictor=(pu, pv))
    assert np.array_equal(bits(gu), bits(wu)) and np.array_equal(bits(gv), bits(wv)) and bytes(grec) == wrec.tobytes()
    hu, hv, hf, hrec = ctx.validate_nodes(nu, nv, nw, nh)
    assert np.array_equal(bits(hu), bits(vu)) and np.array_equal(bits(hf), bits(vf)) and bytes(hrec) == vrec.tobytes()
    assert call(record=None, ns=None) == 0 and validate(record=None, flag=None) == 0
    ctx.synchronize()


# ---- the host layer ---------------------------------------------------------------------------------------------------------------
CHAIN = ((15, 8, 16), (7, 3, 8), (4, 2, 4))


def noisy_speckle(w=96, h=80, seed=1, sigma=25.0):
    sc = scenes_module().make_speckle_scene("large_translation", w, h, seed=seed)
    rng = np.random.default_rng(7)
    frame_0 = (sc.frame_0 * F32(3) - F32(100) + rng.normal(0, sigma, (h, w))).astype(F32)
    frame_1 = (sc.frame_1 * F32(3) - F32(100) + rng.normal(0, sigma, (h, w))).astype(F32)
    return sc, frame_0, frame_1


def report_bytes(reports):
    return [(q.nw, q.nh, bytes(q.correlation), bytes(q.validation)) for q in reports]


def reference_bytes(reports):
    return [(nw, nh, rec.tobytes(), val.tobytes()) for nw, nh, rec, val in reports]


@pytest.mark.parametrize("replace,validate_last", [(True, True), (False, True), (True, False)])
def test_chain_equals_its_parts(flow2d, ctx, replace, validate_last):
    """OpticalFlow.correlate_multipass_device on a noisy speckle pair is the entries called by hand in the order of the header,
    byte for byte, and the restatement's chain; the host-image form returns the same field."""
    sc, frame_0, frame_1 = noisy_speckle()
    h, w = frame_0.shape
    lo, scale = frame_range(frame_0, frame_1)
    assert lo != 0 and scale != 1
    cut = 0.1
    f0, f1 = ctx.plane(w, h, frame_0), ctx.plane(w, h, frame_1)
    new = lambda: ctx.plane(w, h).fill_bytes(0x7F)  # noqa: E731
    wu, wv, ws, wreports, (eu, ev) = multipass_reference(frame_0, frame_1, lo, scale, CHAIN, cut, replace=replace, validate_last=validate_last)
    nw, nh = grid(w, h, CHAIN[-1][0], CHAIN[-1][2])
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        nu, nv, ns, fu, fv = (new() for _ in range(5))
        reports = flow.correlate_multipass_device(f0.ptr, f1.ptr, lo, scale, CHAIN, cut, replace=replace, validate_last=validate_last,
                                                  dev_nodes=(nu.ptr, nv.ptr), dev_score=ns.ptr, dev_flow=(fu.ptr, fv.ptr))
        # by hand
        raw, val, pred = [new(), new()], [new(), new()], None
        hs, du, dv = new(), new(), new()
        records = [ctx.pass_records().fill_bytes(0x7F) for _ in range(2)]
        by_hand = []
        for k, (r, d, s) in enumerate(CHAIN):
            last = k == len(CHAIN) - 1
            gw, gh = grid(w, h, r, s)
            ctx.correlate_offset(f0, f1, w, h, lo, scale, r, d, s, cut, pred, raw[0], raw[1], hs if last else None, records[0])
            entry = [gw, gh, records[0].download(16, 1).tobytes(), bytes(64)]
            final = raw
            if not last or validate_last:
                ctx.validate_nodes(raw[0], raw[1], gw, gh, 2.0, 0.1, 3, flow2d.VALIDATE_REPLACE if (not last or replace) else flow2d.VALIDATE_FLAG,
                                   val[0], val[1], None, records[1])
                entry[3] = records[1].download(16, 1).tobytes()
                final = val
            ctx.expand_nodes(final[0], final[1], gw, gh, r, s, du, dv, w, h)
            pred = (du, dv)
            by_hand.append(tuple(entry))
        ctx.synchronize()
        for a, b in ((nu, final[0]), (nv, final[1]), (ns, hs), (fu, du), (fv, dv)):
            assert a.download(nw, nh).tobytes() == b.download(nw, nh).tobytes()
        assert fu.download().tobytes() == du.download().tobytes() and fv.download().tobytes() == dv.download().tobytes()
        assert (nu.download().view(U32)[nh:] == POISON).all() and (nu.download().view(U32)[:, nw:] == POISON).all()
        assert report_bytes(reports) == by_hand
        # the restatement
        assert np.array_equal(nu.download(nw, nh).view(U32), bits(wu)) and np.array_equal(nv.download(nw, nh).view(U32), bits(wv))
        assert np.array_equal(ns.download(nw, nh).view(U32), bits(ws))
        assert np.array_equal(fu.download().view(U32), bits(eu)) and np.array_equal(fv.download().view(U32), bits(ev))
        assert report_bytes(reports) == reference_bytes(wreports)
        print("chain:", json.dumps([q.summary() for q in reports]))
        assert reports[1].correlation.unpredicted == 0 and reports[0].validation.nodes == reports[0].nw * reports[0].nh
        if not validate_last:
            assert bytes(reports[-1].validation) == bytes(64)
        # without the caller's node planes: the object's own, the same dense field
        gu, gv = new(), new()
        again = flow.correlate_multipass_device(f0.ptr, f1.ptr, lo, scale, CHAIN, cut, replace=replace, validate_last=validate_last,
                                                dev_flow=(gu.ptr, gv.ptr))
        assert gu.download().tobytes() == fu.download().tobytes() and gv.download().tobytes() == fv.download().tobytes()
        assert report_bytes(again) == report_bytes(reports)
        # an initial predictor: the ground truth as a dense flow, one fine pass around it
        pu, pv = ctx.plane(w, h, sc.gt_u), ctx.plane(w, h, sc.gt_v)
        one = flow.correlate_multipass_device(f0.ptr, f1.ptr, lo, scale, CHAIN[-1:], cut, replace=replace, validate_last=validate_last,
                                              dev_predictor=(pu.ptr, pv.ptr), dev_nodes=(nu.ptr, nv.ptr))
        xu, xv, _, xreports, _ = multipass_reference(frame_0, frame_1, lo, scale, CHAIN[-1:], cut, replace=replace, validate_last=validate_last,
                                                     predictor=(sc.gt_u, sc.gt_v))
        assert np.array_equal(nu.download(nw, nh).view(U32), bits(xu)) and report_bytes(one) == reference_bytes(xreports)
        assert np.nanmedian(np.abs(xu)) > CHAIN[-1][1] + 2  # (the motion is beyond the fine pass's own range)
        # the host-image form
        if replace and validate_last:
            pu_, pv_, ps_, preports, (plo, pscale), (qu, qv) = flow.correlate_multipass(frame_0, frame_1, CHAIN, cut, flow=True)
            assert (F32(plo), F32(pscale)) == (lo, scale)
            assert np.array_equal(bits(pu_), bits(wu)) and np.array_equal(bits(pv_), bits(wv)) and np.array_equal(bits(ps_), bits(ws))
            assert np.array_equal(bits(qu), bits(eu)) and np.array_equal(bits(qv), bits(ev)) and report_bytes(preports) == report_bytes(reports)
            for bad in (dict(passes=[]), dict(passes=[(7, 8, 8)] * 7), dict(passes=[(16, 8, 8)]), dict(passes=[(7, 8, 8)], threshold=0.0),
                        dict(passes=[(7, 8, 8)], min_neighbours=9), dict(passes=[(7, 8, 8)], min_score=float("nan"))):
                with pytest.raises(flow2d.Flow2DError):
                    flow.correlate_multipass(frame_0, frame_1, **dict(dict(passes=CHAIN), **bad))
            with pytest.raises(flow2d.Flow2DError):  # a node plane that is a frame
                flow.correlate_multipass_device(f0.ptr, f1.ptr, lo, scale, CHAIN, dev_nodes=(f0.ptr, nv.ptr))
    finally:
        flow.close()


def test_cli_correlation_passes(flow2d, ctx, tmp_path):
    """--correlation-passes on a 96 x 80 speckle pair writes the files of --correlation from the last pass of
    OpticalFlow.correlate_multipass and prints one CorrelationPasses line; --initial-flow is the first pass's predictor;
    --validate-flag-only leaves the last pass's outliers NaN; a bad value or combination is a usage error."""
    w, h = 96, 80
    sc, frame_0, frame_1 = noisy_speckle()
    names = [str(tmp_path / "f0.raw"), str(tmp_path / "f1.raw")]
    frame_0.tofile(names[0])
    frame_1.tofile(names[1])
    truth = str(tmp_path / "truth.flo")
    flow2d.write_flo(truth, sc.gt_u, sc.gt_v)
    spec = ",".join("%d:%d:%d" % p for p in CHAIN)

    def run(options, out):
        out.mkdir()
        q = subprocess.run([flow2d.CLI_PATH] + options + names + [str(w), str(h), "t_", str(out) + "/"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=300)
        return q, {f.name: f.read_bytes() for f in out.iterdir()}

    def printed(q):
        line = [x for x in q.stdout.splitlines() if x.startswith("CorrelationPasses: ")]
        assert len(line) == 1, q.stdout[-2000:]
        return json.loads(line[0][len("CorrelationPasses: "):])

    nw, nh = grid(w, h, CHAIN[-1][0], CHAIN[-1][2])
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        q, files = run(["--flo", "--correlation-passes", spec, "--correlation-min-score", "0.125"], tmp_path / "passes")
        assert q.returncode == 0, q.stdout[-2000:]
        nu, nv, ns, reports, (lo, scale), (fu, fv) = flow.correlate_multipass(frame_0, frame_1, CHAIN, 0.125, flow=True)
        assert files["t_flow-u-96-80.raw"] == fu.tobytes() and files["t_flow-v-96-80.raw"] == fv.tobytes()
        assert files["t_node-u-%d-%d.raw" % (nw, nh)] == nu.tobytes() and files["t_node-v-%d-%d.raw" % (nw, nh)] == nv.tobytes()
        assert files["t_node-score-%d-%d.raw" % (nw, nh)] == ns.tobytes()
        gu, gv = flow2d.read_flo(str(tmp_path / "passes" / "t_flow.flo"))
        assert gu.tobytes() == fu.tobytes() and gv.tobytes() == fv.tobytes()
        line = printed(q)
        assert line["passes"] == [dict(q_.summary(), radius=p[0], range=p[1], spacing=p[2]) for q_, p in zip(reports, CHAIN)]
        assert (line["min_score"], F32(line["lo"]), F32(line["scale"]), line["replace"], line["predictor"]) == (0.125, F32(lo), F32(scale), True, False)
        assert "Correlation: " not in q.stdout
        # the options of the validation, and a predictor
        q, files = run(["--correlation-passes", "4:2:4", "--initial-flow", truth, "--validate-flag-only", "--validate-threshold", "1.5",
                        "--validate-epsilon", "0.05", "--validate-min-neighbours", "4"], tmp_path / "predicted")
        assert q.returncode == 0, q.stdout[-2000:]
        nu, nv, ns, reports, _ = flow.correlate_multipass(frame_0, frame_1, [(4, 2, 4)], threshold=1.5, epsilon=0.05, min_neighbours=4,
                                                          replace=False, predictor=(sc.gt_u, sc.gt_v))
        assert files["t_node-u-%d-%d.raw" % (nw, nh)] == nu.tobytes() and files["t_node-v-%d-%d.raw" % (nw, nh)] == nv.tobytes()
        line = printed(q)
        assert line["predictor"] is True and line["replace"] is False and line["min_neighbours"] == 4
        assert line["passes"][0]["validation"] == reports[0].validation.summary() and reports[0].validation.outliers > 0
        assert np.isnan(nu).sum() >= reports[0].validation.outliers
    finally:
        flow.close()
    plain, plain_files = run(["--flo"], tmp_path / "plain")
    assert plain.returncode == 0 and "CorrelationPasses: " not in plain.stdout and not [f for f in plain_files if "node" in f]
    for bad in (["--correlation-passes"], ["--correlation-passes", "7:8"], ["--correlation-passes", "7:8:8,"], ["--correlation-passes", "0:8:8"],
                ["--correlation-passes", "7:8:x"], ["--correlation-passes", ",".join(["7:8:8"] * 7)],
                ["--correlation-passes", "7:8:8", "--correlation", "7"], ["--correlation-passes", "7:8:8", "--backward"],
                ["--correlation-passes", "7:8:8", "--refine", "3"], ["--correlation-passes", "7:8:8", "--correlation-prior", "7"],
                ["--correlation-passes", "7:8:8", "--validate-threshold", "0"], ["--correlation-passes", "7:8:8", "--validate-min-neighbours", "9"],
                ["--validate-flag-only"], ["--validate-epsilon", "0.1"]):
        q = subprocess.run([flow2d.CLI_PATH] + bad + names + [str(w), str(h), "t_"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert q.returncode == 5, (bad, q.stdout[-500:])
    # a pass the frame cannot hold is refused by the host layer, not by the parser
    q = subprocess.run([flow2d.CLI_PATH, "--correlation-passes", "33:8:8"] + names + [str(w), str(h), "t_", str(tmp_path) + "/"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert q.returncode == 4, q.stdout[-500:]
