"""flow2d_correlate_masked_2d and flow2d_validate_nodes_masked_2d on the device against their numpy restatement
(tests/test_correlate_masked_cpu.py), bit for bit: a one-window frame under the three masks that decide its state, random masks on
windows of 7 and 9 pixels a side (both row-tail lengths) with a node count that is no multiple of the waves, the specimen scene
with a predictor that has a step inside a workgroup's nodes and search areas partly outside frame 1, the limits of radius and
range (the largest LDS slice), the equivalences with Context.correlate_offset and Context.validate_nodes, validation grids of one
node, one row, one column, 2 x 2 and several workgroups under random node masks in both modes; containers larger than the data
with poisoned outputs; the same bytes from a replayed graph, from an instance alone or in a lock-step batch, and on planes of
4 GiB; the refusals on a real context."""
import ctypes

import numpy as np
import pytest

from test_correlate_cpu import F32, NAN_BITS, U32, bits, grid, random_frames, scenes_module
from test_correlate_masked_cpu import (FLAG_MASKED, correlate_masked_reference, counts, default_min_pixels, extremes, included,
                                       off_specimen, validate_masked_reference)
from test_gpu_batch_kernels import Tall, pitch_of, stride_of
from test_gpu_multipass import POISON, WAVES, constant, node_field, padded, release, run_offset, run_validate
from test_gpu_wide_planes import H as TALL_H, HIGH_LINE, LINE, W as TALL_W, node_bits, node_poison, on_both, record_bytes, wrapped_rows_differ
from test_multipass_cpu import FLAG, PASS_DTYPE, REPLACE, VALIDATION_DTYPE
from test_subset_masked_cpu import random_mask

pytestmark = pytest.mark.gpu


def run_masked(ctx, f0, f1, mask, min_pixels, pred, r, d, s, lo=0.0, scale=1.0, cut=-1.0, score=True):
    """(u bits, v bits, score bits, record bytes) of one call into poisoned outputs, which must stay poisoned beyond the grid."""
    h, w = f0.shape
    nw, nh = grid(w, h, r, s)
    frames = [padded(ctx, f0), padded(ctx, f1)] + ([padded(ctx, mask)] if mask is not None else [])
    predictor = [padded(ctx, p) for p in pred] if pred is not None else None
    nodes = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(3)]
    record = ctx.pass_records().fill_bytes(0x7F)
    ctx.correlate_masked(frames[0], frames[1], w, h, lo, scale, r, d, s, frames[2] if mask is not None else None, min_pixels, cut, predictor,
                         nodes[0], nodes[1], nodes[2] if score else None, record)
    got = [q.download().view(U32) for q in nodes]
    for g in got[:3 if score else 2]:
        assert (g[nh:] == POISON).all() and (g[:, nw:] == POISON).all(), "written beyond the grid"
    if not score:
        assert (got[2] == POISON).all()
    result = [g[:nh, :nw] for g in got] + [record.download(16, 1).tobytes()]
    release(ctx, frames + (predictor or []) + nodes + [record])
    return result


def check_masked(ctx, f0, f1, mask, min_pixels, pred, r, d, s, what, lo=0.0, scale=1.0, cut=-1.0):
    """One case against the restatement; returns the restatement's (u, v, score, the record's eight words)."""
    wu, wv, ws, record = correlate_masked_reference(f0, f1, lo, scale, r, d, s, mask, min_pixels, cut, *(pred if pred is not None else (None, None)))
    gu, gv, gs, grec = run_masked(ctx, f0, f1, mask, min_pixels, pred, r, d, s, lo, scale, cut)
    for got, want, name in ((gu, wu, "u"), (gv, wv, "v"), (gs, ws, "score")):
        same = got == bits(want)
        assert same.all(), "%s: %s differs at %d places, first (y, x) = %s: %s, want %s" % (
            what, name, (~same).sum(), np.argwhere(~same)[0], got[~same][0].view(F32), bits(want)[~same][0].view(F32))
    assert grec == record.tobytes(), "%s: record %s, want %s" % (what, np.frombuffer(grec, PASS_DTYPE), record)
    return wu, wv, ws, counts(record)


# ---- flow2d_correlate_masked_2d ---------------------------------------------------------------------------------------------------
def test_one_window_frame_under_the_masks_that_decide_its_state(flow2d, ctx):
    f0, f1 = random_frames(7, 7, seed=2, shift=(0, 0))
    min_pixels = 20
    centre = np.zeros((7, 7), F32)
    centre[3, 3] = 1
    few = np.zeros((7, 7), F32)
    few.flat[:30] = 1  # Nv = 19, the centre (flat index 24) given back below
    few[3, 3] = 0
    few[6, 6] = 1
    assert included(few).sum() == min_pixels - 1
    exact = few.copy()
    exact[6, 6] = 0
    pred = constant((7, 7), np.nan, 0.0)
    for mask, what in ((centre, "centre excluded"), (few, "Nv = min_pixels - 1")):
        wu, _, ws, rec = check_masked(ctx, f0, f1, mask, min_pixels, pred, 3, 2, 3, "7x7, " + what)
        assert rec == [1, 0, 0, 0, 0, 0, 1, 0] and bits(wu)[0, 0] == NAN_BITS and ws[0, 0] == 0  # (not unpredicted: no predictor is read)
    wu, _, _, rec = check_masked(ctx, f0, f1, exact, min_pixels, pred, 3, 2, 3, "7x7, Nv = min_pixels")
    assert rec[:5] == [1, 0, 0, 1, 1] and rec[6] == 0 and np.isfinite(wu[0, 0])
    _, _, _, rec = check_masked(ctx, f0, f1, np.zeros((7, 7), F32), 49, None, 3, 2, 3, "7x7, all zero")
    assert rec == [1, 0, 0, 1, 0, 1, 0, 0]
    nan = np.zeros((7, 7), F32)
    nan[0, 0] = np.nan
    _, _, _, rec = check_masked(ctx, f0, f1, nan, 49, None, 3, 2, 3, "7x7, one NaN, min_pixels 49")
    assert rec == [1, 0, 0, 0, 0, 0, 1, 0]


@pytest.mark.parametrize("w,h,r,d,s,min_pixels", [(40, 33, 3, 4, 5, 30), (37, 29, 4, 3, 3, 50)])
def test_random_masks(flow2d, ctx, w, h, r, d, s, min_pixels):
    """Windows of 7 and 9 pixels a side: the row's tail quad holds 3 and 1 pixels, with masked bytes among them."""
    f0, f1 = random_frames(w, h, seed=w, shift=(2, -1))
    f0[5:17, 4:18] = 77.0  # flat where the mask leaves it: invalid nodes
    mask = random_mask((h, w), seed=w)
    mask[5:17, 4:18] = 0
    mask[20:, 24:] = 1  # a block: centres excluded, and windows below min_pixels beside it
    mask[1, 2] = np.nan
    nw, nh = grid(w, h, r, s)
    assert (nw * nh) % WAVES != 0 and (2 * r + 1) % 4 in (1, 3)
    _, _, _, rec = check_masked(ctx, f0, f1, mask, min_pixels, None, r, d, s, "%dx%d random mask" % (w, h))
    assert rec[0] == nw * nh and 0 < rec[6] < nw * nh and rec[1] > 0
    rng = np.random.default_rng(3)
    pred = (rng.uniform(-4, 4, (h, w)).astype(F32), rng.uniform(-4, 4, (h, w)).astype(F32))
    pred[0][rng.random((h, w)) < 0.1] = np.nan
    _, _, ws, rec = check_masked(ctx, f0, f1, mask, min_pixels, pred, r, d, s, "%dx%d random mask and predictor" % (w, h))
    assert 0 < rec[4] < nw * nh - rec[6]
    cut = float(np.median(ws[ws != 0]))
    check_masked(ctx, f0, f1, mask, 1, pred, r, d, s, "%dx%d min_pixels 1, a minimum score, a scale" % (w, h), lo=-3.7, scale=0.913, cut=cut)
    a, b = run_masked(ctx, f0, f1, mask, min_pixels, pred, r, d, s), run_masked(ctx, f0, f1, mask, min_pixels, pred, r, d, s, score=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3]


def test_specimen_with_a_step_predictor(flow2d, ctx):
    """The plate with a hole moved by (6.4, -3.3) in front of a textured background, grid (7, 8, 8): eleven nodes a row, so a
    workgroup's four nodes straddle the predictor's steps; near each border the predictor points out of frame 1."""
    sc, mask = scenes_module().make_speckle_specimen("stretch", 96, 80, seed=0, translation=(6.4, -3.3), background_gain=1.0,
                                                     background_offset=0.0)
    w, h, r, d, s = 96, 80, 7, 8, 8
    lo, scale = extremes(sc.frame_0, sc.frame_1)
    pu, pv = np.full((h, w), 6.0, F32), np.full((h, w), -3.0, F32)
    pu[:, 44:] = 7.4  # a step between node columns 4 and 5
    pu[:, :16], pu[:, 80:], pv[:12, :], pv[68:, :] = -13.0, 14.5, -12.0, 11.0
    nw, nh = grid(w, h, r, s)
    assert nw == 11 and nw % WAVES != 0
    wu, wv, _, rec = check_masked(ctx, sc.frame_0, sc.frame_1, mask, default_min_pixels(r), (pu, pv), r, d, s, "specimen", lo, scale)
    assert rec[0] == 99 and rec[6] > 20 and rec[4] == 0 and rec[5] > 0
    on = ~off_specimen(mask, nw, nh, r, s)
    assert np.isfinite(wu[on]).sum() > 30


def test_limits_of_radius_and_range(flow2d, ctx):
    """r 15, d 32 on the smallest frame with a 2 x 2 grid at s = 16: the largest slice, 976 + 976 + 9040 bytes a wave."""
    w, h, r, d, s = 47, 47, 15, 32, 16
    f0, f1 = random_frames(w, h, seed=23, shift=(4, 3))
    assert grid(w, h, r, s) == (2, 2)
    mask = random_mask((h, w), seed=8)
    mask[15, 15] = mask[15, 31] = mask[31, 15] = 0
    mask[31, 31] = 1  # one of the four is off the specimen
    pu, pv = np.zeros((h, w), F32), np.zeros((h, w), F32)
    pu[:, 20:], pv[20:, :] = 9.0, -7.0
    _, _, _, rec = check_masked(ctx, f0, f1, mask, default_min_pixels(r), (pu, pv), r, d, s, "r 15, d 32")
    assert rec[0] == 4 and rec[6] == 1 and rec[1] == 0 and rec[5] > 300


@pytest.mark.parametrize("w,h,r,d,s", [(130, 37, 5, 4, 6), (65, 17, 2, 3, 1)])
def test_no_mask_and_a_mask_that_excludes_nothing_give_the_unmasked_bytes(flow2d, ctx, w, h, r, d, s):
    f0, f1 = random_frames(w, h, seed=31, shift=(-1, 2))
    f0[6:24, 30:60] = 50.0
    y, x = np.mgrid[0:h, 0:w]
    pred = ((2.5 * np.sin(x / 7.0)).astype(F32), (2.5 * np.cos(y / 4.0)).astype(F32))
    pred[0][5:9, 40:60] = np.nan
    for p in (None, pred):
        want = run_offset(ctx, f0, f1, p, r, d, s, cut=0.3)
        assert np.frombuffer(want[3], PASS_DTYPE)["invalid"][0] > 0
        for mask, min_pixels in ((None, -7), (np.zeros((h, w), F32), (2 * r + 1) ** 2), (np.full((h, w), 0.25, F32), 1)):
            got = run_masked(ctx, f0, f1, mask, min_pixels, p, r, d, s, cut=0.3)
            assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3]


# ---- flow2d_validate_nodes_masked_2d ------------------------------------------------------------------------------------------------
def run_validate_masked(ctx, nu, nv, mask, r, s, mode, threshold=2.0, epsilon=0.1, k=3, flag=True):
    nh, nw = nu.shape
    h, w = mask.shape
    ins = [padded(ctx, nu), padded(ctx, nv), padded(ctx, mask)]
    outs = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(3)]
    record = ctx.pass_records().fill_bytes(0x7F)
    ctx.validate_nodes_masked(ins[0], ins[1], nw, nh, ins[2], w, h, r, s, threshold, epsilon, k, mode, outs[0], outs[1], outs[2] if flag else None,
                              record)
    got = [q.download().view(U32) for q in outs]
    for g in got[:3 if flag else 2]:
        assert (g[nh:] == POISON).all() and (g[:, nw:] == POISON).all(), "written beyond the grid"
    if not flag:
        assert (got[2] == POISON).all()
    result = [g[:nh, :nw] for g in got] + [record.download(16, 1).tobytes()]
    release(ctx, ins + outs + [record])
    return result


def check_validate_masked(ctx, nu, nv, mask, r, s, mode, what, **kw):
    wu, wv, wf, record = validate_masked_reference(nu, nv, mask, r, s, kw.get("threshold", 2.0), kw.get("epsilon", 0.1), kw.get("k", 3), mode)
    gu, gv, gf, grec = run_validate_masked(ctx, nu, nv, mask, r, s, mode, **kw)
    for got, want, name in ((gu, wu, "u"), (gv, wv, "v"), (gf, wf, "flag"))[:3 if kw.get("flag", True) else 2]:
        same = got == bits(want)
        assert same.all(), "%s: %s differs at %d places, first (y, x) = %s" % (what, name, (~same).sum(), np.argwhere(~same)[0])
    assert grec == record.tobytes(), "%s: record %s, want %s" % (what, np.frombuffer(grec, VALIDATION_DTYPE), record)
    return wu, wv, wf, counts(record)


def centre_mask(nw, nh, r, s, seed, fraction=0.3):
    """A pixel mask of the smallest frame with an nw x nh grid: random beside the centres, and at the centres a random node mask."""
    w, h = 2 * r + 1 + (nw - 1) * s, 2 * r + 1 + (nh - 1) * s
    assert grid(w, h, r, s) == (nw, nh)
    rng = np.random.default_rng(seed)
    mask = (rng.random((h, w)) < 0.5).astype(F32)
    mask[r::s, r::s] = (rng.random((nh, nw)) < fraction).astype(F32)
    return mask


@pytest.mark.parametrize("nw,nh", [(1, 1), (9, 1), (1, 9), (2, 2), (70, 5), (13, 21)])
@pytest.mark.parametrize("mode", [FLAG, REPLACE])
def test_validation_grids(flow2d, ctx, nw, nh, mode):
    r, s = 2, 3
    u, v = node_field(nw, nh, seed=nw + 3 * nh)
    mask = centre_mask(nw, nh, r, s, seed=nw * 7 + nh)
    if nw * nh == 1:
        mask[r, r] = 1
    if (nw, nh) == (2, 2):
        u[:, :], v[:, :] = 1.0, 2.0
        u[1, 1] = 60.0
        mask[r::s, r::s] = [[0, 1], [0, 0]]  # k = 2 < 3: the spike stays, unjudged -- the unmasked test replaces it
    _, _, wf, rec = check_validate_masked(ctx, u, v, mask, r, s, mode, "%dx%d mode %d" % (nw, nh, mode))
    off = off_specimen(mask, nw, nh, r, s)
    assert rec[0] == nw * nh and rec[6] == off.sum() and (wf[off] == FLAG_MASKED).all() and rec[7] == 0
    if (nw, nh) == (2, 2):
        assert rec[:7] == [4, 0, 0, 0, 3, 0, 1] and wf[1, 1] == 0
    if nw * nh > 256:
        assert rec[2] > 0 and (rec[3] > 0) == (mode == REPLACE) and rec[4] > 0 and 0 < rec[6] < nw * nh
    check_validate_masked(ctx, u, v, mask, r, s, mode, "%dx%d k 1" % (nw, nh), k=1, threshold=1.25, epsilon=0.03)
    check_validate_masked(ctx, u, v, mask, r, s, mode, "%dx%d k 8" % (nw, nh), k=8, flag=False)
    # a mask that excludes no centre, and none: the unmasked entry's bytes
    want = run_validate(ctx, u, v, mode)
    beside = np.ones_like(mask)
    beside[r::s, r::s] = 0
    got = run_validate_masked(ctx, u, v, beside, r, s, mode)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3]
    ins = [padded(ctx, u), padded(ctx, v)]
    gu, gv, gf, grec = ctx.validate_nodes_masked(ins[0], ins[1], nw, nh, None, 0, 0, 99, 0, mode=mode)
    assert np.array_equal(bits(gu), want[0]) and np.array_equal(bits(gv), want[1]) and np.array_equal(bits(gf), want[2]) and bytes(grec) == want[3]
    release(ctx, ins)


# ---- graph and batch ----------------------------------------------------------------------------------------------------------------
def masked_case(w, h, seed, shift=(1, -1)):
    f0, f1 = random_frames(w, h, seed=seed, shift=shift)
    mask = random_mask((h, w), 0.25, seed=seed + 1)
    mask[h // 2:, : w // 3] = 1
    y, x = np.mgrid[0:h, 0:w]
    pred = ((shift[0] + 1.4 * np.sin(x / (5.0 + seed % 3))).astype(F32), (shift[1] + 1.3 * np.cos(y / 6.0)).astype(F32))
    pred[1][10:14, 70:90] = np.inf
    return f0, f1, mask, pred


def test_a_replayed_graph_gives_the_eager_bytes(flow2d, ctx):
    w, h, r, d, s = 130, 37, 4, 5, 3
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    f0, f1, mask, pred = masked_case(w, h, 21)
    nw, nh = grid(w, h, r, s)
    wu, wv, ws, wrec = correlate_masked_reference(f0, f1, 0.0, 1.0, r, d, s, mask, 40, 0.2, *pred)
    vu, vv, vf, vrec = validate_masked_reference(wu, wv, mask, r, s, 2.0, 0.1, 3, REPLACE)
    assert counts(wrec)[6] > 0 and counts(vrec)[6] > 0
    frames, predictor = [padded(ctx, f0), padded(ctx, f1), padded(ctx, mask)], [padded(ctx, p) for p in pred]
    nodes = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(6)]
    records = [ctx.pass_records().fill_bytes(0x7F) for _ in range(2)]

    def both():
        ctx.correlate_masked(frames[0], frames[1], w, h, 0.0, 1.0, r, d, s, frames[2], 40, 0.2, predictor, nodes[0], nodes[1], nodes[2], records[0])
        ctx.validate_nodes_masked(nodes[0], nodes[1], nw, nh, frames[2], w, h, r, s, 2.0, 0.1, 3, REPLACE, nodes[3], nodes[4], nodes[5], records[1])

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


@pytest.mark.parametrize("kind", ["rows"])
def test_lock_step_batch(flow2d, ctx, kind):
    """Three instances a padded stride apart with different frames, masks and predictors: node planes, validated planes and
    records of instance b are the restatement's for that instance alone, and every other word of the allocations is what it was."""
    w, h, cw, ch, count, r, d, s = 130, 37, 140, 40, 3, 5, 4, 6
    stride = stride_of(kind, pitch_of(cw), ch)
    cases = [masked_case(w, h, 30 + b, shift=(b - 1, 1)) for b in range(count)]
    cases[1][0][6:24, 30:60] = 50.0
    cases[1][2][6:24, 30:60] = 0  # invalid nodes in one instance only
    nw, nh = grid(w, h, r, s)
    new = lambda: Tall(ctx, cw, ch, count, stride)  # noqa: E731
    t0, t1, tm = new().fill([c[0] for c in cases]), new().fill([c[1] for c in cases]), new().fill([c[2] for c in cases])
    tu, tv = new().fill([c[3][0] for c in cases]), new().fill([c[3][1] for c in cases])
    nu, nv, ns, ou, ov, of = (new() for _ in range(6))
    records = [ctx.pass_records(count).fill_bytes(0x7F) for _ in range(2)]
    with ctx.set_batch(count, stride):
        ctx.correlate_masked(t0, t1, w, h, 0.0, 1.0, r, d, s, tm, 60, 0.3, (tu, tv), nu, nv, ns, records[0], instances=count)
        ctx.validate_nodes_masked(nu, nv, nw, nh, tm, w, h, r, s, 2.0, 0.1, 3, REPLACE, ou, ov, of, records[1], instances=count)
    ctx.synchronize()
    refs = [correlate_masked_reference(c[0], c[1], 0.0, 1.0, r, d, s, c[2], 60, 0.3, *c[3]) for c in cases]
    vals = [validate_masked_reference(ref[0], ref[1], c[2], r, s, 2.0, 0.1, 3, REPLACE) for ref, c in zip(refs, cases)]
    for tall, k, name in ((nu, 0, "node u"), (nv, 1, "node v"), (ns, 2, "node score")):
        tall.check([ref[k] for ref in refs], "%s (%s)" % (name, kind))
    for tall, k, name in ((ou, 0, "validated u"), (ov, 1, "validated v"), (of, 2, "flag")):
        tall.check([val[k] for val in vals], "%s (%s)" % (name, kind))
    for tall in (t0, t1, tm, tu, tv):
        tall.check(None, "inputs")
    got = [q.download(16 * count, 1).tobytes() for q in records]
    assert counts(refs[1][3])[1] > 0 and len({counts(ref[3])[6] for ref in refs}) > 1 and all(counts(ref[3])[6] > 0 for ref in refs)
    for b in range(count):
        assert got[0][64 * b:64 * b + 64] == refs[b][3].tobytes(), "pass record of instance %d" % b
        assert got[1][64 * b:64 * b + 64] == vals[b][3].tobytes(), "validation record of instance %d" % b
        alone = run_masked(ctx, cases[b][0], cases[b][1], cases[b][2], 60, cases[b][3], r, d, s, cut=0.3)
        assert np.array_equal(alone[0], bits(refs[b][0])) and np.array_equal(alone[2], bits(refs[b][2])) and alone[3] == got[0][64 * b:64 * b + 64]
        lone = run_validate_masked(ctx, refs[b][0], refs[b][1], cases[b][2], r, s, REPLACE)
        assert np.array_equal(lone[0], bits(vals[b][0])) and np.array_equal(lone[2], bits(vals[b][2])) and lone[3] == got[1][64 * b:64 * b + 64]
    # a written range must not meet a later instance of the mask
    lib = flow2d.hip_lib()
    with ctx.set_batch(count, stride):
        assert lib.flow2d_correlate_masked_2d(ctx.handle, t0.ptr, t1.ptr, tu.ptr, tv.ptr, w, h, t0.pitch, 0.0, 1.0, r, d, s, -1.0, tm.ptr, 60,
                                              tm.ptr + 2 * stride, nv.ptr, ns.ptr, nu.pitch, records[0].ptr) == 1
        assert lib.flow2d_validate_nodes_masked_2d(ctx.handle, nu.ptr, nv.ptr, nw, nh, nu.pitch, 2.0, 0.1, 3, REPLACE, tm.ptr, w, h, tm.pitch, r, s,
                                                   ou.ptr, tm.ptr + stride, None, records[1].ptr) == 1
    ctx.synchronize()
    nu.check([ref[0] for ref in refs], "node u after the refusals")


# ---- planes of 4 GiB ----------------------------------------------------------------------------------------------------------------
def test_planes_of_4_gib(flow2d, ctx):
    """correlate_masked_kernel<size_t> and the masked validation's 64-bit mask addressing: the 100 x 4200 frame of
    tests/test_gpu_wide_planes.py in planes with a pitch of 1 MiB (only the frame's columns are touched), grid (10, s 64), range 3:
    node row 63 (rows 4032 .. 4052) is sent 50 rows down, across row 4096; row 64 (rows 4096 .. 4116) six rows up, across it; row 65
    lies beyond.  The same bytes as on planes with a pitch of 512 bytes, and the restatement's.  And the same bytes from
    correlate_masked_kernel<unsigned> on planes just below 4 GiB, where row 2101 is the first whose byte offset has bit 31 set: node
    row 32 (rows 2048 .. 2068) is sent 50 rows down, across it; row 33 (rows 2112 .. 2132) twenty rows up; row 34 lies beyond."""
    r, d, s = 10, 3, 64
    f0, f1 = random_frames(TALL_W, TALL_H, seed=52, shift=(2, -1))
    lo, scale = 0.0, 1.0
    nw, nh = grid(TALL_W, TALL_H, r, s)
    cy = r + np.arange(nh) * s
    rng = np.random.default_rng(53)
    pu, pv = (rng.uniform(-3, 3, (TALL_H, TALL_W)).astype(F32) for _ in range(2))
    pv[cy[63] - 2:cy[63] + 3], pv[cy[64] - 2:cy[64] + 3] = 50.0, -6.0
    pv[cy[32] - 2:cy[32] + 3], pv[cy[33] - 2:cy[33] + 3] = 50.0, -20.0
    mask = random_mask((TALL_H, TALL_W), 0.2, seed=56)
    mask[cy[:40], r] = 1          # off the specimen below the line ...
    mask[cy[65], r + s] = 1       # ... and beyond it
    mask[cy[63], :], mask[cy[64], :] = 0, 0
    mask[cy[32], :], mask[cy[33], :] = 0, 0
    min_pixels = default_min_pixels(r)
    wu, wv, ws, record = correlate_masked_reference(f0, f1, lo, scale, r, d, s, mask, min_pixels, -1.0, pu, pv)
    vu, vv, vf, vrecord = validate_masked_reference(wu, wv, mask, r, s, mode=REPLACE)
    wrapped_rows_differ(f0, f1, pu, pv, mask)
    assert cy[63] < LINE <= cy[63] + r + 50 - d and cy[64] - r - 6 - d < LINE <= cy[64] and cy[65] - r - 3 - d >= LINE
    for j in (63, 64):
        assert np.isfinite(wu[j]).all() and np.isfinite(wv[j]).all() and not np.array_equal(wv[j], wv[j - 63])
    assert cy[32] < HIGH_LINE <= cy[32] + r + 50 - d and cy[33] - r - 20 - d < HIGH_LINE <= cy[33] - r and cy[34] - r - 3 - d >= HIGH_LINE
    for j in (32, 33):
        assert np.isfinite(wu[j]).all() and np.isfinite(wv[j]).all() and not np.array_equal(wv[j], wv[j - 32])
    assert np.unique(wu[34:63][np.isfinite(wu[34:63])]).size > 1  # (nodes wholly between the two lines: column 0 is masked there)
    assert np.isfinite(wu[65, 0]) and bits(wu)[65, 1] == NAN_BITS and vf[65, 1] == FLAG_MASKED and vf[0, 0] == FLAG_MASKED
    below = correlate_masked_reference(f0[:LINE], f1[:LINE], lo, scale, r, d, s, mask[:LINE], min_pixels, -1.0, pu[:LINE], pv[:LINE])[3]
    assert below.tobytes() != record.tobytes()
    # (a mask whose rows from 4096 on were rows 0 .. again would give another field: the wrapped mask's restatement differs)
    wrapped = mask.copy()
    wrapped[LINE:] = mask[:TALL_H - LINE]
    assert not np.array_equal(bits(correlate_masked_reference(f0, f1, lo, scale, r, d, s, wrapped, min_pixels, -1.0, pu, pv)[0]), bits(wu))
    wrapped = mask.copy()
    wrapped[HIGH_LINE:] = mask[:TALL_H - HIGH_LINE]
    assert not np.array_equal(bits(correlate_masked_reference(f0, f1, lo, scale, r, d, s, wrapped, min_pixels, -1.0, pu, pv)[0]), bits(wu))

    def run(rig):
        planes = [rig.load(a) for a in (f0, f1, pu, pv, mask)]
        nodes, rec = node_poison(ctx, nw, nh, 6), [ctx.pass_records().fill_bytes(0x7F) for _ in range(2)]
        ctx.correlate_masked(planes[0], planes[1], TALL_W, TALL_H, lo, scale, r, d, s, planes[4], min_pixels, -1.0, (planes[2], planes[3]),
                             nodes[0], nodes[1], nodes[2], rec[0])
        ctx.validate_nodes_masked(nodes[0], nodes[1], nw, nh, planes[4], TALL_W, TALL_H, r, s, 2.0, 0.1, 3, REPLACE, nodes[3], nodes[4], nodes[5],
                                  rec[1])
        ctx.synchronize()
        got = dict(zip(("u", "v", "score", "validated u", "validated v", "flag"), node_bits(nodes, nw, nh)))
        got["record"], got["validation record"] = record_bytes(rec[0], 64), record_bytes(rec[1], 64)
        release(ctx, nodes + rec)
        return got

    got = on_both(ctx, 5, run)
    for name, want in (("u", wu), ("v", wv), ("score", ws), ("validated u", vu), ("validated v", vv), ("flag", vf)):
        same = got[name] == bits(want)
        assert same.all(), "%s differs at %d places, first (y, x) = %s" % (name, (~same).sum(), np.argwhere(~same)[0])
    assert got["record"] == record.tobytes(), "record %s, want %s" % (np.frombuffer(got["record"], PASS_DTYPE), record)
    assert got["validation record"] == vrecord.tobytes()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing(flow2d, ctx):
    w, h, r, d, s = 100, 40, 7, 8, 8
    lib = flow2d.hip_lib()
    f0, f1, mask, pred = masked_case(w, h, 5)
    p0, p1, pm, pu, pv = (ctx.plane(w, h, a) for a in (f0, f1, mask, pred[0], pred[1]))
    nw, nh = grid(w, h, r, s)
    nu, nv, ns, ou, ov, of = (ctx.plane(nw, nh).fill_bytes(0x7F) for _ in range(6))
    records = [ctx.pass_records().fill_bytes(0x7F) for _ in range(2)]
    span = p0.pitch * h
    nan = float("nan")
    base = dict(f0=p0.ptr, f1=p1.ptr, pu=pu.ptr, pv=pv.ptr, w=w, h=h, pitch=p0.pitch, lo=0.0, scale=1.0, r=r, d=d, s=s, cut=-1.0, mask=pm.ptr,
                minp=57, nu=nu.ptr, nv=nv.ptr, ns=ns.ptr, npitch=nu.pitch, record=records[0].ptr)

    def call(**kw):
        a = dict(base, **kw)
        return lib.flow2d_correlate_masked_2d(ctx.handle, a["f0"], a["f1"], a["pu"], a["pv"], a["w"], a["h"], a["pitch"], a["lo"], a["scale"],
                                              a["r"], a["d"], a["s"], a["cut"], a["mask"], a["minp"], a["nu"], a["nv"], a["ns"], a["npitch"],
                                              a["record"])

    bad = [dict(r=0), dict(r=16), dict(d=0), dict(d=33), dict(s=0), dict(s=65), dict(scale=0.0), dict(scale=nan), dict(lo=nan), dict(cut=nan),
           dict(f0=None), dict(f1=None), dict(nu=None), dict(nv=None), dict(w=0), dict(h=0), dict(w=14), dict(pitch=p0.pitch + 8), dict(npitch=16),
           dict(nu=p0.ptr), dict(nv=nu.ptr), dict(record=records[0].ptr + 4), dict(record=nu.ptr), dict(pu=None), dict(pu=pu.ptr + 4),
           dict(nu=pu.ptr), dict(mask=pm.ptr + 4), dict(nu=pm.ptr), dict(nv=pm.ptr + span - p0.pitch), dict(ns=pm.ptr + p0.pitch),
           dict(record=pm.ptr + 64), dict(mask=nu.ptr), dict(minp=0), dict(minp=-3), dict(minp=226), dict(r=3, minp=50)]
    for kw in bad:
        assert call(**kw) == 1, kw

    vbase = dict(nu=nu.ptr, nv=nv.ptr, nw=nw, nh=nh, npitch=nu.pitch, t=2.0, eps=0.1, k=3, mode=REPLACE, mask=pm.ptr, w=w, h=h, pitch=pm.pitch, r=r,
                 s=s, ou=ou.ptr, ov=ov.ptr, flag=of.ptr, record=records[1].ptr)

    def validate(**kw):
        a = dict(vbase, **kw)
        return lib.flow2d_validate_nodes_masked_2d(ctx.handle, a["nu"], a["nv"], a["nw"], a["nh"], a["npitch"], a["t"], a["eps"], a["k"], a["mode"],
                                                   a["mask"], a["w"], a["h"], a["pitch"], a["r"], a["s"], a["ou"], a["ov"], a["flag"], a["record"])

    for kw in [dict(nu=None), dict(ou=None), dict(nw=0), dict(npitch=16), dict(k=0), dict(k=9), dict(t=0.0), dict(eps=nan), dict(mode=2),
               dict(ou=nu.ptr), dict(ov=ou.ptr), dict(flag=ov.ptr), dict(record=records[1].ptr + 4), dict(record=ou.ptr),
               dict(mask=pm.ptr + 4), dict(w=0), dict(pitch=pm.pitch + 8), dict(r=0), dict(r=16), dict(s=0), dict(s=65), dict(w=14), dict(nw=nw - 1),
               dict(nh=nh + 1), dict(s=9), dict(r=3), dict(ou=pm.ptr), dict(flag=pm.ptr + pm.pitch), dict(record=pm.ptr + 64), dict(mask=ou.ptr)]:
        assert validate(**kw) == 1, kw
    ctx.synchronize()
    for q in (nu, nv, ns, ou, ov, of):
        assert (q.download().view(U32) == POISON).all()
    for q in records:
        assert set(q.download(16, 1).tobytes()) == {0x7F}
    # ... and the same planes are accepted
    assert call() == 0 and validate() == 0
    wu, wv, ws, wrec = correlate_masked_reference(f0, f1, 0.0, 1.0, r, d, s, mask, 57, -1.0, *pred)
    vu, vv, vf, vrec = validate_masked_reference(wu, wv, mask, r, s)
    assert np.array_equal(nu.download().view(U32), bits(wu)) and np.array_equal(ns.download().view(U32), bits(ws))
    assert np.array_equal(ou.download().view(U32), bits(vu)) and np.array_equal(of.download().view(U32), bits(vf))
    assert records[0].download(16, 1).tobytes() == wrec.tobytes() and records[1].download(16, 1).tobytes() == vrec.tobytes()
    # the convenience forms: arrays and the records read back, min_pixels by default; no record, no score, no flag
    gu, gv, gs, grec = ctx.correlate_masked(p0, p1, w, h, 0.0, 1.0, r, d, s, pm, predictor=(pu, pv))
    assert np.array_equal(bits(gu), bits(wu)) and np.array_equal(bits(gv), bits(wv)) and bytes(grec) == wrec.tobytes() and grec.masked == counts(wrec)[6]
    hu, hv, hf, hrec = ctx.validate_nodes_masked(nu, nv, nw, nh, pm, w, h, r, s)
    assert np.array_equal(bits(hu), bits(vu)) and np.array_equal(bits(hf), bits(vf)) and bytes(hrec) == vrec.tobytes() and hrec.masked == counts(vrec)[6]
    assert call(record=None, ns=None) == 0 and validate(record=None, flag=None) == 0
    ctx.synchronize()
