"""flow2d_correlate_2d and flow2d_expand_nodes_2d on the device against their numpy restatement (tests/test_correlate_cpu.py), bit
for bit: a frame of one window and one pixel past it, dense and sparse grids over more than one tile of nodes, a node count one
past the tile, ranges that reach beyond the frame, containers larger than the frame and the grid with NaN in the padding, flat,
saturated, periodic and non-finite frames, a minimum score, the record; the same bytes from a replayed graph and from an
instance alone or in a lock-step batch; the refusals on a real context; OpticalFlow.correlate_device against its parts; the
CLI."""
import ctypes
import json
import subprocess

import numpy as np
import pytest

from test_correlate_cpu import (F32, NAN_BITS, RECORD_DTYPE, U32, bits, correlate_reference, expand_reference, frame_range, grid,
                                interior_epe, random_frames, scenes_module)
from test_gpu_batch_kernels import Tall, pitch_of, stride_of

pytestmark = pytest.mark.gpu
POISON = U32(0x7F7F7F7F)
# the kernel's tile of nodes (csrc/correlate.hip, corr_tile_nodes): kCorrTileSpan / spacing held to kCorrTileMin .. kCorrTileMax
# nodes per axis, one workgroup per tile
TILE_SPAN, TILE_MIN, TILE_MAX = 32, 2, 8


def tile_nodes(spacing):
    return min(max(TILE_SPAN // spacing, TILE_MIN), TILE_MAX)


class Pair:
    """Two frames in containers 5 columns wider and 3 rows taller than the frame, the padding NaN."""

    def __init__(self, ctx, f0, f1):
        self.ctx = ctx
        self.h, self.w = f0.shape
        self.cw, self.ch = self.w + 5, self.h + 3
        self.f0, self.f1 = self.container(f0), self.container(f1)

    def container(self, a):
        full = np.full((self.ch, self.cw), np.nan, F32)
        full[:self.h, :self.w] = a
        return self.ctx.plane(self.cw, self.ch, full)

    def run(self, r, d, s, lo=0.0, scale=1.0, cut=-1.0, score=True):
        """(u bits, v bits, score bits, record bytes, expanded u bits, expanded v bits) of one call of each entry into poisoned
        outputs, which must stay poisoned beyond the grid and the frame."""
        ctx = self.ctx
        nw, nh = grid(self.w, self.h, r, s)
        nodes = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(3)]
        record = ctx.correlation_records().fill_bytes(0x7F)
        ctx.correlate(self.f0, self.f1, self.w, self.h, lo, scale, r, d, s, cut, nodes[0], nodes[1], nodes[2] if score else None, record)
        dense = [ctx.plane(self.cw, self.ch).fill_bytes(0x7F) for _ in range(2)]
        ctx.expand_nodes(nodes[0], nodes[1], nw, nh, r, s, dense[0], dense[1], self.w, self.h)
        got = [q.download().view(U32) for q in nodes]
        for g in got[:3 if score else 2]:
            assert (g[nh:] == POISON).all() and (g[:, nw:] == POISON).all(), "written beyond the grid"
        if not score:
            assert (got[2] == POISON).all()
        out = [q.download().view(U32) for q in dense]
        for g in out:
            assert (g[self.h:] == POISON).all() and (g[:, self.w:] == POISON).all(), "written beyond the frame"
        result = [g[:nh, :nw] for g in got] + [record.download(8, 1).tobytes()] + [g[:self.h, :self.w] for g in out]
        for q in nodes + dense + [record]:
            q.free()
            ctx._planes.remove(q)
        return result


def check(ctx, f0, f1, r, d, s, what, lo=0.0, scale=1.0, cut=-1.0, pair=None):
    """One case against the restatement, node field, record and expansion; returns the restatement's (u, v, score, record)."""
    wu, wv, ws, record, _ = correlate_reference(f0, f1, lo, scale, r, d, s, cut)
    eu, ev = expand_reference(wu, wv, r, s, f0.shape[1], f0.shape[0])
    pair = pair or Pair(ctx, f0, f1)
    gu, gv, gs, grec, xu, xv = pair.run(r, d, s, lo, scale, cut)
    for got, want, name in ((gu, wu, "u"), (gv, wv, "v"), (gs, ws, "score"), (xu, eu, "expanded u"), (xv, ev, "expanded v")):
        same = got == bits(want)
        assert same.all(), "%s: %s differs at %d places, first (y, x) = %s: %s, want %s" % (
            what, name, (~same).sum(), np.argwhere(~same)[0], got[~same][0].view(F32), bits(want)[~same][0].view(F32))
    assert grec == record.tobytes(), "%s: record %s, want %s" % (what, np.frombuffer(grec, RECORD_DTYPE), record)
    return wu, wv, ws, record[0]


@pytest.mark.parametrize("r,d,s", [(3, 2, 1), (1, 1, 3), (15, 32, 64)])
def test_one_window_and_one_pixel_past_it(flow2d, ctx, r, d, s):
    """A frame of exactly one window: one node, only displacement 0, unrefined.  One pixel more in x, in y and in both."""
    side = 2 * r + 1
    for dw, dh in ((0, 0), (1, 0), (0, 1), (1, 1)):
        f0, f1 = random_frames(side + dw, side + dh, seed=3 + dw + 2 * dh, shift=(dw, 0))
        _, _, _, rec = check(ctx, f0, f1, r, d, s, "%dx%d r %d" % (side + dw, side + dh, r))
        nw, nh = grid(side + dw, side + dh, r, s)
        assert rec["nodes"] == nw * nh and rec["invalid"] == 0
        if (dw, dh) == (0, 0):
            assert tuple(rec) == (1, 0, 0, 1)


@pytest.mark.parametrize("r", [1, 2, 3])
def test_dense_grid(flow2d, ctx, r):
    """65 x 17, spacing 1: one column past a wave, several tiles of 8 x 8 nodes with a ragged last one, a range that reaches
    beyond the frame from every node of the top and bottom rows."""
    f0, f1 = random_frames(65, 17, seed=r)
    _, _, _, rec = check(ctx, f0, f1, r, 3, 1, "65x17 r %d" % r)
    assert rec["nodes"] == (65 - 2 * r) * (17 - 2 * r) and rec["invalid"] == 0 and 0 < rec["unrefined"] < rec["nodes"]


@pytest.mark.parametrize("w,h,settings", [(130, 37, ((7, 8, 8), (15, 32, 5), (4, 3, 1))), (300, 200, ((7, 8, 8), (4, 3, 1)))])
def test_more_than_one_tile(flow2d, ctx, w, h, settings):
    f0, f1 = random_frames(w, h, seed=7, shift=(3, -2))
    pair = Pair(ctx, f0, f1)
    for r, d, s in settings:
        wu, wv, _, rec = check(ctx, f0, f1, r, d, s, "%dx%d (%d, %d, %d)" % (w, h, r, d, s), pair=pair)
        assert rec["invalid"] == 0 and np.rint(np.nanmedian(wu)) == 3
        if h == 200:  # (the nodes of the short frame's top row cannot reach dy = -2)
            assert np.rint(np.nanmedian(wv)) == -2


@pytest.mark.parametrize("r,d,s", [(7, 4, 8), (2, 3, 1), (2, 3, 64), (3, 2, 16), (1, 2, 5)])
def test_one_node_past_the_tile(flow2d, ctx, r, d, s):
    """tile_nodes(s) + 1 nodes in x and 2 tile_nodes(s) + 1 in y: a last tile of one node column and one node row."""
    t = tile_nodes(s)
    assert t == {8: 4, 1: 8, 64: 2, 16: 2, 5: 6}[s]
    w, h = 2 * r + 1 + t * s, 2 * r + 1 + 2 * t * s
    assert grid(w, h, r, s) == (t + 1, 2 * t + 1)
    f0, f1 = random_frames(w, h, seed=s, shift=(-1, 1))
    check(ctx, f0, f1, r, d, s, "%dx%d s %d" % (w, h, s))
    # ... and one pixel short of the next node
    f0, f1 = random_frames(w + s - 1, h + s - 1, seed=s + 1, shift=(-1, 1))
    assert grid(w + s - 1, h + s - 1, r, s) == (t + 1, 2 * t + 1)
    check(ctx, f0, f1, r, d, s, "%dx%d s %d" % (w + s - 1, h + s - 1, s))


def test_flat_saturated_and_non_finite_frames(flow2d, ctx):
    w, h, r, d, s = 70, 33, 3, 4, 3
    f0, f1 = random_frames(w, h, seed=12)
    flat = np.full((h, w), 100.0, F32)
    _, _, ws, rec = check(ctx, flat, f1, r, d, s, "flat frame 0")
    assert rec["invalid"] == rec["nodes"] and (ws == 0).all()
    _, _, _, rec = check(ctx, f0, flat, r, d, s, "flat frame 1")
    assert rec["invalid"] == rec["nodes"]
    # part of each frame flat: some nodes invalid, some candidates missing, peaks without all four neighbours
    a0, a1 = f0.copy(), f1.copy()
    a0[5:20, 10:30] = 31.0
    a1[12:30, 40:66] = 200.0
    _, _, _, rec = check(ctx, a0, a1, r, d, s, "flat patches")
    assert 0 < rec["invalid"] < rec["nodes"]
    # a saturated region: the range 40 .. 140 onto 0 .. 255, the rest clamps to 0 and 255 (whole windows of either are flat)
    b0, b1 = f0.copy(), f1.copy()
    b0[0:14, 0:30], b1[0:16, 0:34] = 250.0, 251.0
    b0[20:, 50:], b1[18:, 48:] = 3.0, -7.0
    _, _, _, rec = check(ctx, b0, b1, r, d, s, "saturated", lo=40.0, scale=2.55)
    assert 0 < rec["invalid"] < rec["nodes"]
    # NaN, infinities and -0 among the samples; a scale and lo that are no round numbers
    c0, c1 = f0.copy(), f1.copy()
    rng = np.random.default_rng(2)
    for frame in (c0, c1):
        for value in (np.nan, np.inf, -np.inf, -0.0, 254.5, 255.0, 1e30, -1e30):
            frame[rng.integers(0, h, 6), rng.integers(0, w, 6)] = value
    check(ctx, c0, c1, r, d, s, "non-finite")
    check(ctx, c0, c1, r, d, s, "non-finite, scaled", lo=-3.7, scale=0.913)


def test_periodic_pattern_ties(flow2d, ctx):
    """Period 4 in x and 3 in y, range 6: many displacements score the same double; the order of the header decides."""
    h, w = 40, 44
    y, x = np.mgrid[0:h, 0:w]
    f0 = (40 * (x % 4) + 25 * (y % 3) + 7 * ((x % 4) * (y % 3))).astype(F32)
    for shift in (0, 1, 2):
        wu, wv, _, rec = check(ctx, f0, np.roll(f0, shift, axis=1), 3, 6, 2, "period, moved by %d" % shift)
        assert rec["invalid"] == 0
    # (moved by 2: -2 and 2 tie in score and length, the smaller dx wins where it is a candidate)
    assert (np.rint(wu[:, 2:-2]) == -2).all() and (np.rint(wu[:, 0]) == 2).all() and (np.rint(wv) == 0).all()
    # two periodic frames that only partly agree
    g = f0.copy()
    g[10:25, 12:30] += 9
    check(ctx, f0, g, 2, 5, 1, "period, disturbed")


def test_min_score_rejects_some_nodes(flow2d, ctx):
    f0, f1 = random_frames(90, 50, seed=9, noise=60.0)
    _, _, ws, _ = check(ctx, f0, f1, 3, 3, 4, "no minimum")
    cut = float(np.median(ws))
    wu, _, _, rec = check(ctx, f0, f1, 3, 3, 4, "minimum %g" % cut, cut=cut)
    assert 0 < rec["rejected"] < rec["nodes"] and rec["invalid"] == 0 and np.isnan(wu).sum() == rec["rejected"]
    _, _, _, rec = check(ctx, f0, f1, 3, 3, 4, "minimum 2", cut=2.0)
    assert rec["rejected"] == rec["nodes"] and rec["unrefined"] == 0
    # without a score plane the vectors and the record are the same
    pair = Pair(ctx, f0, f1)
    a, b = pair.run(3, 3, 4, cut=cut), pair.run(3, 3, 4, cut=cut, score=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3]


@pytest.mark.parametrize("w,h", [(9, 40), (40, 9), (7, 7)])
def test_expansion_of_one_node_row_or_column(flow2d, ctx, w, h):
    f0, f1 = random_frames(w, h, seed=w, shift=(0, 0))
    f0[:, :] += np.linspace(0, 20, w, dtype=F32)[None, :]
    check(ctx, f0, f1, 3, 2, 4, "%dx%d" % (w, h))
    assert 1 in grid(w, h, 3, 4)
    # a node plane of the caller's own with invalid nodes in it: any nw, nh, any values
    nw, nh = (1, 6) if w < h else (6, 1) if h < w else (1, 1)
    nu = np.array([1.5, np.nan, -2.0, 1e9, np.inf, 4.0], F32)[:nw * nh].reshape(nh, nw)
    nv = np.array([0.5, 1.0, np.nan, -1.0, 2.0, -0.0], F32)[:nw * nh].reshape(nh, nw)
    pu, pv = ctx.plane(nw + 5, nh + 3, np.pad(nu, ((0, 3), (0, 5)), constant_values=np.nan)), ctx.plane(nw + 5, nh + 3, np.pad(nv, ((0, 3), (0, 5)), constant_values=np.nan))
    ou, ov = (ctx.plane(45, 45).fill_bytes(0x7F) for _ in range(2))
    ctx.expand_nodes(pu, pv, nw, nh, 2, 5, ou, ov, 40, 38)
    eu, ev = expand_reference(nu, nv, 2, 5, 40, 38)
    gu, gv = ou.download().view(U32), ov.download().view(U32)
    assert np.array_equal(gu[:38, :40], bits(eu)) and np.array_equal(gv[:38, :40], bits(ev))
    assert (gu[38:] == POISON).all() and (gu[:, 40:] == POISON).all() and (gv[38:] == POISON).all() and (gv[:, 40:] == POISON).all()


def test_a_replayed_graph_gives_the_eager_bytes(flow2d, ctx):
    w, h, r, d, s = 130, 37, 4, 5, 3
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    f0, f1 = random_frames(w, h, seed=21)
    pair = Pair(ctx, f0, f1)
    eager = pair.run(r, d, s, cut=0.2)
    nw, nh = grid(w, h, r, s)
    nodes = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(3)]
    dense = [ctx.plane(pair.cw, pair.ch).fill_bytes(0x7F) for _ in range(2)]
    record = ctx.correlation_records().fill_bytes(0x7F)
    snapshot = lambda: ([q.download(nw, nh).view(U32) for q in nodes] + [record.download(8, 1).tobytes()] +  # noqa: E731
                        [q.download(w, h).view(U32) for q in dense])
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    try:
        ctx.correlate(pair.f0, pair.f1, w, h, 0.0, 1.0, r, d, s, 0.2, nodes[0], nodes[1], nodes[2], record)
        ctx.expand_nodes(nodes[0], nodes[1], nw, nh, r, s, dense[0], dense[1], w, h)
    finally:
        graph = vp()
        assert lib.flow2d_capture_end(ctx.handle, ctypes.byref(graph)) == 0
    try:
        ctx.synchronize()
        assert (snapshot()[0] == POISON).all() and set(snapshot()[3]) == {0x7F}  # captured, not run
        for _ in range(2):
            for q in nodes + dense + [record]:
                q.fill_bytes(0x3C)
            assert lib.flow2d_graph_launch(ctx.handle, graph) == 0
            ctx.synchronize()
            got = snapshot()
            for k in (0, 1, 2, 4, 5):
                assert np.array_equal(got[k], eager[k]), k
            assert got[3] == eager[3]
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)


@pytest.mark.parametrize("kind", ["contiguous", "rows", "bytes"])
def test_lock_step_batch(flow2d, ctx, kind):
    """Three instances `stride` apart, the node planes laid out like the frames: planes and record of instance b are the bytes of
    the same pair correlated alone and the restatement's, and every other word of the output allocations is what it was."""
    w, h, cw, ch, count, r, d, s = 130, 37, 140, 40, 3, 5, 4, 6
    stride = stride_of(kind, pitch_of(cw), ch)
    pairs = [random_frames(w, h, seed=30 + b, shift=(b - 1, 1)) for b in range(count)]
    pairs[1][0][6:24, 30:60] = 50.0  # invalid nodes in one instance only
    nw, nh = grid(w, h, r, s)
    new = lambda: Tall(ctx, cw, ch, count, stride)  # noqa: E731
    t0, t1 = new().fill([p[0] for p in pairs]), new().fill([p[1] for p in pairs])
    nu, nv, ns, du, dv = (new() for _ in range(5))
    records = ctx.correlation_records(count).fill_bytes(0x7F)
    with ctx.set_batch(count, stride):
        ctx.correlate(t0, t1, w, h, 0.0, 1.0, r, d, s, 0.3, nu, nv, ns, records, instances=count)
        ctx.expand_nodes(nu, nv, nw, nh, r, s, du, dv, w, h)
    ctx.synchronize()
    refs = [correlate_reference(p[0], p[1], 0.0, 1.0, r, d, s, 0.3) for p in pairs]
    dense = [expand_reference(ref[0], ref[1], r, s, w, h) for ref in refs]
    for tall, k, name in ((nu, 0, "node u"), (nv, 1, "node v"), (ns, 2, "node score")):
        tall.check([ref[k] for ref in refs], "%s (%s)" % (name, kind))
    du.check([e[0] for e in dense], "expanded u (%s)" % kind)
    dv.check([e[1] for e in dense], "expanded v (%s)" % kind)
    t0.check(None, "frame 0")
    t1.check(None, "frame 1")
    got = records.download(8 * count, 1).tobytes()
    assert refs[1][3]["invalid"][0] > 0 and refs[0][3]["invalid"][0] == 0
    for b, (p, ref) in enumerate(zip(pairs, refs)):
        assert got[32 * b:32 * b + 32] == ref[3].tobytes(), "record of instance %d" % b
        alone = Pair(ctx, *p).run(r, d, s, cut=0.3)
        assert np.array_equal(alone[0], bits(ref[0])) and np.array_equal(alone[1], bits(ref[1])) and np.array_equal(alone[2], bits(ref[2]))
        assert alone[3] == got[32 * b:32 * b + 32]
    # a written range must not meet a later instance of a frame or of another node plane
    lib = flow2d.hip_lib()

    def call(node_u, node_v):
        return lib.flow2d_correlate_2d(ctx.handle, t0.ptr, t1.ptr, w, h, t0.pitch, 0.0, 1.0, r, d, s, -1.0, node_u, node_v, ns.ptr, nu.pitch,
                                       records.ptr)

    with ctx.set_batch(count, stride):
        assert call(t1.ptr + 2 * stride, nv.ptr) == 1
        assert call(nu.ptr, nu.ptr + stride) == 1
        assert lib.flow2d_expand_nodes_2d(ctx.handle, nu.ptr, nv.ptr, nw, nh, nu.pitch, r, s, du.ptr, nv.ptr + 2 * stride, w, h, du.pitch) == 1
    ctx.synchronize()


def test_invalid_arguments_write_nothing(flow2d, ctx):
    w, h, r, d, s = 100, 40, 7, 8, 8
    lib = flow2d.hip_lib()
    f0, f1 = random_frames(w, h, seed=5)
    p0, p1 = ctx.plane(w, h, f0), ctx.plane(w, h, f1)
    nw, nh = grid(w, h, r, s)
    nu, nv, ns = (ctx.plane(nw, nh).fill_bytes(0x7F) for _ in range(3))
    ou, ov = (ctx.plane(w, h).fill_bytes(0x7F) for _ in range(2))
    record = ctx.correlation_records().fill_bytes(0x7F)
    span = p0.pitch * h
    nan, inf = float("nan"), float("inf")
    base = dict(f0=p0.ptr, f1=p1.ptr, w=w, h=h, pitch=p0.pitch, lo=0.0, scale=1.0, r=r, d=d, s=s, cut=-1.0, nu=nu.ptr, nv=nv.ptr, ns=ns.ptr,
                npitch=nu.pitch, record=record.ptr)

    def call(**kw):
        a = dict(base, **kw)
        return lib.flow2d_correlate_2d(ctx.handle, a["f0"], a["f1"], a["w"], a["h"], a["pitch"], a["lo"], a["scale"], a["r"], a["d"],
                                       a["s"], a["cut"], a["nu"], a["nv"], a["ns"], a["npitch"], a["record"])

    bad = [dict(r=0), dict(r=16), dict(d=0), dict(d=33), dict(s=0), dict(s=65), dict(scale=0.0), dict(scale=-2.0), dict(scale=nan),
           dict(scale=inf), dict(lo=nan), dict(lo=inf), dict(cut=nan), dict(f0=None), dict(f1=None), dict(nu=None), dict(nv=None), dict(w=0),
           dict(h=0), dict(w=14), dict(h=14), dict(pitch=p0.pitch + 8), dict(pitch=16), dict(npitch=16), dict(npitch=nu.pitch + 4),
           dict(nu=p0.ptr), dict(nv=p1.ptr + span - p0.pitch), dict(ns=p0.ptr + p0.pitch), dict(nv=nu.ptr), dict(ns=nv.ptr),
           dict(record=record.ptr + 4), dict(record=p0.ptr + 64), dict(record=nu.ptr)]
    for kw in bad:
        assert call(**kw) == 1, kw

    def expand(**kw):
        a = dict(dict(nu=nu.ptr, nv=nv.ptr, nw=nw, nh=nh, npitch=nu.pitch, r=r, s=s, ou=ou.ptr, ov=ov.ptr, w=w, h=h, pitch=ou.pitch), **kw)
        return lib.flow2d_expand_nodes_2d(ctx.handle, a["nu"], a["nv"], a["nw"], a["nh"], a["npitch"], a["r"], a["s"], a["ou"], a["ov"],
                                          a["w"], a["h"], a["pitch"])

    for kw in [dict(nu=None), dict(nv=None), dict(ou=None), dict(ov=None), dict(nw=0), dict(nh=0), dict(w=0), dict(h=0), dict(npitch=16),
               dict(pitch=16), dict(r=-1), dict(r=16), dict(s=0), dict(s=65), dict(ou=nu.ptr), dict(ov=nv.ptr), dict(ov=ou.ptr)]:
        assert expand(**kw) == 1, kw
    ctx.synchronize()
    for q in (nu, nv, ns, ou, ov):
        assert (q.download().view(U32) == POISON).all()
    assert set(record.download(8, 1).tobytes()) == {0x7F}
    assert call() == 0 and expand() == 0
    wu, wv, ws, rec, _ = correlate_reference(f0, f1, 0.0, 1.0, r, d, s)
    assert np.array_equal(nu.download().view(U32), bits(wu)) and np.array_equal(nv.download().view(U32), bits(wv))
    assert np.array_equal(ns.download().view(U32), bits(ws)) and record.download(8, 1).tobytes() == rec.tobytes()
    eu, ev = expand_reference(wu, wv, r, s, w, h)
    assert np.array_equal(ou.download().view(U32), bits(eu)) and np.array_equal(ov.download().view(U32), bits(ev))
    # the convenience form: arrays and the record read back; no record, no score
    gu, gv, gs, grec = ctx.correlate(p0, p1, w, h, 0.0, 1.0, r, d, s)
    assert np.array_equal(bits(gu), bits(wu)) and np.array_equal(bits(gv), bits(wv)) and np.array_equal(bits(gs), bits(ws))
    assert bytes(grec) == rec.tobytes()
    assert call(record=None, ns=None) == 0
    ctx.synchronize()


# ---- the host layer ---------------------------------------------------------------------------------------------------------------
def test_chain_equals_its_parts(flow2d, ctx):
    """OpticalFlow.correlate_device on a speckle pair is the two entries called by hand with the same planes, byte for byte; the
    host-image form chooses lo and scale from the frames and returns the same field; the restatement agrees with both."""
    r, d, s, cut = 7, 6, 8, 0.5
    sc = scenes_module().make_speckle_scene("affine", 96, 80, seed=1)
    h, w = sc.frame_0.shape
    # (a pair outside 0 .. 255, so that lo and scale are not the identity)
    frame_0, frame_1 = (sc.frame_0 * F32(3) - F32(100)).astype(F32), (sc.frame_1 * F32(3) - F32(100)).astype(F32)
    lo, scale = frame_range(frame_0, frame_1)
    assert lo != 0 and scale != 1
    nw, nh = grid(w, h, r, s)
    f0, f1 = ctx.plane(w, h, frame_0), ctx.plane(w, h, frame_1)
    new = lambda: ctx.plane(w, h).fill_bytes(0x7F)  # noqa: E731
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        nu, nv, ns, fu, fv = (new() for _ in range(5))
        rec = flow.correlate_device(f0.ptr, f1.ptr, lo, scale, r, d, s, cut, dev_nodes=(nu.ptr, nv.ptr), dev_score=ns.ptr,
                                    dev_flow=(fu.ptr, fv.ptr))
        # by hand
        hu, hv, hs, du, dv = (new() for _ in range(5))
        record = ctx.correlation_records().fill_bytes(0x7F)
        ctx.correlate(f0, f1, w, h, lo, scale, r, d, s, cut, hu, hv, hs, record)
        ctx.expand_nodes(hu, hv, nw, nh, r, s, du, dv, w, h)
        ctx.synchronize()
        for a, b in ((nu, hu), (nv, hv), (ns, hs), (fu, du), (fv, dv)):
            assert a.download().tobytes() == b.download().tobytes()
        assert (nu.download().view(U32)[nh:] == POISON).all() and (nu.download().view(U32)[:, nw:] == POISON).all()
        assert bytes(rec) == record.download(8, 1).tobytes()
        # the restatement
        wu, wv, ws, wrec, _ = correlate_reference(frame_0, frame_1, lo, scale, r, d, s, cut)
        eu, ev = expand_reference(wu, wv, r, s, w, h)
        assert np.array_equal(nu.download(nw, nh).view(U32), bits(wu)) and np.array_equal(ns.download(nw, nh).view(U32), bits(ws))
        assert np.array_equal(fu.download().view(U32), bits(eu)) and np.array_equal(fv.download().view(U32), bits(ev))
        assert bytes(rec) == wrec.tobytes() and rec.nodes == nw * nh
        err = interior_epe(wu, wv, sc, r, d, s)
        print("speckle affine, seed 1: interior mean EPE %.4f, record %s" % (np.nanmean(err), json.dumps(rec.summary())))
        # without the caller's node planes: the object's own, the same dense field; without anything but the record
        gu, gv = new(), new()
        rec2 = flow.correlate_device(f0.ptr, f1.ptr, lo, scale, r, d, s, cut, dev_flow=(gu.ptr, gv.ptr))
        assert gu.download().tobytes() == fu.download().tobytes() and gv.download().tobytes() == fv.download().tobytes()
        assert bytes(rec2) == bytes(rec) and bytes(flow.correlate_device(f0.ptr, f1.ptr, lo, scale, r, d, s, cut)) == bytes(rec)
        # the host-image form
        pu, pv, ps, prec, (plo, pscale), (qu, qv) = flow.correlate(frame_0, frame_1, r, d, s, cut, flow=True)
        assert (F32(plo), F32(pscale)) == (lo, scale)
        assert np.array_equal(bits(pu), bits(wu)) and np.array_equal(bits(pv), bits(wv)) and np.array_equal(bits(ps), bits(ws))
        assert np.array_equal(bits(qu), bits(eu)) and np.array_equal(bits(qv), bits(ev)) and bytes(prec) == bytes(rec)
        # 8-bit data is taken as it is
        _, _, _, _, identity = flow.correlate(sc.frame_0, sc.frame_1, r, d, s)
        assert identity == (0.0, 1.0)
        for bad in (dict(radius=0), dict(radius=16), dict(search=0), dict(search=33), dict(spacing=0), dict(spacing=65),
                    dict(min_score=float("nan"))):
            with pytest.raises(flow2d.Flow2DError):
                flow.correlate(frame_0, frame_1, **bad)
        for bad in (dict(lo=float("inf")), dict(scale=0.0), dict(scale=float("nan")), dict(radius=16)):
            with pytest.raises(flow2d.Flow2DError):
                flow.correlate_device(f0.ptr, f1.ptr, **dict(dict(lo=lo, scale=scale), **bad))
        with pytest.raises(flow2d.Flow2DError):  # a node plane that is a frame
            flow.correlate_device(f0.ptr, f1.ptr, lo, scale, r, d, s, dev_nodes=(f0.ptr, nv.ptr))
    finally:
        flow.close()
    H = flow2d.host_lib()
    assert H.flow2d_host_correlation_args_ok(96, 80, 0.0, 1.0, 7, 8, 8, -1.0) == 1
    assert H.flow2d_host_correlation_args_ok(15, 15, -5.0, 0.25, 7, 32, 64, 0.9) == 1
    for bad in ((14, 80, 0.0, 1.0, 7, 8, 8, -1.0), (96, 80, 0.0, 0.0, 7, 8, 8, -1.0), (96, 80, float("nan"), 1.0, 7, 8, 8, -1.0),
                (96, 80, 0.0, 1.0, 0, 8, 8, -1.0), (96, 80, 0.0, 1.0, 7, 33, 8, -1.0), (96, 80, 0.0, 1.0, 7, 8, 65, -1.0),
                (96, 80, 0.0, 1.0, 7, 8, 8, float("nan"))):
        assert H.flow2d_host_correlation_args_ok(*bad) == 0, bad


def test_cli_correlation(flow2d, ctx, tmp_path):
    """--correlation on a 96 x 80 speckle pair writes the expanded field of OpticalFlow.correlate where the flow is written and the
    nodes to files of their own, prints the grid and the record and, with --ground-truth, the score; a run without the flag
    neither prints the line nor writes node files; a bad option value or combination is a usage error."""
    w, h = 96, 80
    sc = scenes_module().make_speckle_scene("translation", w, h, seed=0)
    names = [str(tmp_path / "f0.raw"), str(tmp_path / "f1.raw")]
    sc.frame_0.tofile(names[0])
    sc.frame_1.tofile(names[1])
    truth = str(tmp_path / "truth.flo")
    flow2d.write_flo(truth, sc.gt_u, sc.gt_v)

    def run(options, out):
        out.mkdir()
        q = subprocess.run([flow2d.CLI_PATH] + options + names + [str(w), str(h), "t_", str(out) + "/"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=300)
        return q, {f.name: f.read_bytes() for f in out.iterdir()}

    options = ["--correlation", "7", "--correlation-range", "6", "--correlation-spacing", "8", "--correlation-min-score", "0.25"]
    q, files = run(["--flo", "--ground-truth", truth] + options, tmp_path / "correlation")
    assert q.returncode == 0, q.stdout[-2000:]
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        nu, nv, ns, rec, (lo, scale), (fu, fv) = flow.correlate(sc.frame_0, sc.frame_1, 7, 6, 8, 0.25, flow=True)
    finally:
        flow.close()
    nw, nh = grid(w, h, 7, 8)
    assert files["t_flow-u-96-80.raw"] == fu.tobytes() and files["t_flow-v-96-80.raw"] == fv.tobytes()
    assert files["t_node-u-%d-%d.raw" % (nw, nh)] == nu.tobytes() and files["t_node-v-%d-%d.raw" % (nw, nh)] == nv.tobytes()
    assert files["t_node-score-%d-%d.raw" % (nw, nh)] == ns.tobytes()
    gu, gv = flow2d.read_flo(str(tmp_path / "correlation" / "t_flow.flo"))
    assert gu.tobytes() == fu.tobytes() and gv.tobytes() == fv.tobytes()
    assert {"t_res.pgm", "t_amp-96-80.raw"} <= set(files)
    line = [x for x in q.stdout.splitlines() if x.startswith("Correlation: ")]
    assert len(line) == 1, q.stdout[-2000:]
    printed = json.loads(line[0][len("Correlation: "):])
    assert printed == dict(rec.summary(), radius=7, range=6, spacing=8, min_score=0.25, lo=lo, scale=scale, nw=nw, nh=nh)
    scores = [x for x in q.stdout.splitlines() if x.startswith("Flow error: ")]
    assert len(scores) == 1
    err = interior_epe(nu, nv, sc, 7, 6, 8)
    assert np.isfinite(err).all() and err.mean() <= 0.15
    plain, plain_files = run(["--flo"], tmp_path / "plain")
    assert plain.returncode == 0 and "Correlation: " not in plain.stdout and not [f for f in plain_files if "node" in f]
    assert plain_files["t_flow-u-96-80.raw"] != files["t_flow-u-96-80.raw"]
    for bad in (["--correlation", "0"], ["--correlation", "16"], ["--correlation"], ["--correlation", "x"],
                ["--correlation", "7", "--correlation-range", "33"], ["--correlation", "7", "--correlation-spacing", "0"],
                ["--correlation", "7", "--correlation-min-score", "nan"], ["--correlation", "7", "--backward"],
                ["--correlation", "7", "--refine", "3"]):
        q = subprocess.run([flow2d.CLI_PATH] + bad + names + [str(w), str(h), "t_"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert q.returncode == 5, (bad, q.stdout[-500:])
