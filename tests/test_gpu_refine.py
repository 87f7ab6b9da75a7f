"""flow2d_refine_flow_2d on the device against its numpy restatement (tests/test_refine_cpu.py), bit for bit: frames smaller than
the window and one column or row past a workgroup tile, every radius, every combination of guide, mask and spatial weight,
containers larger than the frame with NaN in the padding, unusable vectors, wild mask values, heavy ties, a fully masked frame,
the record; the same bytes from a replayed graph and from an instance alone or in a lock-step batch; the refusals on a real
context; OpticalFlow.refine_flow_device against its parts; the CLI."""
import ctypes
import itertools
import json
import subprocess

import numpy as np
import pytest

from test_gpu_batch_kernels import Tall, pitch_of, stride_of
from test_gpu_denoise import CLI_PARAMS
from test_gpu_tracking import scenes_module
from test_refine_cpu import F32, RECORD_DTYPE, U32, bits, random_case, refine_passes, refine_reference

pytestmark = pytest.mark.gpu
POISON = U32(0x7F7F7F7F)
SIGMA_GUIDE, SIGMA_SPACE = 30.0, 2.5
COMBINATIONS = list(itertools.product((False, True), repeat=3))  # guide, mask, spatial weight


class Frame:
    """The inputs of a case in containers 5 columns wider and 3 rows taller than the frame, the padding NaN."""

    def __init__(self, ctx, u, v, guide, mask):
        self.ctx = ctx
        self.h, self.w = u.shape
        self.cw, self.ch = self.w + 5, self.h + 3
        self.u, self.v = self.container(u), self.container(v)
        self.guide = None if guide is None else self.container(guide)
        self.mask = None if mask is None else self.container(mask)

    def container(self, a):
        full = np.full((self.ch, self.cw), np.nan, F32)
        full[:self.h, :self.w] = a
        return self.ctx.plane(self.cw, self.ch, full)

    def run(self, r, sigma_guide=0.0, sigma_space=0.0, guide=True, mask=True):
        """(u bits, v bits, record bytes) of one call into poisoned outputs, which must stay poisoned beyond the frame."""
        ou, ov = (self.ctx.plane(self.cw, self.ch).fill_bytes(0x7F) for _ in range(2))
        record = self.ctx.refine_records().fill_bytes(0x7F)
        self.ctx.refine_flow(self.u, self.v, self.w, self.h, r, self.guide if guide else None, self.mask if mask else None, sigma_guide,
                             sigma_space, ou, ov, record)
        got = [q.download().view(U32) for q in (ou, ov)]
        for g in got:
            assert (g[self.h:] == POISON).all() and (g[:, self.w:] == POISON).all(), "written beyond the frame"
        return got[0][:self.h, :self.w], got[1][:self.h, :self.w], record.download(8, 1).tobytes()


def check(frame, case, r, use_guide, use_mask, use_space, what):
    u, v, guide, mask = case
    sg, ss = (SIGMA_GUIDE if use_guide else 0.0), (SIGMA_SPACE if use_space else 0.0)
    wu, wv, record = refine_reference(u, v, guide if use_guide else None, mask if use_mask else None, r, sg, ss)
    gu, gv, grec = frame.run(r, sg, ss, use_guide, use_mask)
    for got, want, name in ((gu, wu, "u"), (gv, wv, "v")):
        same = got == bits(want)
        assert same.all(), "%s: %s differs at %d pixels, first (y, x) = %s" % (what, name, (~same).sum(), np.argwhere(~same)[0])
    assert grec == record.tobytes(), "%s: record %s, want %s" % (what, np.frombuffer(grec, RECORD_DTYPE), record)
    return record[0]


@pytest.mark.parametrize("w,h", [(1, 1), (1, 9), (9, 1), (5, 3)])
def test_frames_smaller_than_the_window(flow2d, ctx, w, h):
    case = random_case(w, h, seed=11, wild=False)
    frame = Frame(ctx, *case)
    for r in (1, 7):
        for combo in ((False, False, False), (True, True, True)):
            check(frame, case, r, *combo, "%dx%d r %d %s" % (w, h, r, combo))
    wild = random_case(w, h, seed=12)
    check(Frame(ctx, *wild), wild, 7, True, True, True, "%dx%d wild" % (w, h))


@pytest.mark.parametrize("r", range(1, 8))
def test_every_radius_and_combination(flow2d, ctx, r):
    """65 x 17: one column past a wave and a workgroup's tile, one row past its 16; NaN, infinite and sentinel vectors, -0, mask
    values outside [0, 1] and NaN, NaN in the guide."""
    case = random_case(65, 17)
    frame = Frame(ctx, *case)
    for combo in COMBINATIONS:
        rec = check(frame, case, r, *combo, "65x17 r %d %s" % (r, combo))
        assert rec["pixels"] == 65 * 17 and rec["changed"] > 0 and (rec["filled"] > 0) == combo[1]
    # a guide with sigma 0 is no guide, bit for bit
    a = frame.run(r, 0.0, SIGMA_SPACE, True, True)
    b = frame.run(r, 0.0, SIGMA_SPACE, False, True)
    assert all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and a[2] == b[2]


@pytest.mark.parametrize("w,h,radii", [(130, 37, (2, 7)), (300, 200, (5,))])
def test_more_than_one_tile(flow2d, ctx, w, h, radii):
    case = random_case(w, h)
    frame = Frame(ctx, *case)
    for r in radii:
        check(frame, case, r, True, True, True, "%dx%d r %d" % (w, h, r))
        check(frame, case, r, False, False, False, "%dx%d r %d plain" % (w, h, r))


def test_heavy_ties(flow2d, ctx):
    """A flow quantised to three values (and -0 among them): the cumulated weight jumps at each, whatever the selection does."""
    w, h = 65, 17
    rng = np.random.default_rng(5)
    _, _, guide, mask = random_case(w, h, wild=False)
    u = rng.choice(np.array([-1.5, -0.0, 2.25], F32), (h, w))
    v = rng.choice(np.array([0.0, 1e-30, 3.0], F32), (h, w))
    case = (u, v, guide, mask)
    frame = Frame(ctx, *case)
    for r, combo in ((1, (False, False, False)), (4, (True, True, False)), (7, (True, True, True))):
        check(frame, case, r, *combo, "ties r %d" % r)


def test_fully_masked_frame_is_copied(flow2d, ctx):
    w, h = 70, 20
    u, v, guide, _ = random_case(w, h)
    case = (u, v, guide, np.ones((h, w), F32))
    rec = check(Frame(ctx, *case), case, 3, True, True, True, "fully masked")
    assert rec["unfilled"] == w * h and rec["filled"] == 0 and rec["changed"] == 0
    frame = Frame(ctx, *case)
    gu, gv, _ = frame.run(3, SIGMA_GUIDE, 0.0)
    assert np.array_equal(gu, bits(u)) and np.array_equal(gv, bits(v))


def test_smooth_and_outlier_windows(flow2d, ctx):
    """What the bisection's length depends on: a constant flow (no step), a smooth one, and one vector in a million."""
    w, h = 130, 37
    y, x = np.mgrid[0:h, 0:w].astype(F32)
    _, _, guide, mask = random_case(w, h, wild=False)
    smooth = (F32(4.5) + F32(0.001) * x, F32(-2.25) + F32(0.002) * y, guide, mask)
    const = (np.full((h, w), 4.5, F32), np.full((h, w), -2.25, F32), guide, mask)
    spiky = (smooth[0].copy(), smooth[1].copy(), guide, mask)
    spiky[0][::7, ::5] = -1e6
    spiky[1][3::9, 2::11] = 9e8
    for case, what in ((const, "constant"), (smooth, "smooth"), (spiky, "outliers")):
        check(Frame(ctx, *case), case, 5, True, True, False, what)


def test_a_replayed_graph_gives_the_eager_bytes(flow2d, ctx):
    w, h = 130, 37
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    case = random_case(w, h)
    frame = Frame(ctx, *case)
    eager = frame.run(6, SIGMA_GUIDE, SIGMA_SPACE)
    ou, ov = (ctx.plane(frame.cw, frame.ch).fill_bytes(0x7F) for _ in range(2))
    record = ctx.refine_records().fill_bytes(0x7F)
    snapshot = lambda: (ou.download(w, h).view(U32), ov.download(w, h).view(U32), record.download(8, 1).tobytes())  # noqa: E731
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    try:
        ctx.refine_flow(frame.u, frame.v, w, h, 6, frame.guide, frame.mask, SIGMA_GUIDE, SIGMA_SPACE, ou, ov, record)
    finally:
        graph = vp()
        assert lib.flow2d_capture_end(ctx.handle, ctypes.byref(graph)) == 0
    try:
        ctx.synchronize()
        assert (snapshot()[0] == POISON).all() and set(snapshot()[2]) == {0x7F}  # captured, not run
        for _ in range(2):
            for q in (ou, ov, record):
                q.fill_bytes(0x3C)
            assert lib.flow2d_graph_launch(ctx.handle, graph) == 0
            ctx.synchronize()
            got = snapshot()
            assert np.array_equal(got[0], eager[0]) and np.array_equal(got[1], eager[1]) and got[2] == eager[2]
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)


@pytest.mark.parametrize("kind", ["contiguous", "rows", "bytes"])
def test_lock_step_batch(flow2d, ctx, kind):
    """Three instances `stride` apart: planes and record of instance b are the bytes of the same input refined alone and the
    restatement's, and every other word of the output allocations is what it was."""
    w, h, cw, ch, count = 130, 37, 140, 40, 3
    stride = stride_of(kind, pitch_of(cw), ch)
    cases = [random_case(w, h, seed=20 + b) for b in range(count)]
    fill = lambda arrays: Tall(ctx, cw, ch, count, stride).fill(arrays)  # noqa: E731
    tu, tv, tg, tm = (fill([c[k] for c in cases]) for k in range(4))
    ou, ov = Tall(ctx, cw, ch, count, stride), Tall(ctx, cw, ch, count, stride)
    records = ctx.refine_records(count).fill_bytes(0x7F)
    with ctx.set_batch(count, stride):
        ctx.refine_flow(tu, tv, w, h, 4, tg, tm, SIGMA_GUIDE, SIGMA_SPACE, ou, ov, records, instances=count)
    ctx.synchronize()
    refs = [refine_reference(*c, 4, SIGMA_GUIDE, SIGMA_SPACE) for c in cases]
    ou.check([r[0] for r in refs], "u (%s)" % kind)
    ov.check([r[1] for r in refs], "v (%s)" % kind)
    for t in (tu, tv, tg, tm):
        t.check(None, "an input")
    got = records.download(8 * count, 1).tobytes()
    for b, (c, ref) in enumerate(zip(cases, refs)):
        assert got[32 * b:32 * b + 32] == ref[2].tobytes(), "record of instance %d" % b
        planes = [ctx.plane(cw, ch, a) for a in c]
        au, av = (ctx.plane(cw, ch).fill_bytes(0x7F) for _ in range(2))
        alone = ctx.refine_records().fill_bytes(0x7F)
        ctx.refine_flow(planes[0], planes[1], w, h, 4, planes[2], planes[3], SIGMA_GUIDE, SIGMA_SPACE, au, av, alone)
        assert np.array_equal(au.download(w, h).view(U32), bits(ref[0])) and np.array_equal(av.download(w, h).view(U32), bits(ref[1]))
        assert alone.download(8, 1).tobytes() == got[32 * b:32 * b + 32]
    # a written range must not meet a later instance of an input or of the other output
    lib = flow2d.hip_lib()

    def call(out_u, out_v):
        return lib.flow2d_refine_flow_2d(ctx.handle, tu.ptr, tv.ptr, tg.ptr, tm.ptr, w, h, tu.pitch, 4, SIGMA_GUIDE, SIGMA_SPACE, out_u,
                                         out_v, records.ptr)

    with ctx.set_batch(count, stride):
        assert call(tg.ptr + 2 * stride, ov.ptr) == 1
        assert call(ou.ptr, ou.ptr + stride) == 1
    ctx.synchronize()


def test_invalid_arguments_write_nothing(flow2d, ctx):
    w, h = 100, 40
    lib = flow2d.hip_lib()
    case = random_case(w, h)
    pu, pv, pg, pm = (ctx.plane(w, h, a) for a in case)
    ou, ov = (ctx.plane(w, h).fill_bytes(0x7F) for _ in range(2))
    record = ctx.refine_records().fill_bytes(0x7F)
    span = pu.pitch * h
    d = dict(u=pu.ptr, v=pv.ptr, guide=pg.ptr, mask=pm.ptr, w=w, h=h, pitch=pu.pitch, r=3, sg=SIGMA_GUIDE, ss=SIGMA_SPACE, ou=ou.ptr,
             ov=ov.ptr, record=record.ptr)

    def call(**kw):
        a = dict(d, **kw)
        return lib.flow2d_refine_flow_2d(ctx.handle, a["u"], a["v"], a["guide"], a["mask"], a["w"], a["h"], a["pitch"], a["r"], a["sg"],
                                         a["ss"], a["ou"], a["ov"], a["record"])

    bad = [dict(r=0), dict(r=8), dict(r=-3), dict(sg=-1.0), dict(ss=-1.0), dict(sg=float("nan")), dict(ss=float("inf")), dict(u=None),
           dict(v=None), dict(ou=None), dict(ov=None), dict(w=0), dict(h=0), dict(pitch=pu.pitch + 8), dict(pitch=16),
           dict(ou=pu.ptr), dict(ou=pu.ptr + span - pu.pitch), dict(ou=pg.ptr), dict(ov=pv.ptr), dict(ov=pm.ptr), dict(ov=ou.ptr),
           dict(record=record.ptr + 4), dict(record=pu.ptr + 64), dict(record=ou.ptr)]
    for kw in bad:
        assert call(**kw) == 1, kw
    ctx.synchronize()
    for q in (ou, ov):
        assert (q.download().view(U32) == POISON).all()
    assert set(record.download(8, 1).tobytes()) == {0x7F}
    assert call() == 0
    wu, wv, rec = refine_reference(*case, 3, SIGMA_GUIDE, SIGMA_SPACE)
    assert np.array_equal(ou.download().view(U32), bits(wu)) and np.array_equal(ov.download().view(U32), bits(wv))
    assert record.download(8, 1).tobytes() == rec.tobytes()
    # the convenience form: arrays and the record read back; no record at all
    gu, gv, grec = ctx.refine_flow(pu, pv, w, h, 3, pg, pm, SIGMA_GUIDE, SIGMA_SPACE)
    assert np.array_equal(bits(gu), bits(wu)) and np.array_equal(bits(gv), bits(wv)) and bytes(grec) == rec.tobytes()
    assert call(record=None) == 0
    ctx.synchronize()


# ---- the host layer ---------------------------------------------------------------------------------------------------------------
SMALL_FRAME_PARAMS = (50, 0.9, 40, 5, 5.0, 0.001, 0.001, 3, 0.8)  # a 64 x 64 frame: test_gpu_segmentation.py


def test_chain_equals_its_parts(flow2d, ctx):
    """OpticalFlow.refine_flow_device on `two_layer` at 64 x 64 is the bidirectional flow and the kernel called by hand with the same
    planes -- frame 0 the guide, the forward mask applied in every pass --, byte for byte, for 1, 2 and 3 passes; without masks the
    plain flow; and a flow the caller computed elsewhere is refined as it is."""
    sc = scenes_module().make_scene("two_layer", 64, 64, seed=0)
    h, w = sc.frame_0.shape
    f0, f1 = ctx.plane(w, h, sc.frame_0), ctx.plane(w, h, sc.frame_1)
    new = lambda: ctx.plane(w, h).fill_bytes(0x7F)  # noqa: E731
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        p = flow.params(*SMALL_FRAME_PARAMS)
        u, v, bu, bv, of, ob = (new() for _ in range(6))
        flow.compute_flow_bidirectional_device([f0.ptr, f1.ptr], [u.ptr], [v.ptr], [bu.ptr], [bv.ptr], p, [of.ptr], [ob.ptr])
        ctx.synchronize()
        for masks, iterations, r, sg, ss in ((True, 1, 5, 25.0, 0.0), (True, 2, 3, 20.0, 3.0), (True, 3, 2, 0.0, 0.0), (False, 2, 4, 25.0, 0.0)):
            what = "masks %s, %d passes" % (masks, iterations)
            ru, rv, fu, fv, fm = (new() for _ in range(5))
            rec = flow.refine_flow_device(f0.ptr, f1.ptr, (ru.ptr, rv.ptr), p, r, sg, ss, iterations, masks, dev_flow=(fu.ptr, fv.ptr),
                                          dev_mask=fm.ptr if masks else None)
            # by hand
            if masks:
                cu, cv, cm = u, v, of
            else:
                cu, cv, cm = new(), new(), None
                flow.compute_flow_device(f0.ptr, f1.ptr, cu.ptr, cv.ptr, p)
                ctx.synchronize()
            assert fu.download().tobytes() == cu.download().tobytes() and fv.download().tobytes() == cv.download().tobytes(), what
            if masks:
                assert fm.download().tobytes() == of.download().tobytes(), what
            record = ctx.refine_records().fill_bytes(0x7F)
            a = (cu, cv)
            for _ in range(iterations):
                b = (new(), new())
                ctx.refine_flow(a[0], a[1], w, h, r, f0, cm, sg, ss, b[0], b[1], record)
                a = b
            assert ru.download().tobytes() == a[0].download().tobytes() and rv.download().tobytes() == a[1].download().tobytes(), what
            assert bytes(rec) == record.download(8, 1).tobytes(), what
            # ... and the restatement on the downloaded flow
            wu, wv, wrec = refine_passes(cu.download(), cv.download(), sc.frame_0, cm.download() if cm else None, r, sg, ss, iterations)
            assert np.array_equal(ru.download().view(U32), bits(wu)) and np.array_equal(rv.download().view(U32), bits(wv)), what
            assert bytes(rec) == wrec.tobytes(), what
            print(what, json.dumps(rec.summary()))
        # a flow computed elsewhere: the true flow with the occluded pixels set to the square's motion, the true occlusion mask
        gu, gv = sc.gt_u.copy(), sc.gt_v.copy()
        gu[sc.occlusion > 0], gv[sc.occlusion > 0] = 4.5, -2.25
        du, dv, dm, ru, rv = ctx.plane(w, h, gu), ctx.plane(w, h, gv), ctx.plane(w, h, sc.occlusion), new(), new()
        rec = flow.refine_flow_device(f0.ptr, None, (ru.ptr, rv.ptr), p, 5, 25.0, 0.0, 2, True, dev_flow=(du.ptr, dv.ptr), dev_mask=dm.ptr,
                                      flow_given=True)
        wu, wv, wrec = refine_passes(gu, gv, sc.frame_0, sc.occlusion, 5, 25.0, 0.0, 2)
        assert np.array_equal(ru.download().view(U32), bits(wu)) and np.array_equal(rv.download().view(U32), bits(wv))
        assert bytes(rec) == wrec.tobytes() and rec.filled > 0
        assert du.download().tobytes() == gu.tobytes()  # the caller's flow is read, not written
        # the host-image form returns the same flow and record as the device form
        ru, rv = new(), new()
        rec = flow.refine_flow_device(f0.ptr, f1.ptr, (ru.ptr, rv.ptr), p, 5, 25.0, 0.0, 1, True)
        hu, hv, hrec, (pu, pv) = flow.refine_flow(sc.frame_0, sc.frame_1, p, 5, 25.0, 0.0, 1, True, flow=True)
        assert hu.tobytes() == ru.download().tobytes() and hv.tobytes() == rv.download().tobytes() and bytes(hrec) == bytes(rec)
        assert pu.tobytes() == u.download().tobytes() and pv.tobytes() == v.download().tobytes()
        for bad in (dict(radius=0), dict(radius=8), dict(sigma_guide=-1.0), dict(sigma_space=float("nan")), dict(iterations=0),
                    dict(iterations=17)):
            with pytest.raises(flow2d.Flow2DError):
                flow.refine_flow(sc.frame_0, sc.frame_1, p, **bad)
        with pytest.raises(flow2d.Flow2DError):  # the filter reads a window: not in place
            flow.refine_flow_device(f0.ptr, None, (du.ptr, dv.ptr), p, dev_flow=(du.ptr, dv.ptr), flow_given=True)
    finally:
        flow.close()


def test_cli_refine(flow2d, ctx, tmp_path):
    """--refine on a 96 x 64 `two_layer` pair writes the flow of OpticalFlow.refine_flow where the flow is written, prints its
    record and, with --ground-truth, both scores; every other file is that of a run of the same binary without the flag, whose
    flow files hold the flow as computed; a bad option value is a usage error."""
    w, h = 96, 64
    sc = scenes_module().make_scene("two_layer", w, h, seed=0)
    names = [str(tmp_path / "f0.raw"), str(tmp_path / "f1.raw")]
    sc.frame_0.tofile(names[0])
    sc.frame_1.tofile(names[1])
    truth = str(tmp_path / "truth.flo")
    flow2d.write_flo(truth, sc.gt_u, sc.gt_v)

    def run(options, out):
        out.mkdir()
        r = subprocess.run([flow2d.CLI_PATH] + options + names + [str(w), str(h), "t_", str(out) + "/"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=300)
        return r, {f.name: f.read_bytes() for f in out.iterdir()}

    options = ["--refine", "4", "--refine-sigma", "20", "--refine-space", "3", "--refine-iterations", "2"]
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        p = flow.params(*CLI_PARAMS)
        forward = ("t_flow-u-96-64.raw", "t_flow-v-96-64.raw", "t_res.pgm", "t_amp-96-64.raw", "t_flow.flo")
        for backward in (["--backward"], []):
            tag = "b" if backward else "f"
            r0, plain = run(backward + ["--flo", "--ground-truth", truth], tmp_path / ("plain_" + tag))
            r1, refined = run(backward + ["--flo", "--ground-truth", truth] + options, tmp_path / ("refined_" + tag))
            assert r0.returncode == 0 and r1.returncode == 0, r1.stdout[-2000:]
            assert set(plain) == set(refined) and set(forward) <= set(plain)
            for f in plain:
                if f not in forward:
                    assert refined[f] == plain[f], f
            assert refined[forward[0]] != plain[forward[0]] and refined[forward[1]] != plain[forward[1]]
            ru, rv, rec, (pu, pv) = flow.refine_flow(sc.frame_0, sc.frame_1, p, 4, 20.0, 3.0, 2, bool(backward), flow=True)
            assert refined[forward[0]] == ru.tobytes() and refined[forward[1]] == rv.tobytes()
            assert plain[forward[0]] == pu.tobytes() and plain[forward[1]] == pv.tobytes()
            assert "Refinement: " not in r0.stdout and "before refinement" not in r0.stdout
            line = [q for q in r1.stdout.splitlines() if q.startswith("Refinement: ")]
            assert len(line) == 1, r1.stdout[-2000:]
            printed = json.loads(line[0][len("Refinement: "):])
            assert printed == dict(rec.summary(), radius=4, sigma=20.0, space=3.0, iterations=2)
            assert (rec.filled > 0) == bool(backward)
            scores = [q for q in r1.stdout.splitlines() if q.startswith("Flow error")]
            before = [q for q in r0.stdout.splitlines() if q.startswith("Flow error")]
            assert len(scores) == 2 and len(before) == 1 and scores[0].startswith("Flow error: ")
            assert scores[1] == before[0].replace("Flow error: ", "Flow error before refinement: ")
            assert scores[0] != before[0]
    finally:
        flow.close()
    for bad in (["--refine", "0"], ["--refine", "8"], ["--refine"], ["--refine", "x"], ["--refine", "3", "--refine-sigma", "-1"],
                ["--refine", "3", "--refine-space", "nan"], ["--refine", "3", "--refine-iterations", "0"],
                ["--refine", "3", "--refine-iterations", "17"]):
        q = subprocess.run([flow2d.CLI_PATH] + bad + names + [str(w), str(h), "t_"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert q.returncode == 5, (bad, q.stdout[-500:])
