"""flow2d_deformation_2d on the device against its numpy restatement (tests/test_deformation_cpu.py), bit for bit: all nine
planes and both measures without a mask, with a binary and with a soft one, in containers larger than the frame; subsets of the
planes; the record; the same bytes from repeated calls, a replayed graph and an instance alone or in a lock-step batch; the
refusals on a real context; OpticalFlow.analyse_deformation_device against its parts; the CLI."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from test_deformation_cpu import (F32, GREEN, PLANES, SMALL, STAT_NAMES, STATS_DTYPE, U32, bits, deformation_reference,
                                  masked_case)
from test_gpu_batch_kernels import Tall, pitch_of, stride_of
from test_gpu_denoise import CLI_PARAMS, run_cli, scenes_module
from test_oracle import rub_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = U32(0x7F7F7F7F)
# the smallest that cross a wave (64 columns), a workgroup's row block (16 rows) and 256 columns, with ragged edges
SHAPES = [(2, 2), (2, 9), (9, 2), (3, 3), (63, 5), (64, 4), (65, 17), (257, 33), (300, 37)]
MASKS = ("none", "binary", "soft")


def case_of(w, h, mode):
    u, v, mask = masked_case(w, h, soft=mode == "soft")
    return u, v, (None if mode == "none" else mask)


class Frame:
    """The inputs of a case in containers 5 columns wider and 3 rows taller than the frame, the padding NaN."""

    def __init__(self, ctx, w, h, u, v, mask):
        self.ctx, self.w, self.h, self.cw, self.ch = ctx, w, h, w + 5, h + 3

        def container(a):
            full = np.full((self.ch, self.cw), np.nan, F32)
            full[:h, :w] = a
            return ctx.plane(self.cw, self.ch, full)

        self.u, self.v = container(u), container(v)
        self.mask = None if mask is None else container(mask)

    def outputs(self, names=PLANES):
        return {name: self.ctx.plane(self.cw, self.ch).fill_bytes(0x7F) for name in names}

    def run(self, measure, planes, record=None):
        self.ctx.deformation(self.u, self.v, self.w, self.h, measure, mask=self.mask, planes=planes, stats=record)

    def check(self, planes, ref, what):
        for name, plane in planes.items():
            got = plane.download().view(U32)
            assert np.array_equal(got[:self.h, :self.w], bits(ref[name])), "%s: %s" % (what, name)
            assert (got[self.h:] == POISON).all() and (got[:, self.w:] == POISON).all(), "%s: %s beyond the frame" % (what, name)


def poisoned_record(ctx, instances=1):
    return ctx.deformation_records(instances).fill_bytes(0x7F)


def record_of(ctx, record, instances=1):
    return np.frombuffer(record.download(instances * 64, 1).tobytes(), STATS_DTYPE)


def check_record(got, ref, what):
    """Counts, min and max exact; the double sums within n * 2^-52 * sum|term| of the restatement's: the worst case of any two
    orders of n additions of exactly representable terms (each at most (n - 1) * 2^-53 * sum|term| from the true sum), with a
    factor two of slack.  Derived, not measured."""
    want = ref["stats"][0]
    n = int(want["valid"])
    assert got["valid"] == n and got["invalid"] == want["invalid"], what
    assert not got["reserved"].any(), what
    for name in STAT_NAMES:
        assert got[name]["min"] == want[name]["min"] and got[name]["max"] == want[name]["max"], (what, name)
        for field, total in (("sum", ref["abs_sum"][name]), ("sum_sq", ref["abs_sum_sq"][name])):
            bound = n * 2.0 ** -52 * total
            print("%s %s.%s: |difference| %.3g, bound %.3g" % (what, name, field, abs(got[name][field] - want[name][field]), bound))
            assert abs(got[name][field] - want[name][field]) <= bound, (what, name, field)


@pytest.mark.parametrize("mode", MASKS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_planes_and_record_match_the_definition(flow2d, ctx, w, h, mode):
    u, v, mask = case_of(w, h, mode)
    frame = Frame(ctx, w, h, u, v, mask)
    for measure in (SMALL, GREEN):
        planes, record = frame.outputs(), poisoned_record(ctx)
        frame.run(measure, planes, record)
        ref = deformation_reference(u, v, mask, measure)
        what = "%dx%d %s measure %d" % (w, h, mode, measure)
        frame.check(planes, ref, what)
        check_record(record_of(ctx, record)[0], ref, what)


def test_subsets_cost_no_other_plane(flow2d, ctx):
    """One plane, two of the tensor, three across the sets, and the record alone: the requested planes are the full run's, the
    others keep their poison, and the record is the same bytes whatever planes go with it."""
    w, h = 65, 17
    u, v, mask = case_of(w, h, "soft")
    frame = Frame(ctx, w, h, u, v, mask)
    ref = deformation_reference(u, v, mask, GREEN)
    full, full_record = frame.outputs(), poisoned_record(ctx)
    frame.run(GREEN, full, full_record)
    frame.check(full, ref, "all planes")
    want_record = record_of(ctx, full_record).tobytes()
    for names, with_record in ((("vorticity",), False), (("exx", "eyy"), False), (("divergence", "exy", "e2"), False),
                               (("max_shear",), False), (("dilatation",), True), ((), True)):
        planes, record = frame.outputs(), poisoned_record(ctx)
        frame.run(GREEN, {name: planes[name] for name in names}, record if with_record else None)
        frame.check({name: planes[name] for name in names}, ref, "subset %s" % (names,))
        for name in PLANES:
            if name not in names:
                assert (planes[name].download().view(U32) == POISON).all(), (names, name)
        got = record_of(ctx, record).tobytes()
        assert got == (want_record if with_record else bytes([0x7F]) * 256), names
    # the convenience form: planes by name, the record read back
    got, stats = ctx.deformation(frame.u, frame.v, w, h, GREEN, mask=frame.mask, planes=("e1", "vorticity"))
    assert set(got) == {"e1", "vorticity"} and bytes(stats) == want_record
    for name in got:
        assert np.array_equal(bits(got[name]), bits(ref[name])), name
    assert stats.summary()["valid"] == ref["stats"]["valid"][0]


def test_repeated_calls_and_a_replayed_graph_give_the_same_bytes(flow2d, ctx):
    w, h = 300, 37
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    u, v, mask = case_of(w, h, "soft")
    frame = Frame(ctx, w, h, u, v, mask)
    outs = [(frame.outputs(), poisoned_record(ctx)) for _ in range(3)]

    def snapshot(k):
        return [outs[k][0][name].download().tobytes() for name in PLANES] + [record_of(ctx, outs[k][1]).tobytes()]

    frame.run(GREEN, *outs[0])  # (also allocates the context's workspace)
    frame.run(GREEN, *outs[1])
    eager = snapshot(0)
    assert snapshot(1) == eager
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    try:
        frame.run(GREEN, *outs[2])
    finally:
        graph = vp()
        assert lib.flow2d_capture_end(ctx.handle, ctypes.byref(graph)) == 0
    try:
        ctx.synchronize()
        assert all(set(s) == {0x7F} for s in snapshot(2))  # captured, not run
        for _ in range(2):
            for q in list(outs[2][0].values()) + [outs[2][1]]:
                q.fill_bytes(0x3C)
            assert lib.flow2d_graph_launch(ctx.handle, graph) == 0
            ctx.synchronize()
            got = snapshot(2)
            # (the words beyond the frame hold the other poison now: compare the frame and the record)
            for name, a, b in zip(PLANES, got, eager):
                a, b = (np.frombuffer(q, U32).reshape(frame.ch, frame.cw)[:h, :w] for q in (a, b))
                assert np.array_equal(a, b), name
            assert got[-1] == eager[-1]
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)
    frame.check(outs[0][0], deformation_reference(u, v, mask, GREEN), "300x37")


@pytest.mark.parametrize("kind", ["contiguous", "rows", "bytes"])
def test_lock_step_batch(flow2d, ctx, kind):
    """Three instances `stride` apart: planes and record of instance b are the bytes of the same input analysed alone and the
    restatement's planes, and every other word of the output allocations is what it was."""
    w, h, cw, ch, count = 257, 33, 300, 40, 3
    stride = stride_of(kind, pitch_of(cw), ch)
    cases = [masked_case(w, h, seed=20 + b, soft=b != 1) for b in range(count)]
    fill = lambda arrays: Tall(ctx, cw, ch, count, stride).fill(arrays)  # noqa: E731
    tu, tv, tm = (fill([c[k] for c in cases]) for k in range(3))
    outs = {name: Tall(ctx, cw, ch, count, stride) for name in PLANES}
    records = poisoned_record(ctx, count)
    with ctx.set_batch(count, stride):
        ctx.deformation(tu, tv, w, h, GREEN, mask=tm, planes=outs, stats=records, instances=count)
    ctx.synchronize()
    refs = [deformation_reference(*c, GREEN) for c in cases]
    for name in PLANES:
        outs[name].check([r[name] for r in refs], "%s (%s)" % (name, kind))
    got = record_of(ctx, records, count)
    for b, (c, ref) in enumerate(zip(cases, refs)):
        planes = {name: ctx.plane(cw, ch).fill_bytes(0x7F) for name in PLANES}
        record = poisoned_record(ctx)
        ctx.deformation(ctx.plane(cw, ch, c[0]), ctx.plane(cw, ch, c[1]), w, h, GREEN, mask=ctx.plane(cw, ch, c[2]), planes=planes,
                        stats=record)
        assert record_of(ctx, record).tobytes() == got[b:b + 1].tobytes(), "record of instance %d" % b
        for name in PLANES:
            assert np.array_equal(planes[name].download(w, h).view(U32), bits(ref[name])), (b, name)
        check_record(got[b], ref, "instance %d" % b)
    assert len({got[b:b + 1].tobytes() for b in range(count)}) == count
    for t in (tu, tv, tm):
        t.check(None, "an input")
    # a written range must not meet a later instance of an input or of another output, and one slice is no workspace for three
    lib = flow2d.hip_lib()
    need, ws = ctx._deformation_workspace

    def call(planes, record=records.ptr, ws_bytes=need):
        out = flow2d.DeformationPlanes(**planes)
        return lib.flow2d_deformation_2d(ctx.handle, tu.ptr, tv.ptr, tm.ptr, w, h, tu.pitch, GREEN, ctypes.byref(out), record, ws.ptr,
                                         ws_bytes)

    with ctx.set_batch(count, stride):
        assert call({"e1": tv.ptr + 2 * stride}) == 1
        assert call({"e1": outs["e1"].ptr, "e2": outs["e1"].ptr + stride}) == 1
        assert call({"e1": outs["e1"].ptr}, record=ws.ptr + need - 256) == 1
        assert call({"e1": outs["e1"].ptr}, ws_bytes=lib.flow2d_deformation_workspace_bytes(w, h, 1)) == 1
    ctx.synchronize()


def test_invalid_arguments_write_nothing(flow2d, ctx):
    w, h = 100, 40
    lib = flow2d.hip_lib()
    u, v, mask = case_of(w, h, "binary")
    pu, pv, pm = (ctx.plane(w, h, a) for a in (u, v, mask))
    outs = {name: ctx.plane(w, h).fill_bytes(0x7F) for name in PLANES}
    record = poisoned_record(ctx)
    need = lib.flow2d_deformation_workspace_bytes(w, h, 1)
    ws = ctx.plane(need // 4, 1).fill_bytes(0x7F)
    span = pu.pitch * h
    d = dict(u=pu.ptr, v=pv.ptr, mask=pm.ptr, w=w, h=h, pitch=pu.pitch, measure=SMALL, stats=record.ptr, ws=ws.ptr, ws_bytes=need,
             planes={name: q.ptr for name, q in outs.items()}, out=True)

    def call(**kw):
        a = dict(d, **kw)
        out = flow2d.DeformationPlanes(**a["planes"])
        return lib.flow2d_deformation_2d(ctx.handle, a["u"], a["v"], a["mask"], a["w"], a["h"], a["pitch"], a["measure"],
                                         ctypes.byref(out) if a["out"] else None, a["stats"], a["ws"], a["ws_bytes"])

    e1 = outs["e1"].ptr
    bad = [dict(u=None), dict(v=None), dict(out=False, stats=None), dict(planes={}, stats=None), dict(w=1), dict(h=1), dict(w=0),
           dict(pitch=pu.pitch + 8), dict(pitch=16), dict(measure=2), dict(measure=-1), dict(stats=record.ptr + 4),
           dict(ws=ws.ptr + 8), dict(ws=None), dict(ws_bytes=need - 1),
           dict(planes={"divergence": pu.ptr}), dict(planes={"max_shear": pv.ptr + pu.pitch}), dict(planes={"exx": pm.ptr}),
           dict(planes={"exx": e1, "exy": e1}), dict(planes={"e1": e1, "e2": e1 + span - pu.pitch}), dict(stats=pu.ptr + 64),
           dict(stats=e1), dict(ws=pv.ptr), dict(ws=outs["exy"].ptr), dict(stats=ws.ptr + 16), dict(stats=ws.ptr + need - 8)]
    for kw in bad:
        assert call(**kw) == 1, kw
    with ctx.set_batch(2, span):
        assert call() == 1  # a workspace for one instance under a batch of two
    ctx.synchronize()
    for name, q in outs.items():
        assert (q.download().view(U32) == POISON).all(), name
    assert set(record.download(64, 1).tobytes()) == {0x7F} and (ws.download().view(U32) == POISON).all()
    # without statistics the workspace takes no part, whatever it is
    assert call(stats=None, ws=None, ws_bytes=0, planes={"vorticity": outs["vorticity"].ptr}) == 0
    assert call(stats=None, ws=pv.ptr, ws_bytes=0, planes={"exx": outs["exx"].ptr}) == 0
    ctx.synchronize()
    assert set(record.download(64, 1).tobytes()) == {0x7F} and (ws.download().view(U32) == POISON).all()
    assert call() == 0
    ref = deformation_reference(u, v, mask, SMALL)
    for name, q in outs.items():
        assert np.array_equal(q.download().view(U32), bits(ref[name])), name
    check_record(record_of(ctx, record)[0], ref, "after the refusals")


def test_full_hd(flow2d, ctx):
    w, h = 1920, 1080
    u, v, mask = case_of(w, h, "soft")
    frame = Frame(ctx, w, h, u, v, mask)
    planes, record = frame.outputs(), poisoned_record(ctx)
    frame.run(GREEN, planes, record)
    ref = deformation_reference(u, v, mask, GREEN)
    frame.check(planes, ref, "1920x1080")
    check_record(record_of(ctx, record)[0], ref, "1920x1080")


# ---- the host layer ---------------------------------------------------------------------------------------------------------------
SMALL_FRAME_PARAMS = (50, 0.9, 40, 5, 5.0, 0.001, 0.001, 3, 0.8)  # a 64 x 64 frame: test_gpu_segmentation.py


def test_chain_equals_its_parts(flow2d, ctx):
    """OpticalFlow.analyse_deformation_device on `zoom` at 64 x 64 is flow -> blur -> entry run by hand, byte for byte, with and
    without masks and smoothing.  On the scene's ground-truth flow, u = 0.03 (x - c) rounded to fp32 (at most 2^-24 * max|flow|
    off, delta), every difference is within 2 delta + 2^-24 * 0.03 of 0.03 (the subtraction is exact or rounds a number near
    0.03), and the divergence, their sum, within twice that plus 2^-24 * 0.06."""
    sc = scenes_module().make_scene("zoom", 64, 64, seed=0)
    h, w = sc.frame_0.shape
    f0, f1 = ctx.plane(w, h, sc.frame_0), ctx.plane(w, h, sc.frame_1)
    new = lambda: ctx.plane(w, h).fill_bytes(0x7F)  # noqa: E731
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        p = flow.params(*SMALL_FRAME_PARAMS)
        for masks, sigma, measure in ((False, 0.0, SMALL), (False, 1.5, GREEN), (True, 1.0, GREEN), (True, 0.0, SMALL)):
            outs = {name: new() for name in PLANES}
            fu, fv, fm = new(), new(), new()
            stats = flow.analyse_deformation_device(f0.ptr, f1.ptr, p, measure, sigma, masks, {n: q.ptr for n, q in outs.items()},
                                                    dev_flow=(fu.ptr, fv.ptr), dev_mask=fm.ptr if masks else None)
            # by hand
            u, v, bu, bv, of, ob = (new() for _ in range(6))
            if masks:
                flow.compute_flow_bidirectional_device([f0.ptr, f1.ptr], [u.ptr], [v.ptr], [bu.ptr], [bv.ptr], p, [of.ptr], [ob.ptr])
            else:
                flow.compute_flow_device(f0.ptr, f1.ptr, u.ptr, v.ptr, p)
            ctx.synchronize()
            if sigma > 0:
                taps, radius = flow2d.gaussian_kernel(sigma)
                su, sv = new(), new()
                ctx.gaussian_blur(su, u, w, h, taps, radius)
                ctx.gaussian_blur(sv, v, w, h, taps, radius)
                u, v = su, sv
            hand = {name: new() for name in PLANES}
            record = poisoned_record(ctx)
            ctx.deformation(u, v, w, h, measure, mask=of if masks else None, planes=hand, stats=record)
            what = "masks %s sigma %g" % (masks, sigma)
            assert bytes(stats) == record_of(ctx, record).tobytes(), what
            assert fu.download().tobytes() == u.download().tobytes() and fv.download().tobytes() == v.download().tobytes(), what
            if masks:
                assert fm.download().tobytes() == of.download().tobytes(), what
            for name in PLANES:
                assert outs[name].download().tobytes() == hand[name].download().tobytes(), (what, name)
            print(what, json.dumps(stats.summary()["divergence"]))
        # the host-image form returns the same planes and record
        planes, host_stats = flow.analyse_deformation(sc.frame_0, sc.frame_1, p, SMALL, 0.0, True, planes=("divergence", "e1"))
        assert bytes(host_stats) == bytes(stats)
        for name in planes:
            assert planes[name].tobytes() == outs[name].download().tobytes(), name
        for bad in (dict(measure=2), dict(smoothing_sigma=-1.0), dict(smoothing_sigma=float("nan")), dict(smoothing_sigma=9.0)):
            with pytest.raises(flow2d.Flow2DError):
                flow.analyse_deformation(sc.frame_0, sc.frame_1, p, **bad)
    finally:
        flow.close()
    got, stats = ctx.deformation(ctx.plane(w, h, sc.gt_u), ctx.plane(w, h, sc.gt_v), w, h, SMALL, planes=("divergence",))
    unit = 2.0 ** -24
    delta = unit * float(max(np.abs(sc.gt_u).max(), np.abs(sc.gt_v).max()))
    bound = 2 * (2 * delta + unit * 0.03) + unit * 0.06
    assert bound < 3e-7
    error = np.abs(got["divergence"].astype(np.float64) - 0.06).max()
    print("divergence of zoom's true flow: max error %.3g, bound %.3g" % (error, bound))
    assert stats.valid == w * h and error <= bound


def test_cli_deformation(flow2d, ctx, tmp_path):
    """--deformation writes the nine planes of OpticalFlow.analyse_deformation on the pair, prints its record and leaves every
    other file as it was; a bad --strain or --deformation-sigma is a usage error."""
    w, h = 584, 388
    plain = run_cli(flow2d, ["--backward"], tmp_path / "plain")
    options = ["--backward", "--deformation", "--strain", "green", "--deformation-sigma", "2"]
    out_dir = tmp_path / "deformation"
    out_dir.mkdir()
    data = os.path.join(ROOT, "tests", "data")
    tail = ["--u8", os.path.join(data, "rub1.raw"), os.path.join(data, "rub2.raw"), "584", "388", "t_", str(out_dir) + "/"]
    r = subprocess.run([flow2d.CLI_PATH] + options + tail, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    files = {f: (out_dir / f).read_bytes() for f in os.listdir(out_dir)}
    names = {name: "t_%s-584-388.raw" % name.replace("_", "-") for name in PLANES}
    assert set(files) == set(plain) | set(names.values())
    for f in plain:
        assert files[f] == plain[f], f
    r1, r2 = rub_pair()
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        planes, stats = flow.analyse_deformation(r1, r2, flow.params(*CLI_PARAMS), GREEN, 2.0, True)
    finally:
        flow.close()
    for name in PLANES:
        assert files[names[name]] == planes[name].tobytes(), name
    line = [q for q in r.stdout.splitlines() if q.startswith("Deformation: ")]
    assert len(line) == 1, r.stdout[-2000:]
    printed = json.loads(line[0][len("Deformation: "):])
    want = stats.summary()
    assert printed["measure"] == "green" and printed["sigma"] == 2.0
    assert printed["valid"] == want["valid"] > 0 and printed["invalid"] == want["invalid"]
    for name in STAT_NAMES:
        assert printed[name]["mean"] == want[name]["mean"] and printed[name]["rms"] == want[name]["rms"], name
        assert F32(printed[name]["min"]) == F32(want[name]["min"]) and F32(printed[name]["max"]) == F32(want[name]["max"]), name
    for bad in (["--strain", "large"], ["--strain"], ["--deformation-sigma", "-1"], ["--deformation-sigma", "9"],
                ["--deformation-sigma", "x"]):
        q = subprocess.run([flow2d.CLI_PATH, "--deformation"] + bad + tail[:-2], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert q.returncode == 5, (bad, q.stdout[-500:])
