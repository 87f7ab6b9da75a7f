"""Motion segmentation on the MI355X: flow2d_segment_motion_2d against the numpy restatement of its definition
(tests/test_segmentation_cpu.py), byte for byte -- labels, region table and summary are integers, there is no tolerance --, on
patterns that make every part of the definition bite, at shapes around the kernels' 64 x 16 tile; truncated tables; identical
bytes from repeated calls, a replayed graph and an instance alone or in a lock-step batch; the refusals on a real context;
OpticalFlow.segment_motion against the restatement applied to its own residual planes, and the CLI against the Python path."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from test_gpu_batch_kernels import Tall, pitch_of, stride_of
from test_gpu_denoise import CLI_PARAMS, run_cli, scenes_module
from test_oracle import rub_pair
from test_segmentation_cpu import (INF, PATTERNS, REGION_DTYPE, SMALL_SHAPES, SUMMARY_DTYPE, pattern_case, reference_of,
                                   segment_motion_reference, two_layer_case)

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Outputs:
    """Poisoned labels, table and summary of one call."""

    def __init__(self, ctx, w, h, max_regions, instances=1):
        self.ctx, self.w, self.h, self.max_regions = ctx, w, h, max_regions
        self.labels = ctx.plane(w, h).fill_bytes(0x7F)
        self.regions = ctx.region_records(max_regions, instances).fill_bytes(0x7F)
        self.summary = ctx.segment_summaries(instances).fill_bytes(0x7F)

    def read(self, instance=0):
        labels = self.labels.download(self.w, self.h).view(np.int32)
        words = self.max_regions * 16
        table = self.regions.download((instance + 1) * words, 1)[0, instance * words:] if words else np.zeros(0, F32)
        summary = self.summary.download((instance + 1) * 8, 1)[0, instance * 8:]
        return labels, table.tobytes(), summary.tobytes()

    def untouched(self):
        return all((q.download().view(np.uint32) == 0x7F7F7F7F).all() for q in (self.labels, self.regions, self.summary))


def upload(ctx, case, w, h):
    return (ctx.plane(w, h, case["ru"]), ctx.plane(w, h, case["rv"]), None if case["mask"] is None else ctx.plane(w, h, case["mask"]))


def run(ctx, planes, case, w, h, out):
    ctx.segment_motion(planes[0], planes[1], w, h, case["threshold"], case["join"], case["min_area"], planes[2], out.max_regions,
                       labels=out.labels, regions=out.regions, summary=out.summary)


def check(got, ref, what):
    labels, table, summary = got
    s, r = np.frombuffer(summary, SUMMARY_DTYPE)[0], ref["summary"][0]
    print("%s: regions %d / %d, foreground %d / %d, dropped %d / %d" %
          (what, s["region_count"], r["region_count"], s["foreground"], r["foreground"], s["dropped"], r["dropped"]))
    assert summary == ref["summary"].tobytes(), what
    wrong = labels != ref["labels"]
    assert not wrong.any(), "%s: %d of %d labels differ" % (what, wrong.sum(), wrong.size)
    if table != ref["regions"].tobytes():
        t = np.frombuffer(table, REGION_DTYPE)
        k = int(np.flatnonzero(t != ref["regions"])[0])
        raise AssertionError("%s: record %d is %s, not %s" % (what, k, t[k], ref["regions"][k]))


@pytest.mark.parametrize("w,h", SMALL_SHAPES)
def test_patterns_match_the_definition(flow2d, ctx, w, h):
    max_regions = 512 if w * h > 10000 else w * h
    for name in PATTERNS:
        case = pattern_case(name, w, h)
        out = Outputs(ctx, w, h, max_regions)
        run(ctx, upload(ctx, case, w, h), case, w, h, out)
        check(out.read(), reference_of(case, max_regions), "%dx%d %s" % (w, h, name))


def test_truncated_table_and_no_table(flow2d, ctx):
    w = h = 64
    case = pattern_case("checkerboard", w, h)
    planes = upload(ctx, case, w, h)
    out = Outputs(ctx, w, h, 100)
    run(ctx, planes, case, w, h, out)
    got, ref = out.read(), reference_of(case, 100)
    check(got, ref, "max_regions = 100")
    s = np.frombuffer(got[2], SUMMARY_DTYPE)[0]
    assert s["region_count"] == 2048 and s["recorded"] == 100 and got[0].max() == 2048 and len(got[1]) == 100 * 64
    # no table at all: regions = NULL
    out = Outputs(ctx, w, h, 0)
    assert flow2d.hip_lib().flow2d_segment_motion_2d(
        ctx.handle, planes[0].ptr, planes[1].ptr, None, w, h, planes[0].pitch, 0.5, INF, 1, out.labels.ptr, None, 0, out.summary.ptr,
        ctx._segment_buffers[1].ptr, ctx._segment_buffers[0]) == 0
    check(out.read(), reference_of(case, 0), "max_regions = 0")
    assert (out.regions.download().view(np.uint32) == 0x7F7F7F7F).all()
    # fewer regions than records: the rest of the table is zero
    two = pattern_case("rectangles_join", w, h)
    out = Outputs(ctx, w, h, 7)
    run(ctx, upload(ctx, two, w, h), two, w, h, out)
    check(out.read(), reference_of(two, 7), "two regions, seven records")


def test_full_hd_noise(flow2d, ctx):
    w, h = 1920, 1080
    case = pattern_case("noise", w, h)
    out = Outputs(ctx, w, h, 4096)
    run(ctx, upload(ctx, case, w, h), case, w, h, out)
    ref = reference_of(case, 4096)
    check(out.read(), ref, "1920x1080 noise")
    assert ref["summary"]["region_count"][0] > 4096 and ref["all_regions"]["area"].max() > 1000


def test_repeated_calls_and_a_replayed_graph_give_the_same_bytes(flow2d, ctx):
    w, h = 640, 480
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    case = pattern_case("noise", w, h)
    planes = upload(ctx, case, w, h)
    first, second, replay = (Outputs(ctx, w, h, 1000) for _ in range(3))
    run(ctx, planes, case, w, h, first)      # (also allocates the context's workspace)
    run(ctx, planes, case, w, h, second)
    eager = first.read()
    again = second.read()
    assert eager[0].tobytes() == again[0].tobytes() and eager[1:] == again[1:]
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    try:
        run(ctx, planes, case, w, h, replay)
    finally:
        graph = vp()
        assert lib.flow2d_capture_end(ctx.handle, ctypes.byref(graph)) == 0
    try:
        ctx.synchronize()
        assert replay.untouched()  # captured, not run
        for _ in range(2):
            for q in (replay.labels, replay.regions, replay.summary):
                q.fill_bytes(0x3C)
            assert lib.flow2d_graph_launch(ctx.handle, graph) == 0
            ctx.synchronize()
            got = replay.read()
            assert got[0].tobytes() == eager[0].tobytes() and got[1:] == eager[1:]
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)
    check(eager, reference_of(case, 1000), "640x480 noise")


@pytest.mark.parametrize("kind", ["contiguous", "rows", "bytes"])
def test_lock_step_batch(flow2d, ctx, kind):
    """Three instances `stride` apart: labels, table and summary of instance b are the bytes of the same planes segmented alone
    and those of the restatement, and every other word of the label allocation is what it was."""
    w, h, cw, ch, count, max_regions = 300, 70, 320, 80, 3, 64
    stride = stride_of(kind, pitch_of(cw), ch)
    names = ("noise", "bar", "spiral")
    cases = [pattern_case(name, w, h) for name in names]
    shared = dict(threshold=0.5, join=INF, min_area=2)
    mask = np.zeros((h, w), F32)
    fill = lambda arrays: Tall(ctx, cw, ch, count, stride).fill(arrays)  # noqa: E731
    tu, tv = fill([c["ru"] for c in cases]), fill([c["rv"] for c in cases])
    tm = fill([mask if c["mask"] is None else c["mask"] for c in cases])
    labels = Tall(ctx, cw, ch, count, stride)
    regions, summary = ctx.region_records(max_regions, count).fill_bytes(0x7F), ctx.segment_summaries(count).fill_bytes(0x7F)
    with ctx.set_batch(count, stride):
        ctx.segment_motion(tu, tv, w, h, mask=tm, max_regions=max_regions, instances=count, labels=labels, regions=regions,
                           summary=summary, **shared)
    ctx.synchronize()
    refs = [segment_motion_reference(c["ru"], c["rv"], mask=mask if c["mask"] is None else c["mask"], max_regions=max_regions,
                                     **shared) for c in cases]
    labels.check([r["labels"].view(F32) for r in refs], "labels (%s)" % kind)
    table = regions.download(count * max_regions * 16, 1).tobytes()
    sums = summary.download(count * 8, 1).tobytes()
    for b, (c, ref) in enumerate(zip(cases, refs)):
        assert table[b * max_regions * 64:(b + 1) * max_regions * 64] == ref["regions"].tobytes(), "table of instance %d" % b
        assert sums[b * 32:(b + 1) * 32] == ref["summary"].tobytes(), "summary of instance %d" % b
        alone = Outputs(ctx, w, h, max_regions)
        planes = (ctx.plane(w, h, c["ru"]), ctx.plane(w, h, c["rv"]), ctx.plane(w, h, mask if c["mask"] is None else c["mask"]))
        run(ctx, planes, dict(c, **shared), w, h, alone)
        check(alone.read(), ref, "instance %d alone" % b)
    assert len({r["summary"].tobytes() for r in refs}) == count
    for t in (tu, tv, tm):
        t.check(None, "an input")
    # a written range must not meet a later instance of an input
    lib = flow2d.hip_lib()
    ws = ctx._segment_buffers
    with ctx.set_batch(count, stride):
        assert lib.flow2d_segment_motion_2d(ctx.handle, tu.ptr, tv.ptr, None, w, h, tu.pitch, 0.5, INF, 1, tv.ptr + 2 * stride,
                                            regions.ptr, max_regions, summary.ptr, ws[1].ptr, ws[0]) == 1
        assert lib.flow2d_segment_motion_2d(ctx.handle, tu.ptr, tv.ptr, None, w, h, tu.pitch, 0.5, INF, 1, labels.ptr,
                                            regions.ptr, max_regions, regions.ptr + 2 * max_regions * 64, ws[1].ptr, ws[0]) == 1
        need = lib.flow2d_segment_motion_workspace_bytes(w, h, 1)
        assert lib.flow2d_segment_motion_2d(ctx.handle, tu.ptr, tv.ptr, None, w, h, tu.pitch, 0.5, INF, 1, labels.ptr,
                                            regions.ptr, max_regions, summary.ptr, ws[1].ptr, need) == 1  # one slice for three


def test_invalid_arguments_write_nothing(flow2d, ctx):
    w, h = 100, 40
    lib = flow2d.hip_lib()
    case = pattern_case("bar", w, h)
    pu, pv, pm = upload(ctx, case, w, h)
    out = Outputs(ctx, w, h, 16)
    need = lib.flow2d_segment_motion_workspace_bytes(w, h, 1)
    ws = ctx.plane(need // 4, 1).fill_bytes(0x7F)
    d = dict(ru=pu.ptr, rv=pv.ptr, mask=pm.ptr, w=w, h=h, pitch=pu.pitch, threshold=0.5, join=INF, min_area=1, labels=out.labels.ptr,
             regions=out.regions.ptr, max_regions=16, summary=out.summary.ptr, ws=ws.ptr, ws_bytes=need)

    def call(**kw):
        a = dict(d, **kw)
        return lib.flow2d_segment_motion_2d(ctx.handle, a["ru"], a["rv"], a["mask"], a["w"], a["h"], a["pitch"], a["threshold"],
                                            a["join"], a["min_area"], a["labels"], a["regions"], a["max_regions"], a["summary"],
                                            a["ws"], a["ws_bytes"])

    nan = float("nan")
    bad = [dict(ru=None), dict(rv=None), dict(labels=None), dict(summary=None), dict(ws=None), dict(regions=None), dict(w=0),
           dict(h=0), dict(pitch=pu.pitch + 8), dict(pitch=16), dict(threshold=-0.5), dict(threshold=nan), dict(join=-1.0),
           dict(join=nan), dict(min_area=0), dict(regions=out.regions.ptr + 4), dict(summary=out.summary.ptr + 4), dict(ws=ws.ptr + 8),
           dict(ws_bytes=need - 1), dict(labels=pu.ptr), dict(labels=pm.ptr + pu.pitch), dict(regions=pv.ptr), dict(summary=pu.ptr),
           dict(ws=pv.ptr), dict(ws=out.labels.ptr), dict(summary=out.regions.ptr + 64), dict(regions=ws.ptr),
           dict(summary=out.labels.ptr + 16)]
    for kw in bad:
        assert call(**kw) == 1, kw
    with ctx.set_batch(2, pu.pitch * h):
        assert call() == 1  # a workspace for one instance under a batch of two
    ctx.synchronize()
    assert out.untouched() and (ws.download().view(np.uint32) == 0x7F7F7F7F).all()
    assert call() == 0
    check(out.read(), reference_of(case, 16), "after the refusals")


# ---- the host layer ---------------------------------------------------------------------------------------------------------------
SMALL_FRAME_PARAMS = (50, 0.9, 40, 5, 5.0, 0.001, 0.001, 3, 0.8)  # see test_chain_on_two_layer


def region_bytes(regions):
    return b"".join(bytes(r) for r in regions)


def test_chain_on_two_layer(flow2d, ctx):
    """OpticalFlow.segment_motion on two_layer at 64 x 64 with the computed flow: exactly the restatement applied to the residual
    planes the call returns (with and without masks); and the scene's square -- one region with min_area = 16 and threshold 0.5,
    its box within 3 px of the true one (20, 24) - (35, 39).

    The scene assertion is made with masks and with solver parameters for a 64 x 64 frame, for two reasons that are the scene's
    and the solver's, not the labelling's.  Without masks the forward flow gives the background pixels the square covers in
    frame 1 the square's motion (they have no counterpart), so the region is the square of both frames together, 4.5 px wider
    than the true one: a box within 3 px is out of reach by construction, and the forward occlusion mask exists to leave those
    pixels out.  And the CLI's defaults (alpha 35, a median of radius 5 -- an 11 px window on a 16 px square --, a pre-blur of
    1.5 px) are those of 584 x 388 frames: at 64 x 64 that solver returns no motion at all on the square (|flow| 0.01 px, no
    foreground, 0 regions; the run of this test with those parameters printed "0 regions, 0 foreground").  SMALL_FRAME_PARAMS
    are alpha 5, median radius 3, pre-blur 0.8 px.  With the same flow through the CPU oracle and the restatements: with masks
    one region of 227 pixels, box (19, 22) - (34, 41), 9 pixels dropped; without masks one region of 414 pixels, box
    (19, 21) - (42, 41)."""
    sc, _ = two_layer_case(64, 64)
    h, w = sc.shape
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        p = flow.params(*SMALL_FRAME_PARAMS)
        for masks in (False, True):
            rec, summary, regions, labels, (ru, rv) = flow.segment_motion(sc.frame_0, sc.frame_1, p, flow2d.MOTION_AFFINE, 0.5, 5, 0.5,
                                                                          INF, 16, masks, residual=True)
            plain, (eu, ev) = flow.estimate_global_motion(sc.frame_0, sc.frame_1, p, flow2d.MOTION_AFFINE, 0.5, 5, masks, residual=True)
            assert bytes(plain) == bytes(rec) and eu.tobytes() == ru.tobytes() and ev.tobytes() == rv.tobytes()
            mask = None
            if masks:
                mask = flow.compute_flow_bidirectional(sc.frame_0, sc.frame_1, p)[4]
            ref = segment_motion_reference(ru, rv, 0.5, INF, 16, mask, flow2d.host_lib().flow2d_host_segment_max_regions())
            assert bytes(summary) == ref["summary"].tobytes()
            assert np.array_equal(labels, ref["labels"])
            assert region_bytes(regions) == ref["regions"][:summary.recorded].tobytes()
            print("masks %s: %d regions, %d foreground, %d dropped; boxes %s" %
                  (masks, summary.region_count, summary.foreground, summary.dropped, [r.bbox for r in regions]))
            if masks:
                assert summary.region_count == 1, [(r.area, r.bbox) for r in regions]
                assert max(abs(a - b) for a, b in zip(regions[0].bbox, (20, 24, 35, 39))) <= 3, regions[0].bbox
        f0, f1, dl = ctx.plane(w, h, sc.frame_0), ctx.plane(w, h, sc.frame_1), ctx.plane(w, h)
        dev = flow.segment_motion_device(f0.ptr, f1.ptr, p, flow2d.MOTION_AFFINE, 0.5, 5, 0.5, INF, 16, True, dev_labels=dl.ptr)
        assert bytes(dev[1]) == bytes(summary) and region_bytes(dev[2]) == region_bytes(regions)
        assert np.array_equal(dl.download(w, h).view(np.int32), labels)
        for bad in (dict(threshold=-1.0), dict(join=float("nan")), dict(min_area=0), dict(model=3)):
            with pytest.raises(flow2d.Flow2DError):
                flow.segment_motion(sc.frame_0, sc.frame_1, p, **bad)
    finally:
        flow.close()


def test_cli_segment_motion(flow2d, ctx, tmp_path):
    """--segment-motion prints the summary and the regions of OpticalFlow.segment_motion on the pair, writes the labels and leaves
    every other file as it was; without --global-motion it is a usage error."""
    w, h = 584, 388
    options = ["--global-motion", "affine", "--segment-motion", "0.75", "--segment-join", "1.5", "--segment-min-area", "25"]
    plain = run_cli(flow2d, ["--global-motion", "affine"], tmp_path / "plain")
    out_dir = tmp_path / "segment"
    out_dir.mkdir()
    data = os.path.join(ROOT, "tests", "data")
    tail = ["--u8", os.path.join(data, "rub1.raw"), os.path.join(data, "rub2.raw"), "584", "388", "t_", str(out_dir) + "/"]
    r = subprocess.run([flow2d.CLI_PATH] + options + tail, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    files = {f: (out_dir / f).read_bytes() for f in os.listdir(out_dir)}
    assert set(files) == set(plain) | {"t_labels-584-388.raw"}
    for f in plain:
        assert files[f] == plain[f], f
    r1, r2 = rub_pair()
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        rec, summary, regions, labels = flow.segment_motion(r1, r2, flow.params(*CLI_PARAMS), flow2d.MOTION_AFFINE, 0.5, 5, 0.75, 1.5, 25)
    finally:
        flow.close()
    assert files["t_labels-584-388.raw"] == labels.tobytes()
    line = [q for q in r.stdout.splitlines() if q.startswith("Motion segmentation: ")]
    assert len(line) == 1, r.stdout[-2000:]
    printed = json.loads(line[0][len("Motion segmentation: "):])
    assert printed == {"regions": summary.region_count, "foreground": summary.foreground, "dropped": summary.dropped,
                       "recorded": summary.recorded}
    rows = [json.loads(q.split(": ", 1)[1]) for q in r.stdout.splitlines() if q.startswith("Region ")]
    assert len(rows) == summary.recorded and summary.recorded >= 1
    for row, reg in zip(rows, regions):
        assert row["area"] == reg.area and tuple(row["bbox"]) == reg.bbox
        assert tuple(row["centroid"]) == reg.centroid and tuple(row["motion"]) == reg.mean_motion
    alone = subprocess.run([flow2d.CLI_PATH, "--segment-motion", "0.75"] + tail, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
    assert alone.returncode == 5 and "--global-motion" in alone.stdout
