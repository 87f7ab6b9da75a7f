"""Frame interpolation on the MI355X: flow2d_interpolate_2d bit for bit against the numpy restatement of its definition
(tests/test_interpolation_cpu.py) from 1x1 to 4096^2, a lock-step batch and a captured graph against direct calls, the analytic
scenes with their true flows and through OpticalFlow.interpolate_frames, that path against compute_flow_bidirectional followed
by Context.interpolate, and the CLI's --interpolate."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

from test_interpolation_cpu import interpolation_reference
from test_oracle import rub_pair

pytestmark = pytest.mark.gpu

F32 = np.float32
CLI_PARAMS = (50, 0.9, 40, 5, 35.0, 0.001, 0.001, 5, 1.5)  # the CLI's defaults (main.cpp)
BORDER = 8


def random_case(rng, w, h, edge_cases=True):
    """Frames in [0, 255]; a forward flow of a translation up to +-20 px plus noise, 10 % wild vectors; a backward flow near its
    inverse; with edge_cases NaNs, vectors far out of the frame (+-1e6, +-3e38) and masks in [-0.5, 1.5] with NaNs."""
    f0, f1 = (rng.uniform(0, 255, (h, w)).astype(F32) for _ in range(2))
    t = rng.uniform(-20, 20, 2)
    u = (t[0] + rng.normal(0, 0.5, (h, w))).astype(F32)
    v = (t[1] + rng.normal(0, 0.5, (h, w))).astype(F32)
    bu = (-t[0] + rng.normal(0, 0.5, (h, w))).astype(F32)
    bv = (-t[1] + rng.normal(0, 0.5, (h, w))).astype(F32)
    for a in (u, v, bu, bv):
        wild = rng.random((h, w)) < 0.1
        a[wild] = rng.uniform(-20, 20, wild.sum())
    o0 = (rng.random((h, w)) < 0.3).astype(F32)
    o1 = rng.uniform(-0.5, 1.5, (h, w)).astype(F32)
    if edge_cases:
        for a in (u, v, bu, bv):
            pick = rng.random((h, w))
            a[pick < 0.01] = np.nan
            a[(pick >= 0.01) & (pick < 0.02)] = 1e6
            a[(pick >= 0.02) & (pick < 0.025)] = -3e38
        o0[rng.random((h, w)) < 0.02] = np.nan
        o1[rng.random((h, w)) < 0.02] = np.nan
    return f0, f1, u, v, bu, bv, o0, o1


def device_interpolate(ctx, case, t, iterations, max_residual=0.5, masks=(True, True)):
    h, w = case[0].shape
    planes = [ctx.plane(w, h, a) for a in case[:6]]
    occ = [ctx.plane(w, h, a) if m else None for a, m in zip(case[6:], masks)]
    out = ctx.plane(w, h)
    out.fill_bytes(0x7F)
    ctx.interpolate(*planes, w, h, t, out, occ[0], occ[1], iterations, max_residual)
    ctx.synchronize()
    got = out.download()
    for p in planes + [q for q in occ if q] + [out]:
        p.free()
    return got


def want_of(case, t, iterations, max_residual=0.5, masks=(True, True)):
    o0 = case[6] if masks[0] else None
    o1 = case[7] if masks[1] else None
    return interpolation_reference(*case[:6], t, o0, o1, iterations, max_residual)


def assert_same(got, want, what):
    same = (got.view(np.uint32) == want.view(np.uint32))
    assert same.all(), "%s: %d of %d pixels differ" % (what, (~same).sum(), got.size)


@pytest.mark.parametrize("w,h", [(1, 1), (1, 9), (9, 1), (17, 5), (67, 33), (256, 256)])
def test_kernel_matches_the_definition(flow2d, ctx, w, h):
    case = random_case(np.random.default_rng(w * 10007 + h), w, h)
    for t in (0.0, 0.25, 0.5, 1.0):
        for k in (1, 2, 16):
            for masks in ((True, True), (False, False), (True, False), (False, True)):
                if w * h > 10000 and masks[0] != masks[1]:
                    continue
                assert_same(device_interpolate(ctx, case, t, k, masks=masks), want_of(case, t, k, masks=masks),
                            "%dx%d t=%g K=%d masks=%s" % (w, h, t, k, masks))
    if w * h >= 1000:  # the residual bound: 0 px and a large one
        for r in (0.0, 50.0):
            assert_same(device_interpolate(ctx, case, 0.5, 2, r), want_of(case, 0.5, 2, r), "r=%g" % r)


@pytest.mark.parametrize("w,h,t,k", [(1920, 1080, 0.25, 2), (4096, 4096, 0.5, 2)])
def test_kernel_large_frames(flow2d, ctx, w, h, t, k):
    case = random_case(np.random.default_rng(w + h), w, h)
    assert_same(device_interpolate(ctx, case, t, k), want_of(case, t, k), "%dx%d" % (w, h))


@pytest.mark.parametrize("k", [1, 2, 16])
def test_t0_and_t1_are_the_frames(flow2d, ctx, k):
    """Finite flows, no masks: t = 0 gives frame_0 and t = 1 frame_1 bit for bit.  A NaN flow makes that side's fixed point NaN
    (0 * NaN), so the side is invalid there and the output comes from the plain-blend fallback -- still the frame."""
    w, h = 123, 77
    rng = np.random.default_rng(k)
    case = random_case(rng, w, h, edge_cases=False)
    got0 = device_interpolate(ctx, case, 0.0, k, masks=(False, False))
    got1 = device_interpolate(ctx, case, 1.0, k, masks=(False, False))
    assert_same(got0, case[0], "t=0")
    assert_same(got1, case[1], "t=1")
    nan = list(case)
    nan[4] = case[4].copy()
    nan[4][rng.random((h, w)) < 0.05] = np.nan
    want, d = interpolation_reference(*nan[:6], 1.0, iterations=k, details=True)
    assert not d["ok1"][np.isnan(nan[4])].any()
    got = device_interpolate(ctx, nan, 1.0, k, masks=(False, False))
    assert_same(got, want, "NaN flow")
    assert_same(got, case[1], "NaN flow, fallback")


def test_lock_step_batch(flow2d, ctx):
    """Three instances one below the other in tall containers, flow2d_context_set_batch(3, stride): one launch covers all."""
    w, h, n = 203, 61, 3
    lib = flow2d.hip_lib()
    cases = [random_case(np.random.default_rng(40 + k), w, h) for k in range(n)]
    planes = [ctx.plane(w, n * h, np.vstack([c[i] for c in cases])) for i in range(8)]
    out = ctx.plane(w, n * h)
    out.fill_bytes(0x7F)
    stride = planes[0].pitch * h
    with ctx.set_batch(n, stride):
        ctx.interpolate(*planes[:6], w, h, 0.3, out, planes[6], planes[7], 2, 0.5)
        # the output must not meet a later instance of an input either
        assert lib.flow2d_interpolate_2d(ctx.handle, *[p.ptr for p in planes], w, h, planes[0].pitch, ctypes.c_float(0.3), 2,
                                         ctypes.c_float(0.5), planes[7].ptr + 2 * stride) == 1
    ctx.synchronize()
    got = out.download()
    for k, c in enumerate(cases):
        lone = device_interpolate(ctx, c, 0.3, 2)
        assert_same(got[k * h:(k + 1) * h], lone, "instance %d" % k)
        assert_same(lone, want_of(c, 0.3, 2), "instance %d vs the definition" % k)


def test_captured_graph_gives_the_same_frame(flow2d, ctx):
    w, h = 640, 480
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    case = random_case(np.random.default_rng(5), w, h)
    eager = device_interpolate(ctx, case, 0.6, 4)
    planes = [ctx.plane(w, h, a) for a in case]
    out = ctx.plane(w, h)
    out.fill_bytes(0)
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    rc = lib.flow2d_interpolate_2d(ctx.handle, *[p.ptr for p in planes], w, h, planes[0].pitch, ctypes.c_float(0.6), 4,
                                   ctypes.c_float(0.5), out.ptr)
    graph = vp()
    assert lib.flow2d_capture_end(ctx.handle, ctypes.byref(graph)) == 0 and rc == 0
    try:
        ctx.synchronize()
        assert not out.download().any()  # captured, not run
        for _ in range(2):
            out.fill_bytes(0x7F)
            assert lib.flow2d_graph_launch(ctx.handle, graph) == 0
            ctx.synchronize()
            assert_same(out.download(), eager, "graph replay")
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)


def scenes_module():
    return importlib.import_module("cuda-flow2d_amd.scenes")


def rms(a, b):
    e = (a.astype(np.float64) - b.astype(np.float64))[BORDER:-BORDER, BORDER:-BORDER]
    return float(np.sqrt((e * e).mean()))


def bad_pixels(a, b):
    return int((np.abs(a.astype(np.float64) - b)[BORDER:-BORDER, BORDER:-BORDER] > 5).sum())


def scene_case(s):
    return (s.frame_0, s.frame_1, s.gt_u, s.gt_v, s.gt_back_u, s.gt_back_v,
            np.zeros(s.shape, F32) if s.occlusion is None else s.occlusion,
            np.zeros(s.shape, F32) if s.occlusion_1 is None else s.occlusion_1)


@pytest.mark.parametrize("name", ["translation", "rotation", "zoom", "affine"])
def test_affine_scenes_with_true_flows(flow2d, ctx, name):
    """K = 2 with the true flows: within 0.2 grey levels RMS of the exact frame (8-px border left out), a third of the plain
    blend's error or less; K = 1 is clearly worse on rotation."""
    s = scenes_module().make_scene(name, 256, 256, seed=0)
    case = scene_case(s)
    for t in (0.25, 0.5):
        got = device_interpolate(ctx, case, t, 2)
        assert_same(got, want_of(case, t, 2), "%s t=%g" % (name, t))
        truth = s.frame_at_time(t)
        blend = (F32(1) - F32(t)) * s.frame_0 + F32(t) * s.frame_1
        assert rms(got, truth) < 0.2 and rms(got, truth) < rms(blend, truth) / 3, (name, t, rms(got, truth), rms(blend, truth))
        if name == "rotation":
            assert rms(device_interpolate(ctx, case, t, 1), truth) > 1.5 * rms(got, truth)


def test_two_layer_masks_help(flow2d, ctx):
    """t = 0.5, K = 4, true flows: the true masks of both frames cut the pixels off by more than 5 grey levels from ~390 to ~80
    (the rest are the square's sub-pixel edges)."""
    s = scenes_module().make_scene("two_layer", 256, 256, seed=0)
    case = scene_case(s)
    truth = s.frame_at_time(0.5)
    with_masks = device_interpolate(ctx, case, 0.5, 4)
    without = device_interpolate(ctx, case, 0.5, 4, masks=(False, False))
    assert_same(with_masks, want_of(case, 0.5, 4), "masks")
    assert_same(without, want_of(case, 0.5, 4, masks=(False, False)), "no masks")
    assert bad_pixels(with_masks, truth) <= 100 and bad_pixels(without, truth) >= 300, (bad_pixels(with_masks, truth),
                                                                                         bad_pixels(without, truth))


def test_interpolate_frames_is_bidirectional_then_interpolate(flow2d, ctx):
    """OpticalFlow.interpolate_frames (host images) gives the frames compute_flow_bidirectional's flows and masks give through
    Context.interpolate, with and without masks; the device form over a sequence of three frames gives the same per pair."""
    s = scenes_module().make_scene("two_layer", 192, 160, seed=1)
    h, w = s.shape
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        p = flow.params(*CLI_PARAMS)
        times = [0.25, 0.5, 0.75]
        frames, _ = flow.interpolate_frames(s.frame_0, s.frame_1, p, times, iterations=2, max_residual=0.5, masks=True)
        plain, _ = flow.interpolate_frames(s.frame_0, s.frame_1, p, times, iterations=3, max_residual=1.0, masks=False)
        u, v, bu, bv, o0, o1, _ = flow.compute_flow_bidirectional(s.frame_0, s.frame_1, p)
        case = (s.frame_0, s.frame_1, u, v, bu, bv, o0, o1)
        for j, t in enumerate(times):
            assert_same(frames[j], device_interpolate(ctx, case, t, 2), "masks t=%g" % t)
            assert_same(frames[j], want_of(case, t, 2), "masks t=%g vs the definition" % t)
            assert_same(plain[j], device_interpolate(ctx, case, t, 3, 1.0, masks=(False, False)), "no masks t=%g" % t)
        # a sequence of three frames on the device: pair k, time j at k * len(times) + j
        third = s.frame_at_time(0.5)
        seq = [ctx.plane(w, h, a) for a in (s.frame_0, s.frame_1, third)]
        outs = [ctx.plane(w, h) for _ in range(2 * len(times))]
        for o in outs:
            o.fill_bytes(0x7F)
        flow.interpolate_frames_device([q.ptr for q in seq], times, [o.ptr for o in outs], p)
        ctx.synchronize()
        pair1, _ = flow.interpolate_frames(s.frame_1, third, p, times)
        for j in range(len(times)):
            assert_same(outs[j].download(), frames[j], "device pair 0 t=%g" % times[j])
            assert_same(outs[len(times) + j].download(), pair1[j], "device pair 1 t=%g" % times[j])
        with pytest.raises(flow2d.Flow2DError):
            flow.interpolate_frames(s.frame_0, s.frame_1, p, [1.5])
        with pytest.raises(flow2d.Flow2DError):
            flow.interpolate_frames(s.frame_0, s.frame_1, p, [0.5], iterations=0)
    finally:
        flow.close()


@pytest.mark.parametrize("name", ["translation", "rotation", "zoom", "affine", "two_layer"])
def test_scenes_through_interpolate_frames(flow2d, ctx, name):
    """Computed flows and masks (the CLI's parameters): the middle frame beats the plain blend on every scene."""
    s = scenes_module().make_scene(name, 256, 256, seed=0)
    h, w = s.shape
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        frames, _ = flow.interpolate_frames(s.frame_0, s.frame_1, flow.params(*CLI_PARAMS), [0.5])
    finally:
        flow.close()
    truth = s.frame_at_time(0.5)
    blend = F32(0.5) * s.frame_0 + F32(0.5) * s.frame_1
    assert rms(frames[0], truth) < rms(blend, truth), (name, rms(frames[0], truth), rms(blend, truth))


def run_cli(flow2d, args, out_dir):
    out_dir.mkdir(exist_ok=True)
    data = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
    cmd = [flow2d.CLI_PATH] + args + ["--u8", os.path.join(data, "rub1.raw"), os.path.join(data, "rub2.raw"), "584", "388",
                                      "t_", str(out_dir) + "/"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:]
    return {f: (out_dir / f).read_bytes() for f in os.listdir(out_dir)}


def test_cli_interpolate(flow2d, tmp_path):
    w, h = 584, 388
    plain = run_cli(flow2d, [], tmp_path / "plain")
    interp = run_cli(flow2d, ["--interpolate", "4"], tmp_path / "interp")
    both = run_cli(flow2d, ["--interpolate", "4", "--backward"], tmp_path / "both")
    new = {"t_interp-%d-of-4-584-388.raw" % k for k in (1, 2, 3)}
    assert not new & set(plain)
    assert set(interp) == set(plain) | new            # no backward files without --backward
    for f in plain:
        assert interp[f] == plain[f], f               # the forward files are byte-identical
        assert both[f] == plain[f], f
    for f in new:
        assert both[f] == interp[f], f
    raw = lambda f: np.frombuffer(both[f], F32).reshape(h, w)  # noqa: E731
    r1, r2 = rub_pair()
    case = (r1, r2, raw("t_flow-u-584-388.raw"), raw("t_flow-v-584-388.raw"), raw("t_flow-u-backward-584-388.raw"),
            raw("t_flow-v-backward-584-388.raw"), raw("t_occlusion-584-388.raw"), raw("t_occlusion-backward-584-388.raw"))
    for k in (1, 2, 3):
        assert_same(raw("t_interp-%d-of-4-584-388.raw" % k), want_of(case, k / 4, 2), "interp %d" % k)
