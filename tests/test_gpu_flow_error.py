"""Flow error against ground truth on the MI355X: flow2d_flow_error_2d against the numpy restatement of its definition (the EPE
plane bit for bit, the AE plane within 1e-4 degrees, exact counts, sums to relative 1e-9), determinism (repeated calls, a
lock-step group against lone calls, a captured graph), the analytic scenes through OpticalFlow.compute_flow, and the CLI's
--ground-truth and --flo."""
import ctypes
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

from test_flow_error_cpu import flow_error_reference

pytestmark = pytest.mark.gpu

F32 = np.float32
FILL = np.frombuffer(b"\x7f\x7f\x7f\x7f", F32)[0]
# EPE over all pixels of each scene at 256 x 256, seed 0, Grey, the CLI's defaults: 1.5 x what the CPU oracle's table measured
# (tools/accuracy_table.py --oracle, profiles/accuracy/oracle_256.txt); the product is bit-identical to the oracle for Grey.
SCENE_EPE_LIMIT = {"translation": 1.5 * 0.8220, "rotation": 1.5 * 0.1466, "zoom": 1.5 * 0.1276, "affine": 1.5 * 0.1330,
                   "two_layer": 1.5 * 0.2409}
CLI_PARAMS = (50, 0.9, 40, 5, 35.0, 0.001, 0.001, 5, 1.5)


def random_case(rng, w, h, with_mask):
    """Ground truth up to +-40 px, estimates near it (some far off); NaN / inf / unknown-flow sentinels in the ground truth,
    NaN / inf estimates, a few exact estimates; an occlusion mask with 0 / 1 / NaN values."""
    gu = rng.uniform(-40, 40, (h, w)).astype(F32)
    gv = rng.uniform(-40, 40, (h, w)).astype(F32)
    u = (gu + rng.normal(0, 1.5, (h, w))).astype(F32)
    v = (gv + rng.normal(0, 1.5, (h, w))).astype(F32)
    far = rng.random((h, w)) < 0.05
    u[far] = rng.uniform(-500, 500, far.sum())
    pick = rng.random((h, w))
    gu[pick < 0.01] = np.nan
    gv[(pick >= 0.01) & (pick < 0.02)] = np.inf
    gu[(pick >= 0.02) & (pick < 0.03)] = 1e10  # Middlebury's unknown flow
    gv[(pick >= 0.03) & (pick < 0.035)] = -1e9  # the last valid value
    u[(pick >= 0.04) & (pick < 0.05)] = np.nan
    v[(pick >= 0.05) & (pick < 0.06)] = -np.inf
    exact = (pick >= 0.06) & (pick < 0.08)
    u[exact], v[exact] = gu[exact], gv[exact]
    occ = None
    if with_mask:
        occ = (rng.random((h, w)) < 0.2).astype(F32)
        occ[rng.random((h, w)) < 0.01] = np.nan
    return u, v, gu, gv, occ


def upload(ctx, arrays, container_w):
    """Planes in containers wider than the image: the columns beyond it must stay untouched."""
    out = []
    for a in arrays:
        if a is None:
            out.append(None)
            continue
        p = ctx.plane(container_w, a.shape[0])
        p.fill_bytes(0x7F)
        p.upload(a)
        out.append(p)
    return out


def check_record(got, want, dev_ae, sel_of, rel=1e-9):
    """Counts exactly; sum_epe, sum_epe_sq and max_epe against the restatement; sum_ae against the device's own AE plane
    summed in float64 (relative 1e-9) and against the exact angles (1e-4 degrees a pixel)."""
    assert got["invalid_ground_truth"] == want["invalid_ground_truth"]
    assert got["nonfinite_estimate"] == want["nonfinite_estimate"]
    for name in ("all", "noc", "occ"):
        g, r = got[name], want[name]
        for key in ("count", "above", "fl", "max_epe"):
            assert g[key] == r[key], (name, key, g[key], r[key])
        for key in ("sum_epe", "sum_epe_sq"):
            assert g[key] == pytest.approx(r[key], rel=rel, abs=1e-300), (name, key)
        sel = sel_of[name]
        assert g["sum_ae"] == pytest.approx(float(dev_ae[sel].astype(np.float64).sum()), rel=rel, abs=1e-300), name
        assert abs(g["sum_ae"] - r["sum_ae"]) <= 1e-4 * max(1, r["count"]), name


def run_device(ctx, u, v, gu, gv, occ, container_w=None):
    h, w = u.shape
    cw = container_w or w
    planes = upload(ctx, [u, v, gu, gv, occ], cw)
    epe, ae = upload(ctx, [np.zeros_like(u), np.zeros_like(u)], cw)
    epe.fill_bytes(0x7F)
    ae.fill_bytes(0x7F)
    rec = ctx.flow_error(*planes[:4], w, h, occlusion=planes[4], epe=epe, ae=ae)[0]
    e, a = epe.download(), ae.download()
    for p in planes + [epe, ae]:
        if p is not None:
            p.free()
            ctx._planes.remove(p)
    return rec, e, a


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("w,h", [(1, 1), (37, 5), (1920, 1080), (4096, 4096)])
def test_kernel_matches_the_definition(flow2d, ctx, w, h, with_mask):
    rng = np.random.default_rng(w * 7919 + h * 31 + with_mask)
    u, v, gu, gv, occ = random_case(rng, w, h, with_mask)
    if w * h == 1:
        u[:], v[:], gu[:], gv[:] = 3, 4, 0, 0  # the 3-4-5 error
        if occ is not None:
            occ[:] = 1
    cw = w + 3  # a level inside a wider container
    rec, e, a = run_device(ctx, u, v, gu, gv, occ, cw)
    want, we, wa = flow_error_reference(u, v, gu, gv, occ)
    assert np.array_equal(e[:, :w], we, equal_nan=True), "%d EPE pixels differ" % (~((e[:, :w] == we) | (np.isnan(e[:, :w]) & np.isnan(we)))).sum()
    assert np.array_equal(np.isnan(a[:, :w]), np.isnan(wa))
    ok = ~np.isnan(wa)
    assert np.abs(a[:, :w][ok] - wa[ok]).max(initial=0) <= 1e-4
    assert (e[:, w:].view(np.uint32) == 0x7F7F7F7F).all() and (a[:, w:].view(np.uint32) == 0x7F7F7F7F).all()
    take = ~np.isnan(we)
    occluded = np.zeros_like(take) if occ is None else occ != 0
    check_record(rec, want, a[:, :w], {"all": take, "noc": take & ~occluded, "occ": take & occluded})
    if w * h == 1:
        assert rec["all"]["sum_epe"] == 5 and rec[("occ" if with_mask else "noc")]["count"] == 1
    else:
        assert rec["invalid_ground_truth"] > 0 and rec["nonfinite_estimate"] > 0 and 0 < rec["all"]["above"][3] < rec["all"]["count"]
        if with_mask:
            assert rec["occ"]["count"] > 0 and rec["noc"]["count"] > 0


def test_infinite_epe_and_empty_classes(flow2d, ctx):
    """A finite estimate whose du * du overflows: its EPE is inf and so are the sums; a class without pixels reports zeros."""
    u = np.zeros((3, 37), F32)
    u[1, 5] = 1e30
    z = np.zeros_like(u)
    rec, e, _ = run_device(ctx, u, z, z, z, None)
    assert np.isinf(e[1, 5]) and rec["all"]["sum_epe"] == np.inf and rec["all"]["sum_epe_sq"] == np.inf
    assert rec["all"]["max_epe"] == np.inf and rec["all"]["above"] == [1, 1, 1, 1] and rec["all"]["count"] == u.size
    assert rec["occ"] == {"count": 0, "above": [0] * 4, "fl": 0, "sum_epe": 0.0, "sum_epe_sq": 0.0, "sum_ae": 0.0, "max_epe": 0.0}
    assert rec["noc"] == rec["all"]


def test_repeated_calls_are_bit_identical(flow2d, ctx):
    w, h = 1920, 1080
    u, v, gu, gv, occ = random_case(np.random.default_rng(11), w, h, True)
    planes = upload(ctx, [u, v, gu, gv, occ], w)
    epe, ae = ctx.plane(w, h), ctx.plane(w, h)
    first = ctx.flow_error(*planes[:4], w, h, occlusion=planes[4], epe=epe, ae=ae)
    e1, a1 = epe.download(), ae.download()
    epe.fill_bytes(0)
    ae.fill_bytes(0)
    second = ctx.flow_error(*planes[:4], w, h, occlusion=planes[4], epe=epe, ae=ae)
    assert first == second
    assert epe.download().tobytes() == e1.tobytes() and ae.download().tobytes() == a1.tobytes()
    # the record does not depend on whether the per-pixel planes are written
    assert ctx.flow_error(*planes[:4], w, h, occlusion=planes[4]) == first


def test_lock_step_group_equals_lone_calls(flow2d, ctx):
    """Three pairs one below the other in tall containers, flow2d_context_set_batch(3, stride): one launch pair covers all and
    instance b's record and planes are bit-identical to pair b's lone call."""
    w, h, n = 1021, 203, 3
    lib = flow2d.hip_lib()
    cases = [random_case(np.random.default_rng(40 + k), w, h, True) for k in range(n)]
    planes = [ctx.plane(w, n * h, np.vstack([c[i] for c in cases])) for i in range(5)]
    epe, ae = ctx.plane(w, n * h), ctx.plane(w, n * h)
    stride = planes[0].pitch * h
    with ctx.set_batch(n, stride):
        group = ctx.flow_error(*planes[:4], w, h, occlusion=planes[4], epe=epe, ae=ae, instances=n)
        # the outputs must not meet another instance of an input either: an epe plane inside u's second instance is refused
        ws = ctx._flow_error_buffers
        assert lib.flow2d_flow_error_2d(ctx.handle, planes[0].ptr, planes[1].ptr, planes[2].ptr, planes[3].ptr, None, w, h,
                                        planes[0].pitch, planes[0].ptr + stride, None, ws[3].ptr, ws[2].ptr, ws[0]) == 1
    ge, ga = epe.download(), ae.download()
    assert len(group) == n
    for k, c in enumerate(cases):
        lone, le, la = run_device(ctx, *c)
        assert group[k] == lone, k
        assert ge[k * h:(k + 1) * h].tobytes() == le.tobytes() and ga[k * h:(k + 1) * h].tobytes() == la.tobytes(), k


def test_captured_graph_gives_the_same_record(flow2d, ctx):
    w, h = 640, 480
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    u, v, gu, gv, occ = random_case(np.random.default_rng(5), w, h, True)
    planes = upload(ctx, [u, v, gu, gv, occ], w)
    eager = ctx.flow_error(*planes[:4], w, h, occlusion=planes[4])[0]
    need = lib.flow2d_flow_error_workspace_bytes(w, h, 1)
    ws, stats = ctx.plane(need // 4, 1), ctx.plane(64, 1)
    stats.fill_bytes(0)
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    rc = lib.flow2d_flow_error_2d(ctx.handle, *[p.ptr for p in planes], w, h, planes[0].pitch, None, None, stats.ptr, ws.ptr, need)
    graph = vp()
    assert lib.flow2d_capture_end(ctx.handle, ctypes.byref(graph)) == 0 and rc == 0
    try:
        ctx.synchronize()
        assert not stats.download().any()  # captured, not run
        for _ in range(2):
            stats.fill_bytes(0)
            assert lib.flow2d_graph_launch(ctx.handle, graph) == 0
            ctx.synchronize()
            rec = (flow2d.FlowErrorStats * 1).from_buffer_copy(stats.download().tobytes())[0]
            assert flow2d._stats_dict(rec) == eager
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)


@pytest.mark.parametrize("name", ["translation", "rotation", "zoom", "affine", "two_layer"])
def test_scene_accuracy(flow2d, ctx, name):
    """OpticalFlow.compute_flow on an analytic scene, then Context.flow_error on the device planes: the same record as
    evaluate_flow on the downloaded flow, the counts of the restatement, and an EPE under the scene's limit."""
    scenes = importlib.import_module("cuda-flow2d_amd.scenes")
    s = scenes.make_scene(name, 256, 256, seed=0)
    h, w = s.shape
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    planes = [ctx.plane(w, h, a) for a in (s.frame_0, s.frame_1)] + [ctx.plane(w, h), ctx.plane(w, h)]
    try:
        flow.compute_flow_device(*[p.ptr for p in planes], flow.params(*CLI_PARAMS))
    finally:
        flow.close()
    gt = [ctx.plane(w, h, a) for a in (s.gt_u, s.gt_v)]
    occ = ctx.plane(w, h, s.occlusion) if s.occlusion is not None else None
    rec = ctx.flow_error(planes[2], planes[3], gt[0], gt[1], w, h, occlusion=occ)[0]
    u, v = planes[2].download(), planes[3].download()
    assert flow2d.evaluate_flow(u, v, s.gt_u, s.gt_v, occlusion=s.occlusion) == rec
    want, _, _ = flow_error_reference(u, v, s.gt_u, s.gt_v, s.occlusion)
    for cls in ("all", "noc", "occ"):
        assert rec[cls]["count"] == want[cls]["count"] and rec[cls]["above"] == want[cls]["above"]
        assert rec[cls]["sum_epe"] == pytest.approx(want[cls]["sum_epe"], rel=1e-9)
    epe = flow2d.flow_error_metrics(rec)["all"]["epe"]
    assert epe < SCENE_EPE_LIMIT[name], (name, epe)
    if s.occlusion is not None:
        assert rec["occ"]["count"] == int((s.occlusion != 0).sum()) > 0


def run_cli(flow2d, args, out_dir, files, w, h):
    out_dir.mkdir(exist_ok=True)
    cmd = [flow2d.CLI_PATH] + args + [str(files[0]), str(files[1]), str(w), str(h), "t_", str(out_dir) + "/"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    return p.returncode, p.stdout, {f: (out_dir / f).read_bytes() for f in os.listdir(out_dir)}


def printed_metrics(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("Flow error: ")]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0][len("Flow error: "):])


def test_cli_ground_truth_and_flo(flow2d, tmp_path):
    scenes = importlib.import_module("cuda-flow2d_amd.scenes")
    w, h = 256, 192
    s = scenes.make_scene("two_layer", w, h, seed=2)
    frames = [tmp_path / "f0.raw", tmp_path / "f1.raw"]
    for f, a in zip(frames, (s.frame_0, s.frame_1)):
        f.write_bytes(a.tobytes())
    gt = tmp_path / "gt.flo"
    flow2d.write_flo(str(gt), s.gt_u, s.gt_v)

    rc, out, plain = run_cli(flow2d, [], tmp_path / "plain", frames, w, h)
    assert rc == 0 and "Flow error" not in out
    assert set(plain) == {"t_flow-u-%d-%d.raw" % (w, h), "t_flow-v-%d-%d.raw" % (w, h), "t_res.pgm", "t_amp-%d-%d.raw" % (w, h)}
    rc, out, both = run_cli(flow2d, ["--ground-truth", str(gt), "--flo"], tmp_path / "gt", frames, w, h)
    assert rc == 0, out[-2000:]
    assert set(both) == set(plain) | {"t_flow.flo"}
    for f in plain:
        assert both[f] == plain[f], f  # the existing files do not change
    u = np.frombuffer(plain["t_flow-u-%d-%d.raw" % (w, h)], F32).reshape(h, w)
    v = np.frombuffer(plain["t_flow-v-%d-%d.raw" % (w, h)], F32).reshape(h, w)
    fu, fv = flow2d.read_flo(str(tmp_path / "gt" / "t_flow.flo"))
    assert fu.tobytes() == u.tobytes() and fv.tobytes() == v.tobytes()
    assert printed_metrics(out) == flow2d.flow_error_metrics(flow2d.evaluate_flow(u, v, s.gt_u, s.gt_v))

    # with --backward the forward occlusion mask splits noc / occ
    rc, out, bw = run_cli(flow2d, ["--backward", "--ground-truth", str(gt), "--flo"], tmp_path / "bw", frames, w, h)
    assert rc == 0, out[-2000:]
    assert {"t_flow.flo", "t_flow-backward.flo"} <= set(bw)
    occ = np.frombuffer(bw["t_occlusion-%d-%d.raw" % (w, h)], F32).reshape(h, w)
    bu = np.frombuffer(bw["t_flow-u-backward-%d-%d.raw" % (w, h)], F32).reshape(h, w)
    bu_flo, _ = flow2d.read_flo(str(tmp_path / "bw" / "t_flow-backward.flo"))
    assert bu_flo.tobytes() == bu.tobytes()
    m = printed_metrics(out)
    assert m == flow2d.flow_error_metrics(flow2d.evaluate_flow(u, v, s.gt_u, s.gt_v, occlusion=occ))
    assert m["occ"]["count"] == int((occ != 0).sum())

    # a missing, malformed or wrong-sized ground truth: the frame-load exit code, no output
    bad = tmp_path / "bad.flo"
    bad.write_bytes(gt.read_bytes()[:-4])
    small = tmp_path / "small.flo"
    flow2d.write_flo(str(small), s.gt_u[:, :-1], s.gt_v[:, :-1])
    for k, path in enumerate((tmp_path / "missing.flo", bad, small)):
        rc, out, files = run_cli(flow2d, ["--ground-truth", str(path)], tmp_path / ("bad%d" % k), frames, w, h)
        assert rc == 2 and not files, (path, rc, out[-500:])
