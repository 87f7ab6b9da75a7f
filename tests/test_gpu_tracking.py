"""Point tracking on the MI355X: flow2d_track_points_2d and flow2d_seed_points_2d bit for bit against the numpy restatement of
their definitions (tests/test_tracking_cpu.py) from 1x1 to 4096^2, repeats and a captured graph of a track-and-seed step,
OpticalFlow.track_points_device against compute_flow_bidirectional_device followed by the two kernels over more than one flow
window, the analytic scenes with their true flows, the host-image form and the CLI's --track."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

from test_tracking_cpu import seed_reference, track_reference

pytestmark = pytest.mark.gpu

F32 = np.float32
SMALL_PARAMS = (4, 0.5, 3, 5, 35.0, 0.001, 0.001, 5, 1.5)


def scenes_module():
    return importlib.import_module("cuda-flow2d_amd.scenes")


def table(ctx, values):
    """A device table (Plane of height 1) holding `values`."""
    p = ctx.plane(max(len(values), 4), 1)
    p.fill_bytes(0xFF)
    p.upload(np.asarray(values, F32).reshape(1, -1))
    return p


def download(p, n):
    return p.download(n, 1)[0]


def assert_bits(got, want, what):
    same = np.asarray(got).view(np.uint32) == np.asarray(want, F32).view(np.uint32)
    assert same.all(), "%s: %d of %d differ" % (what, (~same).sum(), same.size)


def random_tracking_case(rng, w, h, cap):
    t = rng.uniform(-3, 3, 2)
    u = (t[0] + rng.normal(0, 0.3, (h, w))).astype(F32)
    v = (t[1] + rng.normal(0, 0.3, (h, w))).astype(F32)
    bu = (-u + rng.normal(0, 0.4, (h, w))).astype(F32)
    bv = (-v + rng.normal(0, 0.4, (h, w))).astype(F32)
    for a in (u, v, bu, bv):
        a[rng.random((h, w)) < 0.01] = np.nan
    x = rng.uniform(-2, w + 1, cap).astype(F32)
    y = rng.uniform(-2, h + 1, cap).astype(F32)
    pick = rng.random(cap)
    x[pick < 0.05] = np.nan
    y[(pick >= 0.05) & (pick < 0.07)] = np.inf
    x[(pick >= 0.07) & (pick < 0.1)] = F32(w - 1)  # edge-exact positions
    y[(pick >= 0.1) & (pick < 0.13)] = F32(h - 1)
    x[(pick >= 0.13) & (pick < 0.15)] = 0
    y[(pick >= 0.15) & (pick < 0.17)] = 0
    i = pick >= 0.8  # integer positions
    x[i], y[i] = np.floor(np.clip(x[i], 0, w - 1)), np.floor(np.clip(y[i], 0, h - 1))
    return u, v, bu, bv, x, y


def run_track(ctx, case, count, back=True, boundaries=True):
    u, v, bu, bv, x, y = case
    h, w = u.shape
    cap = len(x)
    planes = [ctx.plane(w, h, a) for a in (u, v, bu, bv)]
    tx, ty = table(ctx, x), table(ctx, y)
    ox, oy = ctx.plane(max(cap, 4), 1), ctx.plane(max(cap, 4), 1)
    reason = ctx.plane(max((cap + 3) // 4, 4), 1)
    for p in (ox, oy, reason):
        p.fill_bytes(0x5A)
    n = ctx.counter(count)
    ctx.track_points(planes[0], planes[1], planes[2] if back else None, planes[3] if back else None, w, h, tx, ty, n, cap, ox, oy,
                     reason, boundaries=boundaries)
    ctx.synchronize()
    r = reason.download(max((cap + 3) // 4, 4), 1).view(np.uint8).ravel()[:cap]
    got = download(ox, cap), download(oy, cap), r.copy()
    for p in planes + [tx, ty, ox, oy, reason, n]:
        p.free()
        ctx._planes.remove(p)
    return got


@pytest.mark.parametrize("w,h,cap", [(1, 1, 5), (1, 7, 40), (9, 1, 40), (17, 5, 300), (67, 33, 5000), (333, 197, 70000),
                                     (4096, 4096, 1 << 20)])
def test_track_kernel_matches_the_definition(flow2d, ctx, w, h, cap):
    rng = np.random.default_rng(w * 7919 + h)
    case = random_tracking_case(rng, w, h, cap)
    count = cap - cap // 5
    seen = set()
    for back, boundaries in ((True, True), (False, True), (True, False)):
        got = run_track(ctx, case, count, back, boundaries)
        want = track_reference(case[0], case[1], case[2] if back else None, case[3] if back else None, case[4], case[5], count,
                               boundaries=boundaries)
        assert_bits(got[0], want[0], "x %dx%d back=%d b=%d" % (w, h, back, boundaries))
        assert_bits(got[1], want[1], "y")
        assert np.array_equal(got[2], want[2]), "reasons differ at %d slots" % (got[2] != want[2]).sum()
        seen |= set(np.unique(want[2]).tolist())
    if cap >= 300:
        assert seen == {0, 1, 2, 3, 4}, seen  # every reason occurs


def run_seed(ctx, frame, spacing, min_eig, x, y, count):
    h, w = frame.shape
    cap = len(x)
    f = ctx.plane(w, h, frame)
    tx, ty = table(ctx, x), table(ctx, y)
    n, dropped = ctx.counter(count), ctx.counter(12345)
    ctx.seed_points(f, w, h, spacing, tx, ty, n, cap, min_eig, dropped)
    got = download(tx, cap), download(ty, cap), ctx.read_count(n), ctx.read_count(dropped)
    for p in (f, tx, ty, n, dropped):
        p.free()
        ctx._planes.remove(p)
    return got


@pytest.mark.parametrize("w,h,spacing", [(1, 1, 1), (1, 9, 2), (9, 1, 1), (17, 5, 3), (67, 33, 1), (333, 197, 4),
                                         (640, 480, 1), (4096, 4096, 4)])
def test_seed_kernel_matches_the_definition(flow2d, ctx, w, h, spacing):
    rng = np.random.default_rng(w * 31 + h)
    frame = rng.uniform(0, 255, (h, w)).astype(F32)
    frame[: h // 3, : w // 3] = 7.0  # a flat corner: lambda_min = 0
    cells = (-(-w // spacing)) * (-(-h // spacing))
    for cap_factor, count, min_eig in ((1.5, 0, 0.0), (1.5, 0, 50.0), (1.0, cells // 3, 20.0), (0.6, cells // 4, 0.0)):
        cap = max(int(cells * cap_factor), 1)
        x = np.full(cap, np.nan, F32)
        y = np.full(cap, np.nan, F32)
        live = min(count, cap)
        x[:live] = rng.uniform(-1, w, live)
        y[:live] = rng.uniform(-1, h, live)
        x[: live // 10] = np.nan
        got = run_seed(ctx, frame, spacing, min_eig, x, y, count)
        want = seed_reference(frame, spacing, min_eig, x, y, count)
        assert_bits(got[0], want[0], "x %dx%d s=%d" % (w, h, spacing))
        assert_bits(got[1], want[1], "y")
        assert got[2:] == want[2:], (got[2:], want[2:])


def test_repeats_and_a_graph_replay_give_the_same_bytes(flow2d, ctx):
    """A track-and-seed step (table k -> k+1, then seeding frame k+1) twice eagerly and twice from a captured graph."""
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    w, h, s = 640, 480, 2
    rng = np.random.default_rng(3)
    case = random_tracking_case(rng, w, h, (w // s) * (h // s))
    cap = 3 * len(case[4])
    frame = rng.uniform(0, 255, (h, w)).astype(F32)
    planes = [ctx.plane(w, h, a) for a in case[:4]] + [ctx.plane(w, h, frame)]
    src_x, src_y = table(ctx, np.concatenate([case[4], np.full(cap - len(case[4]), np.nan, F32)])), \
        table(ctx, np.concatenate([case[5], np.full(cap - len(case[5]), np.nan, F32)]))
    out_x, out_y, n = ctx.plane(cap, 1), ctx.plane(cap, 1), ctx.counter(0)
    reason = ctx.plane(cap // 4, 1)
    start = len(case[4]) * 2 // 3

    def reset():
        n.upload(np.frombuffer(np.array([start, 0], np.uint64).tobytes(), F32).reshape(1, 4))
        for p in (out_x, out_y, reason):
            p.fill_bytes(0x33)
        ctx.synchronize()

    def step():
        ctx.track_points(*planes[:4], w, h, src_x, src_y, n, cap, out_x, out_y, reason)
        ctx.seed_points(planes[4], w, h, s, out_x, out_y, n, cap, 10.0)

    def state():
        return out_x.download().tobytes() + out_y.download().tobytes() + reason.download().tobytes(), ctx.read_count(n)

    reset()
    step()
    first = state()
    assert first[1] > start
    reset()
    step()
    assert state() == first
    reset()
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    step()
    graph = vp()
    assert lib.flow2d_capture_end(ctx.handle, ctypes.byref(graph)) == 0
    try:
        for _ in range(2):
            reset()
            assert lib.flow2d_graph_launch(ctx.handle, graph) == 0
            ctx.synchronize()
            assert state() == first
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)


def test_track_points_device_is_bidirectional_then_the_kernels(flow2d, ctx):
    """Seven frames (two flow windows of OpticalFlow2D::kTrackWindow = 4 pairs): the tables and counts of track_points_device
    equal compute_flow_bidirectional_device on the whole sequence followed by seeding and tracking through Context."""
    q = scenes_module().make_sequence("two_layer", 7, 96, 80, seed=4)
    n, h, w = q.frames.shape
    s, eig, cap = 3, 2.0, 4000
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        p = flow.params(*SMALL_PARAMS)
        frames = [ctx.plane(w, h, f) for f in q.frames]
        xs, ys = [ctx.plane(cap, 1) for _ in range(n)], [ctx.plane(cap, 1) for _ in range(n)]
        counts = flow.track_points_device([f.ptr for f in frames], [t.ptr for t in xs], [t.ptr for t in ys], cap, p, spacing=s,
                                          min_eigenvalue=eig)
        got_x = [download(t, cap) for t in xs]
        got_y = [download(t, cap) for t in ys]
        flows = [[ctx.plane(w, h) for _ in range(n - 1)] for _ in range(4)]
        flow.compute_flow_bidirectional_device([f.ptr for f in frames], *[[a.ptr for a in f] for f in flows], p)
        ctx.synchronize()
    finally:
        flow.close()
    rx, ry = [ctx.plane(cap, 1) for _ in range(n)], [ctx.plane(cap, 1) for _ in range(n)]
    rx[0].fill_bytes(0xFF)
    ry[0].fill_bytes(0xFF)
    cnt = ctx.counter(0)
    want_counts = []
    ctx.seed_points(frames[0], w, h, s, rx[0], ry[0], cnt, cap, eig)
    want_counts.append(ctx.read_count(cnt))
    for k in range(n - 1):
        ctx.track_points(flows[0][k], flows[1][k], flows[2][k], flows[3][k], w, h, rx[k], ry[k], cnt, cap, rx[k + 1], ry[k + 1])
        ctx.seed_points(frames[k + 1], w, h, s, rx[k + 1], ry[k + 1], cnt, cap, eig)
        want_counts.append(ctx.read_count(cnt))
    assert counts == want_counts
    for k in range(n):
        assert_bits(got_x[k], download(rx[k], cap), "x frame %d" % k)
        assert_bits(got_y[k], download(ry[k], cap), "y frame %d" % k)
    assert counts[-1] > counts[0]  # later frames were seeded


def track_true_sequence(ctx, q, spacing, boundaries, min_eig=0.0):
    """Seed and track q's frames with its true flows through Context.  Returns (xs, ys, reasons, counts): [frame_count, cap]."""
    n, h, w = q.frames.shape
    cells = (-(-w // spacing)) * (-(-h // spacing))
    cap = n * cells
    before = list(ctx._planes)
    tx, ty = [ctx.plane(cap, 1) for _ in range(n)], [ctx.plane(cap, 1) for _ in range(n)]
    reasons = [ctx.plane(cap // 4 + 4, 1) for _ in range(n)]
    tx[0].fill_bytes(0xFF)
    ty[0].fill_bytes(0xFF)
    cnt = ctx.counter(0)
    frames = [ctx.plane(w, h, f) for f in q.frames]
    counts = []
    ctx.seed_points(frames[0], w, h, spacing, tx[0], ty[0], cnt, cap, min_eig)
    counts.append(ctx.read_count(cnt))
    for k in range(n - 1):
        fl = [ctx.plane(w, h, a[k]) for a in (q.gt_u, q.gt_v, q.gt_back_u, q.gt_back_v)]
        ctx.track_points(*fl, w, h, tx[k], ty[k], cnt, cap, tx[k + 1], ty[k + 1], reasons[k + 1], boundaries=boundaries)
        ctx.synchronize()
        for a in fl:
            a.free()
            ctx._planes.remove(a)
        ctx.seed_points(frames[k + 1], w, h, spacing, tx[k + 1], ty[k + 1], cnt, cap, min_eig)
        counts.append(ctx.read_count(cnt))
    xs = np.stack([download(t, cap) for t in tx])
    ys = np.stack([download(t, cap) for t in ty])
    rs = np.stack([r.download(cap // 4 + 4, 1).view(np.uint8).ravel()[:cap] for r in reasons])
    rs[0] = 1
    for p in [p for p in ctx._planes if p not in before and p is not ctx._seed_workspace[1]]:
        p.free()
        ctx._planes.remove(p)
    return xs, ys, rs, counts


def start_frames(xs):
    """Per slot, the frame its track starts in (the first frame with a position)."""
    seen = ~np.isnan(xs)
    return np.where(seen.any(0), seen.argmax(0), -1)


@pytest.mark.parametrize("name", ["translation", "rotation", "zoom", "affine"])
def test_affine_scenes_follow_the_true_trajectories(flow2d, ctx, name):
    """Ten frames with the true flows: every alive track is within 1e-3 px of its analytic trajectory.  Rotation runs without
    the boundary test (its 3 degrees fail the paper's thresholds within ~11 px of the centre)."""
    q = scenes_module().make_sequence(name, 10, 128, 128, seed=0)
    xs, ys, rs, counts = track_true_sequence(ctx, q, 4, boundaries=name != "rotation")
    first = start_frames(xs[:, : counts[-1]])
    worst = 0.0
    for k in range(1, 10):
        for m in range(k):
            sel = np.nonzero((first == m) & ~np.isnan(xs[k, : counts[-1]]))[0]
            if sel.size == 0:
                continue
            tx, ty = q.trajectory(xs[m, sel].astype(np.float64), ys[m, sel].astype(np.float64), k, start=m)
            worst = max(worst, float(np.hypot(xs[k, sel] - tx, ys[k, sel] - ty).max()))
    assert worst < 1e-3, (name, worst)
    alive = (~np.isnan(xs[-1, : counts[0]])).sum()
    assert alive > 0.3 * counts[0], (name, alive, counts[0])
    assert set(np.unique(rs[1:, : counts[-1]])) <= {0, 1, 2, 3}  # nothing is occluded with true flows


def test_two_layer_terminations(flow2d, ctx):
    """Background tracks the square covers end with reason OCCLUDED within one frame of being covered, without the boundary
    test (which ends some of them a step earlier as MOTION_BOUNDARY).  profiles/tracking/ measures every one of them (r_occ
    1.000 in the true_no_boundaries row); the bound leaves a margin."""
    q = scenes_module().make_sequence("two_layer", 10, 256, 256, seed=0)
    xs, ys, rs, counts = track_true_sequence(ctx, q, 4, boundaries=False)
    n = counts[-1]
    first = start_frames(xs[:, :n])
    events = hits = 0
    for k in range(1, 10):
        alive_before = ~np.isnan(xs[k - 1, :n])
        sel = np.nonzero(alive_before)[0]
        m = first[sel]
        ok = np.ones(sel.size, bool)
        for start in np.unique(m):
            pick = m == start
            x0, y0 = xs[start, sel[pick]].astype(np.float64), ys[start, sel[pick]].astype(np.float64)
            on_square = q._in_square(x0, y0, start)
            ok[pick] = q.visible(x0, y0, k - 1, start=start) & ~q.visible(x0, y0, k, start=start) & ~on_square
        covered = sel[ok]
        events += covered.size
        ended = (rs[k, covered] == 4) | ((rs[min(k + 1, 9), covered] == 4) if k + 1 < 10 else False)
        hits += int(ended.sum())
    assert events > 100, events
    assert hits / events >= 0.95, (hits, events)


def test_host_form_and_cli(flow2d, ctx, tmp_path):
    q = scenes_module().make_sequence("translation", 4, 96, 64, seed=1)
    n, h, w = q.frames.shape
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        p = flow.params(*SMALL_PARAMS)
        xs, ys = flow.track_points(q.frames, p, spacing=4)
        cap = 2000
        frames = [ctx.plane(w, h, f) for f in q.frames]
        dx, dy = [ctx.plane(cap, 1) for _ in range(n)], [ctx.plane(cap, 1) for _ in range(n)]
        counts = flow.track_points_device([f.ptr for f in frames], [t.ptr for t in dx], [t.ptr for t in dy], cap, p, spacing=4)
    finally:
        flow.close()
    assert xs.shape == (n, counts[-1]) and ys.shape == xs.shape
    for k in range(n):
        assert_bits(xs[k], download(dx[k], cap)[: counts[-1]], "host form, frame %d" % k)
    assert (~np.isnan(xs[-1])).sum() > counts[0] // 2
    # the CLI: seed frame 1 at spacing 8 and track into frame 2
    data = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
    out = tmp_path / "cli"
    out.mkdir()
    cmd = [flow2d.CLI_PATH, "--track", "8", "--u8", os.path.join(data, "rub1.raw"), os.path.join(data, "rub2.raw"), "584", "388",
           "t_", str(out) + "/"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = (out / "t_tracks.txt").read_text().splitlines()
    rows = np.array([[float(t) for t in line.split()] for line in lines])
    assert rows.shape[1] == 4 and len(rows) >= 73 * 49 // 2
    summary = [line for line in r.stdout.splitlines() if line.startswith("Tracks:")]
    assert len(summary) == 1
    alive, ended, seeded = [int(t) for t in summary[0].replace(",", "").split() if t.isdigit()][:3]
    first = ~np.isnan(rows[:, 0])
    assert alive + ended == first.sum() and seeded == (~first).sum()
    assert alive == (first & ~np.isnan(rows[:, 2])).sum() and alive > 0
