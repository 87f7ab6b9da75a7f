"""Bidirectional flow and forward-backward occlusion masks on the MI355X: the consistency kernel against the numpy restatement
of its definition (bit for bit), OpticalFlow2D::ComputeFlowBidirectional* against two separate ComputeFlowDevice calls (bit for
bit), an occlusion scene with known covered pixels, and the CLI's --backward."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_bidirectional_cpu import consistency_reference
from test_oracle import rub_pair

pytestmark = pytest.mark.gpu

F32 = np.float32


def random_flows(rng, w, h, edge_cases=True):
    """Forward flow: a translation of up to +-40 px plus noise, 10 % of the pixels anywhere in +-40 px; backward flow: the
    opposite translation plus noise (so both answers occur).  NaNs in both, and forward vectors that land exactly on column 0 /
    w - 1 and row 0 / h - 1."""
    t = rng.uniform(-40, 40, 2).astype(F32)
    u0 = (t[0] + rng.normal(0, 0.3, (h, w))).astype(F32)
    v0 = (t[1] + rng.normal(0, 0.3, (h, w))).astype(F32)
    wild = rng.random((h, w)) < 0.1
    u0[wild] = rng.uniform(-40, 40, wild.sum())
    v0[wild] = rng.uniform(-40, 40, wild.sum())
    u1 = (-t[0] + rng.normal(0, 0.3, (h, w))).astype(F32)
    v1 = (-t[1] + rng.normal(0, 0.3, (h, w))).astype(F32)
    if edge_cases:
        ys, xs = np.mgrid[0:h, 0:w]
        pick = rng.random((h, w))
        u0 = np.where(pick < 0.05, -xs, u0).astype(F32)                    # xf == 0
        u0 = np.where((pick >= 0.05) & (pick < 0.1), w - 1 - xs, u0).astype(F32)  # xf == w - 1
        v0 = np.where((pick >= 0.1) & (pick < 0.15), -ys, v0).astype(F32)  # yf == 0
        v0 = np.where((pick >= 0.15) & (pick < 0.2), h - 1 - ys, v0).astype(F32)  # yf == h - 1
        for a in (u0, v0, u1, v1):
            a[rng.random((h, w)) < 0.01] = np.nan
    return u0, v0, u1, v1


def device_mask(ctx, u0, v0, u1, v1, alpha1=0.01, alpha2=0.5):
    h, w = u0.shape
    planes = [ctx.plane(w, h, a) for a in (u0, v0, u1, v1)]
    out = ctx.plane(w, h)
    out.fill_bytes(0x7F)
    ctx.consistency(*planes, w, h, out, alpha1, alpha2)
    ctx.synchronize()
    m = out.download()
    for p in planes + [out]:
        p.free()
    return m


@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (7, 1), (17, 5), (584, 388), (4096, 4096)])
def test_kernel_matches_the_definition(flow2d, ctx, w, h):
    rng = np.random.default_rng(w * 10007 + h)
    u0, v0, u1, v1 = random_flows(rng, w, h)
    got = device_mask(ctx, u0, v0, u1, v1)
    want = consistency_reference(u0, v0, u1, v1)
    assert np.array_equal(got, want), "%d of %d pixels differ" % ((got != want).sum(), w * h)
    if w * h >= 1000:
        assert 0.05 < want.mean() < 0.95  # both answers are exercised


def test_kernel_non_default_alphas(flow2d, ctx):
    w, h = 331, 97
    u0, v0, u1, v1 = random_flows(np.random.default_rng(3), w, h)
    for a1, a2 in ((0.05, 2.0), (0.0, 0.0), (0.3, 0.01)):
        assert np.array_equal(device_mask(ctx, u0, v0, u1, v1, a1, a2), consistency_reference(u0, v0, u1, v1, a1, a2)), (a1, a2)


def test_kernel_lock_step_batch(flow2d, ctx):
    """Two pairs one below the other in tall containers, flow2d_context_set_batch(2, stride): one launch covers both."""
    w, h = 203, 61
    lib = flow2d.hip_lib()
    cases = [random_flows(np.random.default_rng(20 + k), w, h) for k in range(2)]
    planes = [ctx.plane(w, 2 * h, np.vstack([c[i] for c in cases])) for i in range(4)]
    out = ctx.plane(w, 2 * h)
    out.fill_bytes(0x7F)
    stride = planes[0].pitch * h
    with ctx.set_batch(2, stride):
        ctx.consistency(*planes, w, h, out, 0.02, 0.75)
        # the mask must not meet the second instance of an input either: a base inside u's second instance is refused
        assert lib.flow2d_consistency_2d(ctx.handle, planes[0].ptr, planes[1].ptr, planes[2].ptr, planes[3].ptr, w, h,
                                         planes[0].pitch, ctypes.c_float(0.01), ctypes.c_float(0.5),
                                         planes[0].ptr + stride) == 1
    ctx.synchronize()
    got = out.download()
    for k, c in enumerate(cases):
        assert np.array_equal(got[k * h:(k + 1) * h], consistency_reference(*c, 0.02, 0.75)), k


def frames_of(oracle, w, h, n, seed):
    shifts = [(0.0, 0.0), (1.5, -0.75), (2.5, 0.5), (4.0, 1.0)]
    return [oracle.synthetic_pair(w, h, dx, dy, seed=seed + k, noise=True)[1] for k, (dx, dy) in enumerate(shifts[:n])]


def check_against_pairs(flow, ctx, planes, p, fwd, bwd, occ_f, occ_b, alphas=(0.01, 0.5)):
    """Every forward / backward flow against ComputeFlowDevice in that direction, every mask against the restatement."""
    w, h = flow.width, flow.height
    pu, pv = ctx.plane(w, h), ctx.plane(w, h)
    try:
        for k in range(len(planes) - 1):
            for (a, b), (ou, ov) in (((k, k + 1), fwd[k]), ((k + 1, k), bwd[k])):
                flow.compute_flow_device(planes[a].ptr, planes[b].ptr, pu.ptr, pv.ptr, p)
                ctx.synchronize()
                u, v = pu.download(), pv.download()
                assert np.array_equal(ou.download(), u) and np.array_equal(ov.download(), v), "flow %d -> %d" % (a, b)
            if occ_f:
                u, v, bu, bv = (q.download() for q in fwd[k] + bwd[k])
                assert np.array_equal(occ_f[k].download(), consistency_reference(u, v, bu, bv, *alphas)), "occ_fwd %d" % k
                assert np.array_equal(occ_b[k].download(), consistency_reference(bu, bv, u, v, *alphas)), "occ_bwd %d" % k
    finally:
        pu.free()
        pv.free()


@pytest.mark.parametrize("w,h,constancy,sigma", [
    (200, 120, 0, 0.0), (200, 120, 0, 1.5),
    (200, 120, 1, 0.0), (200, 120, 1, 1.5),
    (200, 120, 3, 0.0), (200, 120, 3, 1.5),
    (640, 528, 1, 1.5),   # a fused-kernel level
    (640, 528, 3, 0.0),
])
def test_bidirectional_pair_matches_two_calls(flow2d, oracle, ctx, w, h, constancy, sigma):
    flow = flow2d.OpticalFlow(w, h, constancy, ctx=ctx)
    try:
        p = flow.params(4, 0.5, 2, 4, 35.0, 0.001, 0.001, 5, sigma)
        frames = frames_of(oracle, w, h, 2, seed=31)
        planes = [ctx.plane(w, h, f) for f in frames]
        fwd, bwd = [(ctx.plane(w, h), ctx.plane(w, h))], [(ctx.plane(w, h), ctx.plane(w, h))]
        occ_f, occ_b = [ctx.plane(w, h)], [ctx.plane(w, h)]
        for q in [x for pair in fwd + bwd for x in pair] + occ_f + occ_b:
            q.fill_bytes(0x33)
        flow.compute_flow_bidirectional_device([q.ptr for q in planes], [fwd[0][0].ptr], [fwd[0][1].ptr], [bwd[0][0].ptr],
                                               [bwd[0][1].ptr], p, [occ_f[0].ptr], [occ_b[0].ptr])
        ctx.synchronize()
        check_against_pairs(flow, ctx, planes, p, fwd, bwd, occ_f, occ_b)
        for q, f in zip(planes, frames):
            assert np.array_equal(q.download(), f)  # frames are only read
        # the host form: the forward flow of ComputeFlow, the backward flow of ComputeFlow on the swapped pair
        u, v, bu, bv, o0, o1, ms = flow.compute_flow_bidirectional(frames[0], frames[1], p)
        cu, cv, _ = flow.compute_flow(frames[0], frames[1], p)
        cbu, cbv, _ = flow.compute_flow(frames[1], frames[0], p)
        assert np.array_equal(u, cu) and np.array_equal(v, cv) and np.array_equal(bu, cbu) and np.array_equal(bv, cbv)
        assert np.array_equal(o0, consistency_reference(u, v, bu, bv)) and np.array_equal(o1, consistency_reference(bu, bv, u, v))
        assert ms > 0
    finally:
        flow.close()


@pytest.mark.parametrize("sigma,constancy", [(1.5, 0), (0.0, 1)])
def test_bidirectional_sequence(flow2d, oracle, ctx, sigma, constancy):
    """Four frames: three forward and three backward flows, each against its own pair; masks without and with non-default
    thresholds; a second call reuses the cache's planes and gives the same bits; without mask planes nothing else changes."""
    w, h, n = 200, 120, 4
    flow = flow2d.OpticalFlow(w, h, constancy, ctx=ctx)
    try:
        p = flow.params(4, 0.5, 2, 3, 35.0, 0.001, 0.001, 5, sigma)
        frames = frames_of(oracle, w, h, n, seed=41)
        planes = [ctx.plane(w, h, f) for f in frames]
        fwd = [(ctx.plane(w, h), ctx.plane(w, h)) for _ in range(n - 1)]
        bwd = [(ctx.plane(w, h), ctx.plane(w, h)) for _ in range(n - 1)]
        occ_f, occ_b = [ctx.plane(w, h) for _ in range(n - 1)], [ctx.plane(w, h) for _ in range(n - 1)]
        lists = [[q[0].ptr for q in fwd], [q[1].ptr for q in fwd], [q[0].ptr for q in bwd], [q[1].ptr for q in bwd]]
        for rep, alphas, masks in ((0, (0.01, 0.5), True), (1, (0.05, 1.0), True), (2, (0.01, 0.5), False)):
            for q in [x for pair in fwd + bwd for x in pair]:
                q.fill_bytes(0x33)
            extra = ([q.ptr for q in occ_f], [q.ptr for q in occ_b]) if masks else (None, None)
            flow.compute_flow_bidirectional_device([q.ptr for q in planes], *lists, p, *extra, alpha1=alphas[0], alpha2=alphas[1])
            ctx.synchronize()
            check_against_pairs(flow, ctx, planes, p, fwd, bwd, occ_f if masks else None, occ_b if masks else None, alphas)
        for q, f in zip(planes, frames):
            assert np.array_equal(q.download(), f)
        with pytest.raises(ValueError):
            flow.compute_flow_bidirectional_device([q.ptr for q in planes], *[a[:-1] for a in lists], p)
        with pytest.raises(flow2d.Flow2DError):  # an output that is one of the frames
            flow.compute_flow_bidirectional_device([q.ptr for q in planes], [planes[1].ptr] + lists[0][1:], *lists[1:], p)
        with pytest.raises(flow2d.Flow2DError):  # two outputs in one plane
            flow.compute_flow_bidirectional_device([q.ptr for q in planes], lists[0], lists[0], *lists[2:], p)
        with pytest.raises(flow2d.Flow2DError):  # a negative threshold
            flow.compute_flow_bidirectional_device([q.ptr for q in planes], *lists, p, [q.ptr for q in occ_f],
                                                   [q.ptr for q in occ_b], alpha1=-1.0)
    finally:
        flow.close()


def test_bidirectional_config3_full_size(flow2d, ctx):
    """bench.py's cfg3_4096_gradient pair (4096^2, Gradient, 8 levels at 0.5, 10 x 5 sweeps, sigma 1.5): both flows against two
    ComputeFlowDevice calls, both masks against the restatement."""
    import bench

    cfg = bench.WORKLOADS["cfg3_4096_gradient"]
    w, h = cfg["w"], cfg["h"]
    f0, f1 = bench.synthetic_pair(w, h, cfg["dx"], cfg["dy"])
    flow = flow2d.OpticalFlow(w, h, cfg["constancy"], ctx=ctx)
    try:
        p = flow.params(cfg["levels"], cfg["scale"], cfg["outer"], cfg["inner"], cfg["alpha"], 0.001, 0.001, cfg["median"],
                        cfg["sigma"])
        planes = [ctx.plane(w, h, f0), ctx.plane(w, h, f1)]
        fwd, bwd = [(ctx.plane(w, h), ctx.plane(w, h))], [(ctx.plane(w, h), ctx.plane(w, h))]
        occ_f, occ_b = [ctx.plane(w, h)], [ctx.plane(w, h)]
        flow.compute_flow_bidirectional_device([q.ptr for q in planes], [fwd[0][0].ptr], [fwd[0][1].ptr], [bwd[0][0].ptr],
                                               [bwd[0][1].ptr], p, [occ_f[0].ptr], [occ_b[0].ptr])
        ctx.synchronize()
        check_against_pairs(flow, ctx, planes, p, fwd, bwd, occ_f, occ_b)
    finally:
        flow.close()


def smooth_noise(rng, h, w, sigma):
    a = rng.normal(0, 1, (h, w))
    r = int(3 * sigma)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    a = np.apply_along_axis(lambda q: np.convolve(q, k, "same"), 1, a)
    a = np.apply_along_axis(lambda q: np.convolve(q, k, "same"), 0, a)
    return a / a.std()


def test_occlusion_scene(flow2d, oracle, ctx):
    """256 x 192: a smooth random texture moves by (+2, 0); a 64 x 64 square of its own texture, at x = 96 .. 159 and
    y = 64 .. 127 in frame 0, moves by (-6, 0).  The background of frame 0 at x in [88, 96) lands under the square in frame 1
    (8 x 64 covered pixels), and the last two columns leave the frame.  Alpha 3.5 (the rub settings' value; at 35 the flow of
    this texture's contrast stays far below 2 px).  The thresholds are the starting ones."""
    w, h, x0, y0, n = 256, 192, 96, 64, 64
    rng = np.random.default_rng(5)
    m = 16
    bg = 128 + 40 * smooth_noise(rng, h, w + 2 * m, 2.0)
    sq = 128 + 40 * smooth_noise(rng, n, n, 2.0)
    f0, f1 = bg[:, m:m + w].copy(), bg[:, m - 2:m - 2 + w].copy()
    f0[y0:y0 + n, x0:x0 + n] = sq
    f1[y0:y0 + n, x0 - 6:x0 - 6 + n] = sq
    f0, f1 = f0.astype(F32), f1.astype(F32)
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        p = flow.params(5, 0.5, 10, 5, 3.5, 0.001, 0.001, 5, 0.0)
        u, v, bu, bv, occ_0, occ_1, _ = flow.compute_flow_bidirectional(f0, f1, p)
    finally:
        flow.close()
    ou, ov, _ = oracle.compute_flow(f0, f1, 5, 0.5, 10, 5, 3.5, 0.001, 0.001, 5, 0.0, flow2d.GREY)
    assert np.array_equal(u, ou) and np.array_equal(v, ov)
    assert np.array_equal(occ_0, consistency_reference(u, v, bu, bv))
    assert np.array_equal(occ_1, consistency_reference(bu, bv, u, v))
    covered = occ_0[y0:y0 + n, x0 - 8:x0]
    assert covered.mean() >= 0.6, covered.mean()
    assert occ_0[:, w - 1].mean() >= 0.9, occ_0[:, w - 1].mean()
    ys, xs = np.mgrid[0:h, 0:w]
    # distance to the square's outline (frame 0's position) and to the frame border
    ddx = np.maximum(np.maximum(x0 - xs, xs - (x0 + n - 1)), 0)
    ddy = np.maximum(np.maximum(y0 - ys, ys - (y0 + n - 1)), 0)
    inside = (ddx == 0) & (ddy == 0)
    to_square = np.where(inside, np.minimum.reduce([xs - x0, x0 + n - 1 - xs, ys - y0, y0 + n - 1 - ys]), np.hypot(ddx, ddy))
    to_border = np.minimum.reduce([xs, w - 1 - xs, ys, h - 1 - ys])
    far = (to_square > 12) & (to_border > 12)
    assert far.sum() > 20000
    assert occ_0[far].mean() < 0.05, occ_0[far].mean()


def run_cli(flow2d, args, out_dir):
    out_dir.mkdir(exist_ok=True)
    data = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
    cmd = [flow2d.CLI_PATH] + args + ["--u8", os.path.join(data, "rub1.raw"), os.path.join(data, "rub2.raw"), "584", "388",
                                      "t_", str(out_dir) + "/"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:]
    return {f: (out_dir / f).read_bytes() for f in os.listdir(out_dir)}


def test_cli_backward(flow2d, tmp_path):
    w, h = 584, 388
    plain = run_cli(flow2d, [], tmp_path / "plain")
    both = run_cli(flow2d, ["--backward"], tmp_path / "backward")
    new = {"t_flow-u-backward-584-388.raw", "t_flow-v-backward-584-388.raw", "t_occlusion-584-388.raw",
           "t_occlusion-backward-584-388.raw", "t_occlusion.pgm"}
    assert not new & set(plain)                  # without the flag: none of the new files
    assert set(both) == set(plain) | new
    for f in plain:
        assert both[f] == plain[f], f            # the forward files are byte-identical
    for f in new - {"t_occlusion.pgm"}:
        assert len(both[f]) == w * h * 4, f
    header = b"P5\n584 388\n255\n"
    assert both["t_occlusion.pgm"][:len(header)] == header and len(both["t_occlusion.pgm"]) == len(header) + w * h
    raw = {f: np.frombuffer(both[f], F32).reshape(h, w) for f in new - {"t_occlusion.pgm"}}
    u = np.frombuffer(both["t_flow-u-584-388.raw"], F32).reshape(h, w)
    v = np.frombuffer(both["t_flow-v-584-388.raw"], F32).reshape(h, w)
    bu, bv = raw["t_flow-u-backward-584-388.raw"], raw["t_flow-v-backward-584-388.raw"]
    r1, r2 = rub_pair()
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY)
    try:  # the CLI's defaults (main.cpp): 50 levels at 0.9, 40 x 5 sweeps, alpha 35, median 5, sigma 1.5
        cu, cv, _ = flow.compute_flow(r2, r1, flow.params(50, 0.9, 40, 5, 35.0, 0.001, 0.001, 5, 1.5))
    finally:
        flow.close()
    assert np.array_equal(bu, cu) and np.array_equal(bv, cv)
    occ = raw["t_occlusion-584-388.raw"]
    assert np.array_equal(occ, consistency_reference(u, v, bu, bv))
    assert np.array_equal(raw["t_occlusion-backward-584-388.raw"], consistency_reference(bu, bv, u, v))
    pgm = np.frombuffer(both["t_occlusion.pgm"][len(header):], np.uint8).reshape(h, w)
    assert np.array_equal(pgm, np.where(occ != 0, 255, 0).astype(np.uint8))
