"""Point tracking, the parts that need no device: the new entries are exported, flow2d_track_points_2d and flow2d_seed_points_2d
refuse bad arguments (and lock-step batches) before they touch the device, the CLI refuses a bad --track value, the numpy
restatement of both definitions (include/flow2d_c_abi.h) -- the checker of tests/test_gpu_tracking.py -- gives hand-computed
answers, and the sequences of scenes.make_sequence carry exact ground truth."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = F32(np.nan)


def bilinear(p, px, py):
    """S(P, p) of flow2d_consistency_2d for positions inside the frame, left to right in fp32."""
    h, w = p.shape
    xi, yi = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    dx, dy = px - xi.astype(F32), py - yi.astype(F32)
    x1, y1 = np.minimum(w - 1, xi + 1), np.minimum(h - 1, yi + 1)
    one = F32(1)
    return ((one - dx) * (one - dy) * p[yi, xi] + dx * (one - dy) * p[yi, x1] + (one - dx) * dy * p[y1, xi] +
            dx * dy * p[y1, x1])


def _inside(x, y, w, h):
    return (x >= F32(0)) & (x <= F32(w - 1)) & (y >= F32(0)) & (y <= F32(h - 1))


def track_reference(u, v, bu, bv, x, y, count, alpha1=0.01, alpha2=0.5, boundaries=True, beta1=0.01, beta2=0.002):
    """(out_x, out_y, reason) of flow2d_track_points_2d, operation for operation in fp32.  bu = bv = None: no forward-backward
    check.  capacity = len(x)."""
    u, v = np.asarray(u, F32), np.asarray(v, F32)
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    h, w = u.shape
    cap = x.size
    reason = np.zeros(cap, np.uint8)
    open_ = np.ones(cap, bool)

    def decide(cond, code):
        hit = open_ & cond
        reason[hit] = code
        open_[hit] = False

    with np.errstate(invalid="ignore", over="ignore"):
        decide((np.arange(cap) >= count) | ~np.isfinite(x) | ~np.isfinite(y), 1)
        decide(~_inside(x, y, w, h), 3)
        px, py = np.where(open_, x, F32(0)), np.where(open_, y, F32(0))  # safe positions for the slots already decided
        u0, v0 = bilinear(u, px, py), bilinear(v, px, py)
        m0 = u0 * u0 + v0 * v0
        if boundaries:
            ix = np.floor(px + F32(0.5)).astype(np.int64)
            iy = np.floor(py + F32(0.5)).astype(np.int64)
            xl, xr = np.maximum(ix - 1, 0), np.minimum(ix + 1, w - 1)
            yu, yd = np.maximum(iy - 1, 0), np.minimum(iy + 1, h - 1)
            half = F32(0.5)
            ux, uy = half * (u[iy, xr] - u[iy, xl]), half * (u[yd, ix] - u[yu, ix])
            vx, vy = half * (v[iy, xr] - v[iy, xl]), half * (v[yd, ix] - v[yu, ix])
            g = (ux * ux + uy * uy) + (vx * vx + vy * vy)
            decide(~(g <= F32(beta1) * m0 + F32(beta2)), 2)
        qx, qy = px + u0, py + v0
        decide(~np.isfinite(qx) | ~np.isfinite(qy), 4)
        decide(~_inside(qx, qy, w, h), 3)
        if bu is not None:
            bu, bv = np.asarray(bu, F32), np.asarray(bv, F32)
            sx, sy = np.where(open_, qx, F32(0)), np.where(open_, qy, F32(0))
            b_u, b_v = bilinear(bu, sx, sy), bilinear(bv, sx, sy)
            eu, ev = u0 + b_u, v0 + b_v
            decide(~(eu * eu + ev * ev <= F32(alpha1) * (m0 + (b_u * b_u + b_v * b_v)) + F32(alpha2)), 4)
    out_x = np.where(reason == 0, qx, NAN).astype(F32)
    out_y = np.where(reason == 0, qy, NAN).astype(F32)
    return out_x, out_y, reason


def min_eigenvalues(frame, sx, sy):
    """lambda_min of flow2d_seed_points_2d at the pixels (sx, sy), in fp32."""
    f = np.asarray(frame, F32)
    h, w = f.shape
    a = np.zeros(sx.shape, F32)
    b = np.zeros(sx.shape, F32)
    c = np.zeros(sx.shape, F32)
    half = F32(0.5)
    for dy in range(-2, 3):
        yy = np.clip(sy + dy, 0, h - 1)
        for dx in range(-2, 3):
            xx = np.clip(sx + dx, 0, w - 1)
            gx = half * (f[yy, np.minimum(xx + 1, w - 1)] - f[yy, np.maximum(xx - 1, 0)])
            gy = half * (f[np.minimum(yy + 1, h - 1), xx] - f[np.maximum(yy - 1, 0), xx])
            a = a + gx * gx
            b = b + gx * gy
            c = c + gy * gy
    with np.errstate(invalid="ignore", over="ignore"):
        return half * (a + c) - np.sqrt(F32(0.25) * (a - c) * (a - c) + b * b)


def seed_reference(frame, spacing, min_eigenvalue, x, y, count):
    """flow2d_seed_points_2d on copies of the tables: returns (x, y, new count, dropped).  capacity = len(x)."""
    h, w = np.asarray(frame).shape
    x, y = np.array(x, F32), np.array(y, F32)
    s = spacing
    cw, ch = -(-w // s), -(-h // s)
    covered = np.zeros(ch * cw, bool)
    n = min(count, x.size)
    with np.errstate(invalid="ignore"):
        live = np.isfinite(x[:n]) & np.isfinite(y[:n]) & _inside(x[:n], y[:n], w, h)
    cx = np.floor(x[:n][live]).astype(np.int64) // s
    cy = np.floor(y[:n][live]).astype(np.int64) // s
    covered[cy * cw + cx] = True
    j, i = np.divmod(np.arange(ch * cw), cw)
    sx, sy = np.minimum(i * s + s // 2, w - 1), np.minimum(j * s + s // 2, h - 1)
    seed = ~covered
    if min_eigenvalue != 0:
        seed &= min_eigenvalues(frame, sx, sy) >= F32(min_eigenvalue)
    cells = np.nonzero(seed)[0]
    avail = max(x.size - count, 0)
    put = cells[:avail]
    x[count:count + put.size] = sx[put].astype(F32)
    y[count:count + put.size] = sy[put].astype(F32)
    return x, y, count + put.size, cells.size - put.size


def test_new_entries_are_exported(flow2d):
    lib = flow2d.hip_lib()
    for name in ("flow2d_track_points_2d", "flow2d_seed_points_2d", "flow2d_seed_points_workspace_bytes"):
        assert hasattr(lib, name), name
    host = flow2d.host_lib()
    assert hasattr(host, "flow2d_host_track_points") and hasattr(host, "flow2d_host_track_points_device")
    for name in ("track_points", "seed_points", "counter", "read_count"):
        assert hasattr(flow2d.Context, name), name
    assert hasattr(flow2d.OpticalFlow, "track_points") and hasattr(flow2d.OpticalFlow, "track_points_device")
    assert lib.flow2d_abi_version() == 1  # an addition: the version stays
    assert lib.flow2d_seed_points_workspace_bytes(0, 4, 1) == 0 and lib.flow2d_seed_points_workspace_bytes(4, 4, 0) == 0
    assert lib.flow2d_seed_points_workspace_bytes(64, 48, 4) > 16 * 12


def set_batch(lib, ctx, count, stride):
    return lib.flow2d_context_set_batch(ctypes.c_void_p(ctx), ctypes.c_size_t(count), ctypes.c_size_t(stride))


def _fake_context():
    buf = ctypes.create_string_buffer(4096)  # a zeroed stand-in: batch count 0, nothing a device call could use
    return buf, ctypes.addressof(buf)


def test_track_rejects_bad_arguments_without_a_device(flow2d):
    lib = flow2d.hip_lib()
    buf, ctx = _fake_context()
    w, h, pitch, cap = 64, 8, 256, 1000
    names = ("u", "v", "bu", "bv", "x", "y", "count", "ox", "oy", "reason")
    ptrs = {n: 0x1000000 * (k + 1) for k, n in enumerate(names)}

    def call(ctx=ctx, w=w, h=h, pitch=pitch, cap=cap, a1=0.01, a2=0.5, b1=0.01, b2=0.002, **kw):
        p = dict(ptrs, **kw)
        return lib.flow2d_track_points_2d(ctx, p["u"], p["v"], p["bu"], p["bv"], w, h, pitch, p["x"], p["y"], p["count"], cap,
                                          a1, a2, 1, b1, b2, p["ox"], p["oy"], p["reason"])

    assert call(ctx=None) == 1
    for n in ("u", "v", "x", "y", "count", "ox", "oy"):
        assert call(**{n: None}) == 1, n
    assert call(bu=None) == 1 and call(bv=None) == 1  # both back planes or neither
    assert call(w=0) == 1 and call(h=0) == 1 and call(cap=0) == 1
    assert call(pitch=8) == 1 and call(pitch=264) == 1 and call(w=1, pitch=0) == 1
    assert call(u=ptrs["u"] + 4) == 1 and call(count=ptrs["count"] + 4) == 1
    for k in ("a1", "a2", "b1", "b2"):
        for bad in (-0.01, float("nan"), float("inf")):
            assert call(**{k: bad}) == 1, (k, bad)
    # outputs overlapping an input, the count or each other
    assert call(ox=ptrs["x"] + 400) == 1 and call(oy=ptrs["u"] + 4 * 100) == 1 and call(ox=ptrs["count"]) == 1
    assert call(oy=ptrs["ox"] + 3996) == 1 and call(reason=ptrs["oy"] + 3999) == 1
    assert call(reason=ptrs["count"] - 999) == 1
    # unsupported: a capacity beyond what the kernel indexes, and a lock-step batch
    assert call(cap=1 << 40) == 5
    assert set_batch(lib, ctx, 2, 4096) == 0
    assert call() == 5
    assert set_batch(lib, ctx, 1, 0) == 0


def test_seed_rejects_bad_arguments_without_a_device(flow2d):
    lib = flow2d.hip_lib()
    buf, ctx = _fake_context()
    w, h, pitch, cap, s = 64, 8, 256, 1000, 4
    need = lib.flow2d_seed_points_workspace_bytes(w, h, s)
    names = ("frame", "x", "y", "count", "dropped", "ws")
    ptrs = {n: 0x1000000 * (k + 1) for k, n in enumerate(names)}

    def call(ctx=ctx, w=w, h=h, pitch=pitch, s=s, e=1.0, cap=cap, wsb=need, **kw):
        p = dict(ptrs, **kw)
        return lib.flow2d_seed_points_2d(ctx, p["frame"], w, h, pitch, s, e, p["x"], p["y"], p["count"], cap, p["dropped"],
                                         p["ws"], wsb)

    assert call(ctx=None) == 1
    for n in ("frame", "x", "y", "count", "ws"):
        assert call(**{n: None}) == 1, n
    assert call(w=0) == 1 and call(h=0) == 1 and call(s=0) == 1 and call(cap=0) == 1
    assert call(pitch=8) == 1 and call(pitch=264) == 1
    for bad in (-1.0, float("nan"), float("inf")):
        assert call(e=bad) == 1, bad
    assert call(wsb=need - 1) == 1 and call(ws=ptrs["ws"] + 8) == 1
    assert call(count=ptrs["count"] + 4) == 1 and call(dropped=ptrs["dropped"] + 4) == 1
    assert call(x=ptrs["frame"] + 1024) == 1 and call(y=ptrs["x"] + 3996) == 1 and call(count=ptrs["y"] + 16) == 1
    assert call(dropped=ptrs["count"]) == 1 and call(ws=ptrs["frame"] + 1024) == 1 and call(dropped=ptrs["ws"] + need - 8) == 1
    assert call(cap=1 << 40) == 5
    big = lib.flow2d_seed_points_workspace_bytes(1 << 17, 1 << 17, 2)  # 2^32 cells
    assert call(w=1 << 17, h=1 << 17, pitch=1 << 19, s=2, wsb=big, frame=1 << 44) == 5
    assert set_batch(lib, ctx, 3, 4096) == 0
    assert call() == 5
    assert set_batch(lib, ctx, 1, 0) == 0


def test_cli_refuses_a_bad_track_spacing(flow2d):
    for bad in (["--track"], ["--track", "0"], ["--track", "-2"], ["--track", "x"], ["--track", "2.5"]):
        p = subprocess.run([flow2d.CLI_PATH] + bad, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60,
                           env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert p.returncode == 5, (bad, p.stdout)
        assert "--track" in p.stdout


def planes(h, w, u=0.0, v=0.0):
    return np.full((h, w), u, F32), np.full((h, w), v, F32)


def test_integer_translation_is_carried_exactly():
    u, v = planes(6, 8, 2.0, -1.0)
    x = np.array([0, 3.25, 4.5, 7, 2], F32)
    y = np.array([1, 2.75, 5, 4, 0.5], F32)
    ox, oy, r = track_reference(u, v, -u, -v, x, y, 5)
    assert list(r) == [0, 0, 0, 3, 3]  # x = 7 + 2 leaves on the right, y = 0.5 - 1 at the top
    assert list(ox[:3]) == [2, 5.25, 6.5] and list(oy[:3]) == [0, 1.75, 4]
    assert np.isnan(ox[3:]).all() and np.isnan(oy[3:]).all()


def test_a_point_leaving_each_edge():
    h, w = 5, 6
    for (du, dv), (px, py) in [((-1.5, 0), (1, 2)), ((1.5, 0), (4, 2)), ((0, -1.5), (2, 1)), ((0, 1.5), (2, 3))]:
        u, v = planes(h, w, du, dv)
        _, _, r = track_reference(u, v, None, None, np.array([px], F32), np.array([py], F32), 1)
        assert r[0] == 3, (du, dv)
    # a point already outside, and points exactly on the edge (inside)
    u, v = planes(h, w)
    _, _, r = track_reference(u, v, None, None, np.array([-0.01, 5.0, 0.0, 5.01], F32), np.array([0, 4, 4, 0], F32), 4)
    assert list(r) == [3, 0, 0, 3]


def test_nan_flow_and_inactive_slots():
    u, v = planes(4, 4, 0.5, 0.5)
    u[1, 1] = np.nan
    x = np.array([1, 1, 2, np.nan, np.inf, 0], F32)
    y = np.array([1, 1, 2, 1, 1, 0], F32)
    ox, _, r = track_reference(u, v, None, None, x, y, 5, boundaries=True)
    assert list(r) == [2, 2, 0, 1, 1, 1]  # the NaN sample fails the boundary test; (2, 2) touches no NaN; slot 5 >= count
    _, _, r = track_reference(u, v, None, None, x, y, 5, boundaries=False)
    assert list(r) == [4, 4, 0, 1, 1, 1]  # without it, q is NaN: occluded
    assert np.isnan(ox).sum() == 5


def test_forward_backward_failure():
    u, v = planes(8, 8, 1.0, 0.0)
    bu, bv = planes(8, 8, -1.0, 0.0)
    bu[:, 5] = 1.0  # the backward flow at column 5 does not cancel: |e|^2 = 4 > 0.01 * 2 + 0.5
    x = np.array([2, 4, 3.5], F32)
    y = np.array([3, 3, 3], F32)
    _, _, r = track_reference(u, v, bu, bv, x, y, 3)
    assert list(r) == [0, 4, 4]  # 3.5 + 1 samples half of column 5: |e|^2 = 1 > 0.52
    _, _, r = track_reference(u, v, None, None, x, y, 3)
    assert list(r) == [0, 0, 0]


def test_motion_boundary_failure():
    u, v = planes(8, 8)
    u[:, 4:] = 1.0
    x = np.array([1, 3, 4.6, 6], F32)
    y = np.array([2, 2, 2, 2], F32)
    _, _, r = track_reference(u, v, None, None, x, y, 4)
    # 3: ux = 0.5 * (1 - 0) = 0.5, g = 0.25 > 0.01 * 0 + 0.002; 4.6 rounds to 5: ux = 0.5 * (1 - 1) = 0
    assert list(r) == [0, 2, 0, 0]
    _, _, r = track_reference(u, v, None, None, x, y, 4, beta2=0.3)
    assert list(r) == [0, 0, 0, 0]


def test_seeding_order_capacity_and_drops():
    frame = np.zeros((6, 9), F32)
    # spacing 4: cells 3 x 2, seed pixels x in (2, 6, 8), y in (2, 5)
    x = np.full(8, NAN)
    y = np.full(8, NAN)
    x[0], y[0] = 6.5, 1.0  # covers cell (1, 0)
    x[1], y[1] = np.inf, 1.0  # not finite: covers nothing
    nx, ny, n, dropped = seed_reference(frame, 4, 0.0, x, y, 2)
    assert n == 7 and dropped == 0
    assert list(zip(nx[2:7], ny[2:7])) == [(2, 2), (8, 2), (2, 5), (6, 5), (8, 5)]
    assert nx[0] == 6.5 and np.isinf(nx[1]) and np.isnan(nx[7])
    nx, ny, n, dropped = seed_reference(frame, 4, 0.0, x[:4], y[:4], 2)
    assert n == 4 and dropped == 3 and list(nx[2:]) == [2, 8]
    # a flat frame has lambda_min = 0: nothing is seeded above a threshold
    _, _, n, dropped = seed_reference(frame, 4, 1e-3, x, y, 2)
    assert n == 2 and dropped == 0
    # spacing 1: every pixel a cell; a track on (3, 4) covers it
    x1 = np.full(60, NAN)
    y1 = np.full(60, NAN)
    x1[0], y1[0] = 3.9, 4.0
    nx, ny, n, _ = seed_reference(frame, 1, 0.0, x1, y1, 1)
    assert n == 54 and (nx[1], ny[1]) == (0, 0) and (3, 4) not in set(zip(nx[1:n], ny[1:n]))


def test_min_eigenvalue_of_a_corner():
    frame = np.zeros((9, 9), F32)
    frame[4:, 4:] = 100.0
    lam = min_eigenvalues(frame, np.array([4, 1, 4]), np.array([4, 1, 7]))
    assert lam[0] > 1000 and lam[1] == 0 and abs(lam[2]) < 1e-3  # a corner, a flat area, a straight edge


def test_sequences_carry_exact_ground_truth():
    scenes = importlib.import_module("cuda-flow2d_amd.scenes")
    for name in scenes.SCENES:
        q = scenes.make_sequence(name, 4, 48, 40, seed=2)
        s = scenes.make_scene(name, 48, 40, seed=2)
        assert q.frames.shape == (4, 40, 48) and q.gt_u.shape == (3, 40, 48)
        assert np.array_equal(q.frames[0], s.frame_0) and np.array_equal(q.frames[1], s.frame_1)
        ys, xs = np.mgrid[0:40, 0:48].astype(np.float64)
        for k in range(3):
            tx, ty = q.trajectory(xs, ys, k + 1, start=k)
            assert np.array_equal(q.gt_u[k], (tx - xs).astype(F32)) and np.array_equal(q.gt_v[k], (ty - ys).astype(F32))
            # the point keeps its grey level along the true motion where it stays seen
            seen = q.visible(xs, ys, k + 1, start=k)
            assert np.abs(q.frame_at(k + 1, tx, ty) - q.frame_at(k, xs, ys))[seen].max() < 1e-9, (name, k)
            bx, by = xs + q.gt_back_u[k], ys + q.gt_back_v[k]
            if name == "two_layer":  # the square shown in frame k + 1 moves back by -t, the rest stays
                moved = (q.gt_back_u[k] != 0) | (q.gt_back_v[k] != 0)
                assert q.gt_back_u[k][moved].tolist() == [-4.5] * int(moved.sum())
                assert moved.sum() == q.gt_u[k].astype(bool).sum()
            else:  # W^-1 then W is the identity
                fx, fy = q.trajectory(bx, by, k + 1, start=k)
                assert np.abs(fx - xs).max() < 1e-4 and np.abs(fy - ys).max() < 1e-4, name
        x3, y3 = q.trajectory(xs, ys, 3)
        if name != "two_layer":
            assert np.allclose(q.frame_at(3, x3, y3), q.frame_at(0, xs, ys), atol=1e-9)


def test_two_layer_visibility():
    scenes = importlib.import_module("cuda-flow2d_amd.scenes")
    q = scenes.make_sequence("two_layer", 6, 64, 64, seed=0)
    # the square: n = 16 at (20, 24) in frame 0, moving by (4.5, -2.25) per frame
    assert q.visible(38.0, 30.0, 0) and not q.visible(38.0, 30.0, 1)  # background, covered in frame 1
    assert not q.visible(41.0, 30.0, 2) and not q.visible(41.0, 30.0, 4) and q.visible(41.0, 30.0, 5)  # covered in frames 2-4
    assert q.visible(22.0, 30.0, 5)  # on the square: moves along
    x, y = q.trajectory(22.0, 30.0, 5)
    assert (x, y) == (22.0 + 22.5, 30.0 - 11.25)
    edge = scenes.make_sequence("two_layer", 12, 48, 48, seed=0)  # the square leaves the top edge after a few frames
    assert edge.visible(20.0, 18.5, 3) and not edge.visible(20.0, 18.5, 9)
