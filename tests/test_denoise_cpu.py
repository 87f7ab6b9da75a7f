"""Motion-compensated temporal denoising, the parts that need no device: the new entries are exported; flow2d_denoise_2d,
flow2d_compose_flow_2d, the host layer and the CLI's --denoise refuse bad arguments before they touch the device; the numpy
restatements of the two definitions (include/flow2d_c_abi.h) -- the checkers of tests/test_gpu_denoise.py -- give hand-computed
answers, keep the noise bound of a mean of N + 1 samples on the affine scenes, gain from the true visibility on two_layer and
return the centre frame in the degenerate cases; composed true flows follow the scenes' trajectories; and the scenes' new
ground truth between any two frames agrees with what they had."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE_SIGMA = 8.0


def _grid(h, w):
    ys, xs = np.mgrid[0:h, 0:w]
    return xs.astype(F32), ys.astype(F32)


def _sample(p, qx, qy):
    """S(P, q) for q inside the frame: the bilinear sample of flow2d_consistency_2d, left to right."""
    h, w = p.shape
    xi, yi = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
    dx, dy = qx - xi.astype(F32), qy - yi.astype(F32)
    x1, y1 = np.minimum(w - 1, xi + 1), np.minimum(h - 1, yi + 1)
    one = F32(1)
    return ((one - dx) * (one - dy) * p[yi, xi] + dx * (one - dy) * p[yi, x1] + (one - dx) * dy * p[y1, xi] +
            dx * dy * p[y1, x1])


def _target(u, v):
    """q = x + flow, ok = q inside the frame (a NaN or an infinity fails), and q replaced by x where not ok."""
    h, w = u.shape
    cx, cy = _grid(h, w)
    qx, qy = cx + u, cy + v
    ok = (qx >= F32(0)) & (qx <= F32(w - 1)) & (qy >= F32(0)) & (qy <= F32(h - 1))
    return np.where(ok, qx, cx), np.where(ok, qy, cy), ok


def denoise_reference(centre, frames, us, vs, occs=None, range_sigma=0.0):
    """(output, weight_sum) of flow2d_denoise_2d, operation for operation in fp32."""
    c = np.asarray(centre, F32)
    sigma = F32(range_sigma)
    sigma_sq = sigma * sigma
    num, den = c.copy(), np.ones_like(c)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        for n in range(len(frames)):
            qx, qy, ok = _target(np.asarray(us[n], F32), np.asarray(vs[n], F32))
            s = _sample(np.asarray(frames[n], F32), qx, qy)
            occ = None if occs is None else occs[n]
            m = np.zeros_like(c) if occ is None else np.asarray(occ, F32).copy()
            m = np.where(~(m <= F32(1)), F32(1), m)
            m = np.where(~(m >= F32(0)), F32(0), m)
            d = s - c
            g = np.ones_like(c) if sigma == 0 else sigma_sq / (sigma_sq + d * d)
            wgt = np.where(ok, (F32(1) - m) * g, F32(0)).astype(F32)
            t = wgt * s
            bad = ~np.isfinite(t)
            wgt, t = np.where(bad, F32(0), wgt), np.where(bad, F32(0), t)
            num = num + t
            den = den + wgt
        return (num / den).astype(F32), den.astype(F32)


def compose_reference(ab_u, ab_v, bc_u, bc_v, mask_ab=None, mask_bc=None):
    """(out_u, out_v, out_mask) of flow2d_compose_flow_2d, operation for operation in fp32; every NaN is 0x7fc00000."""
    ab_u, ab_v, bc_u, bc_v = (np.asarray(a, F32) for a in (ab_u, ab_v, bc_u, bc_v))
    qx, qy, ok = _target(ab_u, ab_v)
    nan = F32(np.nan)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        out = []
        for first, second in ((ab_u, bc_u), (ab_v, bc_v)):
            r = first + _sample(second, qx, qy)
            out.append(np.where(ok & ~np.isnan(r), r, nan).astype(F32))
        ma = np.zeros_like(ab_u) if mask_ab is None else np.asarray(mask_ab, F32)
        sm = np.zeros_like(ab_u) if mask_bc is None else _sample(np.asarray(mask_bc, F32), qx, qy)
        mask = (~ok | ~(ma == F32(0)) | ~(sm <= F32(0))).astype(F32)
    return out[0], out[1], mask


def zeros(h, w):
    return np.zeros((h, w), F32)


def ramp(h, w, seed=0):
    return np.random.default_rng(seed).uniform(1, 255, (h, w)).astype(F32)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def scenes_module():
    return importlib.import_module("cuda-flow2d_amd.scenes")


# ---- exports and argument checks ------------------------------------------------------------------------------------------
def test_new_entries_are_exported(flow2d):
    lib, host = flow2d.hip_lib(), flow2d.host_lib()
    assert hasattr(lib, "flow2d_denoise_2d") and hasattr(lib, "flow2d_compose_flow_2d")
    for name in ("flow2d_host_denoise_sequence", "flow2d_host_denoise_sequence_device", "flow2d_host_denoise_args_ok"):
        assert hasattr(host, name), name
    assert hasattr(flow2d.Context, "denoise") and hasattr(flow2d.Context, "compose_flow")
    assert hasattr(flow2d.OpticalFlow, "denoise_sequence") and hasattr(flow2d.OpticalFlow, "denoise_sequence_device")
    assert lib.flow2d_abi_version() == 1  # additions: the version stays
    header = open(os.path.join(ROOT, "include", "flow2d_c_abi.h")).read()
    assert "#define FLOW2D_DENOISE_MAX_NEIGHBOURS 8" in header


def test_denoise_rejects_bad_arguments_without_a_device(flow2d):
    """Every refusal below happens before the context is touched: the context is a zeroed stand-in and the planes are
    16-byte aligned addresses nothing reads."""
    lib = flow2d.hip_lib()
    fake_ctx = ctypes.create_string_buffer(4096)
    ctx = ctypes.addressof(fake_ctx)
    w, h, pitch = 64, 8, 256
    base = 0x1000000
    centre, out, wsum = base, 2 * base, 3 * base
    plane = lambda kind, n: (4 + 4 * n + kind) * base  # noqa: E731  kind: 0 frame, 1 u, 2 v, 3 occlusion
    vp = ctypes.c_void_p

    def call(ctx=ctx, n=2, w=w, h=h, pitch=pitch, sigma=0.0, centre=centre, out=out, wsum=wsum, occ=True, length=None, **swap):
        length = max(n, 1) if length is None else length
        arrays = []
        for kind in range(4):
            arrays.append((vp * length)(*[swap.get("p%d_%d" % (kind, k), plane(kind, k)) for k in range(length)]))
        if swap.get("no_frames"):
            arrays[0] = None
        return lib.flow2d_denoise_2d(ctx, centre, n, arrays[0], arrays[1], arrays[2], arrays[3] if occ else None, w, h, pitch,
                                     ctypes.c_float(sigma), out, wsum)

    assert call(ctx=None) == 1
    assert call(n=0) == 1 and call(n=9, length=9) == 1 and call(n=1000, length=9) == 1
    assert call(no_frames=True) == 1
    assert call(centre=None) == 1 and call(out=None) == 1
    for kind in range(3):
        assert call(**{"p%d_1" % kind: None}) == 1, kind      # a null entry of a required array
    assert call(p3_0=plane(3, 0) + 4) == 1                     # an optional plane, given, is checked like the others
    assert call(w=0) == 1 and call(h=0) == 1
    assert call(pitch=8) == 1 and call(pitch=264) == 1 and call(w=1, pitch=0) == 1
    for sigma in (-1.0, -1e-30, float("nan"), float("inf"), -float("inf")):
        assert call(sigma=sigma) == 1, sigma
    # the byte ranges of output and weight_sum against every input's, the masks included, and against each other
    inputs = [centre] + [plane(kind, k) for kind in range(4) for k in range(2)]
    for p in inputs:
        assert call(out=p + pitch) == 1 and call(out=p - (h - 1) * pitch) == 1, hex(p)
        assert call(wsum=p + pitch) == 1 and call(wsum=p - (h - 1) * pitch) == 1, hex(p)
    assert call(wsum=out) == 1 and call(wsum=out + (h - 1) * pitch) == 1
    if flow2d.device_count() == 0:
        # arguments that pass every check reach the device guard: no device here, so a device error -- not a refusal
        assert call() == 3 and call(n=1) == 3 and call(n=8, length=8) == 3
        assert call(wsum=None) == 3 and call(occ=False, out=plane(3, 0)) == 3  # an absent mask's address is no input
        assert call(p3_1=None) == 3 and call(sigma=12.5) == 3
        assert call(w=1, h=1, pitch=16) == 3


def test_compose_rejects_bad_arguments_without_a_device(flow2d):
    lib = flow2d.hip_lib()
    fake_ctx = ctypes.create_string_buffer(4096)
    ctx = ctypes.addressof(fake_ctx)
    w, h, pitch = 64, 8, 256
    names = ("ab_u", "ab_v", "bc_u", "bc_v", "m_ab", "m_bc", "out_u", "out_v", "out_m")
    planes = {n: 0x1000000 * (k + 1) for k, n in enumerate(names)}

    def call(ctx=ctx, w=w, h=h, pitch=pitch, **kw):
        p = dict(planes, **kw)
        return lib.flow2d_compose_flow_2d(ctx, *[p[n] for n in names[:6]], w, h, pitch, *[p[n] for n in names[6:]])

    assert call(ctx=None) == 1
    for n in ("ab_u", "ab_v", "bc_u", "bc_v", "out_u", "out_v"):
        assert call(**{n: None}) == 1, n
    assert call(m_ab=planes["m_ab"] + 4) == 1 and call(out_m=planes["out_m"] + 8) == 1
    assert call(w=0) == 1 and call(h=0) == 1 and call(pitch=8) == 1 and call(pitch=264) == 1
    for o in ("out_u", "out_v", "out_m"):
        for n in names[:6]:
            assert call(**{o: planes[n] + pitch}) == 1 and call(**{o: planes[n] - (h - 1) * pitch}) == 1, (o, n)
    assert call(out_v=planes["out_u"]) == 1 and call(out_m=planes["out_v"] + pitch) == 1
    if flow2d.device_count() == 0:
        assert call() == 3 and call(m_ab=None, m_bc=None, out_m=None) == 3
        assert call(m_ab=None, out_u=planes["m_ab"]) == 3  # an absent mask's address is no input


def test_host_layer_refuses_bad_arguments_without_a_device(flow2d):
    host = flow2d.host_lib()
    ok = lambda n, r, s: host.flow2d_host_denoise_args_ok(n, r, ctypes.c_float(s))  # noqa: E731
    assert ok(2, 1, 0.0) == 1 and ok(12, 4, 25.0) == 1
    assert ok(1, 1, 0.0) == 0 and ok(0, 1, 0.0) == 0          # frame_count < 2
    assert ok(5, 0, 0.0) == 0 and ok(5, 5, 0.0) == 0          # radius 0 or 5
    for s in (-1.0, float("nan"), float("inf")):
        assert ok(5, 1, s) == 0, s
    # the entries themselves: refused (1) before the object is looked at
    params = flow2d.OpticalFlow.params(4, 0.5, 3, 5, 35.0, 0.001, 0.001, 5, 1.5)
    frames = np.zeros((3, 8, 8), F32)
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))  # noqa: E731
    for n, r, s in ((1, 1, 0.0), (3, 0, 0.0), (3, 5, 0.0), (3, 1, -2.0), (3, 1, float("nan"))):
        assert host.flow2d_host_denoise_sequence(None, fp(frames), n, r, s, 1, fp(frames), None, ctypes.byref(params), None) == 1
        arr = (ctypes.c_void_p * 3)(0x1000, 0x2000, 0x3000)
        assert host.flow2d_host_denoise_sequence_device(None, arr, n, r, s, 1, arr, None, ctypes.byref(params)) == 1


def run_cli(args):
    exe = os.path.join(ROOT, "cuda-flow2d_amd", "host", "flow2d")
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value", [None, "x", "-1", "-0.5", "nan", "inf", "-inf", "4x", "1e999", ""])
def test_cli_refuses_a_bad_denoise_sigma_before_the_device(flow2d, tmp_path, value):
    positional = ["a.raw", "b.raw", "8", "8", str(tmp_path) + "/"]
    r = run_cli(["--denoise", value] + positional if value is not None else positional + ["--denoise"])
    assert r.returncode == 5, (value, r.stdout, r.stderr)
    assert "--denoise" in r.stdout
    assert os.listdir(tmp_path) == []


# ---- the restatements: hand-computed answers ---------------------------------------------------------------------------------
def test_denoise_reference_hand_computed():
    """One row of four pixels, two neighbours.  Neighbour 0 moves by +1 (pixel 3 leaves the frame), neighbour 1 by -0.5
    (pixel 0 leaves): mean of the valid samples."""
    c = np.array([[10, 20, 30, 40]], F32)
    f0 = np.array([[1, 2, 3, 4]], F32)
    f1 = np.array([[100, 200, 300, 400]], F32)
    z = zeros(1, 4)
    out, den = denoise_reference(c, [f0, f1], [z + F32(1), z - F32(0.5)], [z, z])
    assert np.array_equal(den, np.array([[2, 3, 3, 2]], F32))
    # pixel 0: (10 + f0[1]) / 2; pixel 1: (20 + f0[2] + (f1[0] + f1[1]) / 2) / 3; pixel 3: (40 + (f1[2] + f1[3]) / 2) / 2
    want = np.array([[(10 + 2) / 2, (20 + 3 + 150) / 3, (30 + 4 + 250) / 3, (40 + 350) / 2]], F32)
    assert np.array_equal(out, want)
    # masks: 1 drops the neighbour, 0.5 halves it, NaN and 2 count as 1, -1 as 0
    occ0 = np.array([[1, 0.5, np.nan, 0]], F32)
    occ1 = np.array([[0, 2, -1, 0.25]], F32)
    out, den = denoise_reference(c, [f0, f1], [z + F32(1), z - F32(0.5)], [z, z], [occ0, occ1])
    assert np.array_equal(den, np.array([[1, 1.5, 2, 1.75]], F32))
    want = np.array([[10, (20 + 0.5 * 3) / 1.5, (30 + 250) / 2, (40 + 0.75 * 350) / 1.75]], F32)
    assert np.array_equal(out, want)
    # a None entry of the mask list is "nothing occluded"
    out2, den2 = denoise_reference(c, [f0, f1], [z + F32(1), z - F32(0.5)], [z, z], [None, occ1])
    assert np.array_equal(den2, np.array([[2, 2, 3, 1.75]], F32))


def test_denoise_reference_range_weight():
    """g = sigma^2 / (sigma^2 + d^2): d = sigma halves the neighbour, d = 0 keeps it, a huge d removes it."""
    c = np.array([[10, 10, 10, 10]], F32)
    f = np.array([[10, 14, 6, 3e30]], F32)
    z = zeros(1, 4)
    out, den = denoise_reference(c, [f], [z], [z], range_sigma=4.0)
    assert np.array_equal(den, np.array([[2, 1.5, 1.5, 1]], F32))
    assert np.array_equal(out, np.array([[10, (10 + 7) / 1.5, (10 + 3) / 1.5, 10]], F32))
    # sigma = 0: no photometric weight
    out, den = denoise_reference(c, [f], [z], [z], range_sigma=0.0)
    assert np.array_equal(den, np.full((1, 4), 2, F32)) and out[0, 1] == F32(12)
    # a NaN or infinite sample contributes nothing, with and without the photometric weight
    f_bad = np.array([[np.nan, np.inf, -np.inf, 20]], F32)
    for sigma in (0.0, 4.0):
        out, den = denoise_reference(c, [f_bad], [z], [z], range_sigma=sigma)
        assert np.array_equal(den[0, :3], np.ones(3, F32)) and np.array_equal(out[0, :3], c[0, :3]), sigma


@pytest.mark.parametrize("sigma", [0.0, 7.5])
def test_degenerate_calls_return_the_centre(sigma):
    """Every mask 1, every flow NaN, every flow leaving the frame: the centre frame bit for bit, weight sum 1."""
    h, w, n = 9, 13, 3
    rng = np.random.default_rng(5)
    c = ramp(h, w, 1)
    frames = [ramp(h, w, 2 + k) for k in range(n)]
    flows = [rng.uniform(-3, 3, (h, w)).astype(F32) for _ in range(2 * n)]
    ones = [np.ones((h, w), F32)] * n
    nan = [np.full((h, w), np.nan, F32)] * n
    far = [np.full((h, w), 1e6, F32), np.full((h, w), -3e38, F32), np.full((h, w), np.inf, F32)]
    for us, vs, occs in ((flows[:n], flows[n:], ones), (nan, flows[n:], None), (flows[:n], nan, None), (far, flows[n:], None),
                         (flows[:n], far, None)):
        out, den = denoise_reference(c, frames, us, vs, occs, sigma)
        assert same_bits(out, c) and same_bits(den, np.ones((h, w), F32))


def test_compose_reference_hand_computed():
    """a -> b moves by +1 in x, b -> c by +0.5 in y on b's grid, with a ramp in its u."""
    h, w = 3, 4
    ab_u, ab_v = np.ones((h, w), F32), zeros(h, w)
    bc_u = np.tile(np.arange(w, dtype=F32), (h, 1)) * F32(0.25)  # u_bc(x) = x / 4
    bc_v = np.full((h, w), 0.5, F32)
    u, v, m = compose_reference(ab_u, ab_v, bc_u, bc_v)
    # q = x + 1: inside for x <= 2; out_u = 1 + (x + 1) / 4, out_v = 0.5; the last column leaves the frame: NaN, mask 1
    assert np.array_equal(u[:, :3], np.tile(np.array([1.25, 1.5, 1.75], F32), (h, 1)))
    assert np.array_equal(v[:, :3], np.full((h, 3), 0.5, F32))
    assert (u[:, 3].view(np.uint32) == 0x7FC00000).all() and (v[:, 3].view(np.uint32) == 0x7FC00000).all()
    assert np.array_equal(m, np.tile(np.array([0, 0, 0, 1], F32), (h, 1)))
    # masks: a's own mask, and b's mask carried along a -> b (any positive sample counts)
    m_ab = zeros(h, w)
    m_ab[0, 0] = 1
    m_bc = zeros(h, w)
    m_bc[1, 2] = 0.5
    _, _, m = compose_reference(ab_u, ab_v, bc_u, bc_v, m_ab, m_bc)
    want = np.tile(np.array([0, 0, 0, 1], F32), (h, 1))
    want[0, 0] = 1
    want[1, 1] = 1  # x = 1 lands on (2, 1) of b
    assert np.array_equal(m, want)
    # a NaN in b -> c where a -> b lands: the canonical NaN
    bc_bad = bc_u.copy()
    bc_bad[0, 1] = -np.nan
    u, _, _ = compose_reference(ab_u, ab_v, bc_bad, bc_v)
    assert u[0, 0].view(np.uint32) == 0x7FC00000 and np.isfinite(u[1:, :3]).all() and np.isfinite(u[0, 1:3]).all()


def test_compose_with_a_zero_flow_returns_the_other():
    """Zero on either side: the other flow bit for bit where the position is inside the frame."""
    h, w = 17, 23
    rng = np.random.default_rng(8)
    fu, fv = (rng.uniform(-6, 6, (h, w)).astype(F32) for _ in range(2))
    z = zeros(h, w)
    u, v, m = compose_reference(z, z, fu, fv)          # zero first: q = x, S(f, x) = f[x]
    assert same_bits(u, fu) and same_bits(v, fv) and not m.any()
    u, v, m = compose_reference(fu, fv, z, z)          # zero second: w_ab + 0
    _, _, ok = _target(fu, fv)
    assert ok.sum() > h * w // 4 and (~ok).sum() > 0
    assert same_bits(u[ok], fu[ok]) and same_bits(v[ok], fv[ok]) and np.isnan(u[~ok]).all() and np.isnan(v[~ok]).all()
    assert np.array_equal(m, (~ok).astype(F32))


# Measured here with this file's restatement on the four scenes at 256 x 256, 5 frames, every chain 2 -> 3 -> 4 and 2 -> 1 -> 0:
# the largest deviation of a composed flow component from the trajectory over two steps, in pixels
COMPOSE_MEASURED_DEVIATION = 1.9e-6


@pytest.mark.parametrize("name", ["translation", "rotation", "zoom", "affine"])
def test_composed_true_flows_follow_the_trajectory(name):
    """The true consecutive flows of an affine sequence composed over two steps, forwards (2 -> 3 -> 4) and backwards
    (2 -> 1 -> 0), against Sequence.trajectory_between where the first step stays inside the frame.  The bilinear sample of an
    affine flow is exact up to rounding, so the tolerance is the largest deviation the float32 restatement itself shows on these
    scenes -- measured: translation 3.81e-7, rotation 1.86e-6, zoom 8.49e-7, affine 1.84e-6 px; COMPOSE_MEASURED_DEVIATION is
    the largest, rounded up -- plus one float32 ulp of the largest flow component (4.8e-7 .. 9.5e-7 px here)."""
    seq = scenes_module().make_sequence(name, 5, 256, 256, seed=0)
    worst = 0.0
    for mid, end in ((3, 4), (1, 0)):
        ab_u, ab_v, _ = seq.flow_between(2, mid)
        bc_u, bc_v, _ = seq.flow_between(mid, end)
        u, v, m = compose_reference(ab_u, ab_v, bc_u, bc_v)
        ys, xs = np.mgrid[0:256, 0:256].astype(np.float64)
        tx, ty = seq.trajectory_between(xs, ys, 2, end)
        ok = m == 0
        assert ok.mean() > 0.8 and np.isnan(u[~ok]).all()
        tol = COMPOSE_MEASURED_DEVIATION + float(np.spacing(F32(max(np.abs(tx - xs)[ok].max(), np.abs(ty - ys)[ok].max()))))
        dev = max(np.abs(u[ok] - (tx - xs)[ok]).max(), np.abs(v[ok] - (ty - ys)[ok]).max())
        print("%s 2->%d->%d: deviation %.3g px, tolerance %.3g" % (name, mid, end, dev, tol))
        worst = max(worst, dev)
        assert dev <= tol, (name, mid, end, dev, tol)
    assert worst > 0  # the comparison is not vacuous


# ---- the scenes ---------------------------------------------------------------------------------------------------------------
def noisy(frames, seed=0, sigma=NOISE_SIGMA):
    """Seeded Gaussian noise of standard deviation `sigma` added to the exact frames."""
    rng = np.random.default_rng(1000 + seed)
    return (frames.astype(np.float64) + rng.normal(0, sigma, frames.shape)).astype(F32)


def neighbours_of(seq, frames, k, radius, masks):
    """(frames, us, vs, occs) of centre k in ascending frame order, with the true flows and, with masks, the true visibility."""
    js = [j for j in range(k - radius, k + radius + 1) if j != k and 0 <= j < seq.frame_count]
    flows = [seq.flow_between(k, j) for j in js]
    occs = [(~f[2]).astype(F32) for f in flows] if masks else None
    return [frames[j] for j in js], [f[0] for f in flows], [f[1] for f in flows], occs


def rmse(a, b, sel):
    e = (a.astype(np.float64) - b.astype(np.float64))[sel]
    return float(np.sqrt((e * e).mean()))


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("name", ["translation", "rotation", "zoom", "affine"])
def test_noise_bound_on_the_affine_scenes(name, radius):
    """No photometric weight, no masks: a pixel whose N neighbours are all valid is the mean of N + 1 samples, each a bilinear
    sample whose weights' squares sum to at most 1, so independent noise of standard deviation s per frame leaves at most
    s / sqrt(N + 1).  With b the RMSE of the same call on the noise-free frames: RMSE <= b + s / sqrt(N + 1) over those pixels,
    which are at least 85 % of the frame."""
    seq = scenes_module().make_sequence(name, 5, 256, 256, seed=0)
    k, n = 2, 2 * radius
    clean = seq.frames
    noised = noisy(clean)
    out_clean, den_clean = denoise_reference(clean[k], *neighbours_of(seq, clean, k, radius, False))
    out, den = denoise_reference(noised[k], *neighbours_of(seq, noised, k, radius, False))
    assert np.array_equal(den, den_clean)
    full = den == F32(n + 1)
    left_out = 1.0 - full.mean()
    b = rmse(out_clean, clean[k], full)
    got = rmse(out, clean[k], full)
    bound = b + NOISE_SIGMA / np.sqrt(n + 1)
    print("%s radius %d: rmse %.3f, bound %.3f (b %.3f), left out %.1f %%, before %.3f" %
          (name, radius, got, bound, b, 100 * left_out, rmse(noised[k], clean[k], full)))
    assert left_out <= 0.15, left_out
    assert got <= bound, (got, bound)


def test_two_layer_true_visibility_helps():
    """True flows; over the pixels of the centre frame whose content is hidden in some neighbour, the true visibility as masks
    gives a lower RMSE than no masks (which average in the occluder).  Values: profiles/denoising/README.md."""
    seq = scenes_module().make_sequence("two_layer", 5, 256, 256, seed=0)
    k, radius = 2, 2
    clean, noised = seq.frames, noisy(seq.frames)
    with_masks = neighbours_of(seq, noised, k, radius, True)
    hidden = np.zeros(clean[k].shape, bool)
    for occ in with_masks[3]:
        hidden |= occ != 0
    assert hidden.sum() > 500
    out_m, _ = denoise_reference(noised[k], *with_masks)
    out_p, _ = denoise_reference(noised[k], *neighbours_of(seq, noised, k, radius, False))
    e_m, e_p = rmse(out_m, clean[k], hidden), rmse(out_p, clean[k], hidden)
    print("two_layer hidden pixels %d: rmse with masks %.3f, without %.3f" % (hidden.sum(), e_m, e_p))
    assert e_m < e_p, (e_m, e_p)


@pytest.mark.parametrize("name", ["translation", "rotation", "zoom", "affine", "two_layer"])
def test_sequence_ground_truth_between_frames(name):
    """flow_between / visible_between: for neighbouring frames the arrays the sequence already had; over two steps the texture
    is matched exactly where the point is seen; backwards is the inverse of forwards."""
    seq = scenes_module().make_sequence(name, 4, 96, 80, seed=3)
    h, w = 80, 96
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    for k in range(3):
        u, v, _ = seq.flow_between(k, k + 1)
        assert np.array_equal(u, seq.gt_u[k]) and np.array_equal(v, seq.gt_v[k])
        bu, bv, _ = seq.flow_between(k + 1, k)
        assert np.array_equal(bu, seq.gt_back_u[k]) and np.array_equal(bv, seq.gt_back_v[k])
    for start, end in ((0, 2), (3, 1), (1, 3), (2, 0)):
        px, py = seq.trajectory_between(xs, ys, start, end)
        seen = seq.visible_between(xs, ys, start, end)
        assert seen.mean() > 0.5
        diff = np.abs(seq.frame_at(end, px, py) - seq.frame_at(start, xs, ys))
        assert diff[seen].max() <= 1e-8, (start, end, diff[seen].max())
        # and back again
        qx, qy = seq.trajectory_between(px, py, end, start)
        assert np.abs(qx - xs)[seen].max() <= 1e-9 and np.abs(qy - ys)[seen].max() <= 1e-9
    u, v, seen = seq.flow_between(1, 1)
    assert not u.any() and not v.any() and seen.all()
