"""Robust global motion and stabilisation, the parts that need no device: the new entries are exported and refuse bad arguments
before they touch the device; the numpy restatements of the three definitions (include/flow2d_c_abi.h) and of
OpticalFlow2D::ComposeGlobalMotion -- the checkers of tests/test_gpu_global_motion.py -- return the analytic scenes' exact
parameters, find the background of two_layer under its moving square, survive 30 % outliers, honour masks, fall back to the
simpler models on degenerate supports, compose associatively and stabilise an affine sequence as well as its exact motion does.

GPU_TOLERANCE, the bound of the GPU tests on the six parameters, is measured here, not guessed: the restatement runs under three
orders of summation -- row-major cumsum, numpy's pairwise sum and math.fsum -- on the GPU tests' own inputs (fit_case: the flows
of test_gpu_denoise.random_case, with their NaN, +-1e6 and +-3e38 entries) at every small test shape, and the largest spread of
any parameter is taken; GPU_TOLERANCE = max(1e3 * spread, 1e-11).  Measured: a spread of 1.0e-11 (the plain least-squares
fits, whose +-1e6 vectors put the parameters in the hundreds of pixels and the sums near 1e12; 3.8e-13 on the reweighted fits,
where those vectors weigh next to nothing), so GPU_TOLERANCE = 1.0e-8; GPU_WEIGHT_RTOL, the relative bound on weight_sum,
likewise: max(1e3 * relative spread, 1e-12) with a measured relative spread of 5.3e-13 (the weights of a pass move with the
parameters of the pass before)."""
import ctypes
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

from test_denoise_cpu import _sample, scenes_module
from test_gpu_denoise import random_case

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANSLATION, SIMILARITY, AFFINE = 0, 1, 2
MODELS = (TRANSLATION, SIMILARITY, AFFINE)
QUIET_NAN = np.full(1, 0x7FC00000, np.uint32).view(F32)[0]

SUMMERS = {
    "pairwise": lambda a: float(np.sum(a)),
    "cumsum": lambda a: float(np.cumsum(a.ravel())[-1]),
    "fsum": lambda a: math.fsum(a.ravel().tolist()),
}


# ---- the restatements ---------------------------------------------------------------------------------------------------------
def centred_grid(h, w):
    """(xc, yc) in double: x - (w - 1) / 2, y - (h - 1) / 2."""
    ys, xs = np.mgrid[0:h, 0:w].astype(F64)
    return xs - (w - 1) / 2.0, ys - (h - 1) / 2.0


def model_planes(p, h, w):
    """(mu, mv) in double: (p0 + p1*xc) + p2*yc and (p3 + p4*xc) + p5*yc."""
    xc, yc = centred_grid(h, w)
    p = [F64(q) for q in p]
    return (p[0] + p[1] * xc) + p[2] * yc, (p[3] + p[4] * xc) + p[5] * yc


def pixel_terms(u, v, mask):
    """(valid, b, u, v) of the definition: valid = |u|, |v| <= 1e9; b = valid ? 1 - clamp(mask) : 0 (fp32, then double); u = v = 0
    where not valid.  fp32 planes are compared in fp32, as the kernels do; double planes (the scenes' exact flows) in double."""
    u, v = np.asarray(u), np.asarray(v)
    with np.errstate(invalid="ignore"):
        limit = F32(1e9) if u.dtype == F32 else 1e9
        valid = (np.abs(u) <= limit) & (np.abs(v) <= limit)
        m = np.zeros(u.shape, F32) if mask is None else np.asarray(mask, F32).copy()
        m = np.where(~(m <= F32(1)), F32(1), m)
        m = np.where(~(m >= F32(0)), F32(0), m)
        b = np.where(valid, (F32(1) - m).astype(F64), 0.0)
    return valid, b, np.where(valid, u, 0).astype(F64), np.where(valid, v, 0).astype(F64)


def solve_reference(s, model):
    """(p, model_used) from the twelve sums, operation for operation."""
    p = np.zeros(6)
    s0 = s[0]
    if not s0 > 0:
        return p, -1
    mx, my, mu, mv = s[1] / s0, s[2] / s0, s[6] / s0, s[9] / s0
    cxx, cxy, cyy = s[3] / s0 - mx * mx, s[4] / s0 - mx * my, s[5] / s0 - my * my
    cxu, cyu = s[7] / s0 - mx * mu, s[8] / s0 - my * mu
    cxv, cyv = s[10] / s0 - mx * mv, s[11] / s0 - my * mv
    spread, det = cxx + cyy, cxx * cyy - cxy * cxy
    used = model
    if used == AFFINE and not (spread > 1e-9 and det > 1e-9 * (spread * spread)):
        used = SIMILARITY
    if used == SIMILARITY and not spread > 1e-9:
        used = TRANSLATION
    p1 = p2 = p4 = p5 = 0.0
    if used == AFFINE:
        p1, p2 = (cxu * cyy - cyu * cxy) / det, (cyu * cxx - cxu * cxy) / det
        p4, p5 = (cxv * cyy - cyv * cxy) / det, (cyv * cxx - cxv * cxy) / det
    elif used == SIMILARITY:
        a, b = (cxu + cyv) / spread, (cxv - cyu) / spread
        p1, p2, p4, p5 = a, -b, b, a
    p[:] = (mu - (p1 * mx + p2 * my), p1, p2, mv - (p4 * mx + p5 * my), p4, p5)
    return p, used


def global_motion_reference(u, v, mask=None, model=AFFINE, sigma=0.0, iterations=0, summer="pairwise"):
    """The record of flow2d_global_motion_2d: {"p", "weight_sum", "support", "model_used"}; `summer` picks the order of the sums
    (the one thing the definition leaves open)."""
    total = SUMMERS[summer]
    h, w = np.asarray(u).shape
    xc, yc = centred_grid(h, w)
    valid, b, ud, vd = pixel_terms(u, v, mask)
    s2 = F64(sigma) * F64(sigma)
    p, used, s = np.zeros(6), -1, None
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        for k in range(1 + (iterations if sigma > 0 else 0)):
            wgt = b
            if k > 0:
                du = ud - ((p[0] + p[1] * xc) + p[2] * yc)
                dv = vd - ((p[3] + p[4] * xc) + p[5] * yc)
                wgt = b * (s2 / (s2 + (du * du + dv * dv)))
            wx, wy = wgt * xc, wgt * yc
            terms = (wgt, wx, wy, wx * xc, wx * yc, wy * yc, wgt * ud, wx * ud, wy * ud, wgt * vd, wx * vd, wy * vd)
            s = [total(t) for t in terms]
            p, used = solve_reference(s, model)
    return {"p": p, "weight_sum": s[0], "support": int((b > 0).sum()), "model_used": used}


def _to_f32(a):
    """One rounding to fp32; every NaN becomes the quiet NaN 0x7fc00000."""
    with np.errstate(over="ignore", invalid="ignore"):
        out = np.asarray(a, F64).astype(F32)
    out[np.isnan(out)] = QUIET_NAN
    return out


def global_flow_reference(p, shape, u=None, v=None, mask=None, sigma=0.0):
    """The planes of flow2d_global_flow_2d: {"model_u", "model_v"} and, with a flow, {"residual_u", "residual_v", "weight"}."""
    h, w = shape
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        mu, mv = model_planes(p, h, w)
        out = {"model_u": _to_f32(mu), "model_v": _to_f32(mv)}
        if u is not None:
            valid, b, ud, vd = pixel_terms(u, v, mask)
            du, dv = ud - mu, vd - mv
            out["residual_u"] = np.where(valid, _to_f32(du), QUIET_NAN)
            out["residual_v"] = np.where(valid, _to_f32(dv), QUIET_NAN)
            s2 = F64(sigma) * F64(sigma)
            out["weight"] = _to_f32(b * (s2 / (s2 + (du * du + dv * dv))) if sigma > 0 else b)
    return out


def warp_global_reference(p, frame, fill=0.0):
    """(output, valid) of flow2d_warp_global_2d."""
    frame = np.asarray(frame, F32)
    h, w = frame.shape
    ys, xs = np.mgrid[0:h, 0:w].astype(F64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        mu, mv = model_planes(p, h, w)
        qx, qy = (xs + mu).astype(F32), (ys + mv).astype(F32)
        ok = (qx >= F32(0)) & (qx <= F32(w - 1)) & (qy >= F32(0)) & (qy <= F32(h - 1))
        s = _sample(frame, np.where(ok, qx, xs.astype(F32)), np.where(ok, qy, ys.astype(F32)))
    return np.where(ok, s, F32(fill)).astype(F32), ok.astype(F32)


def compose_motion(first, second):
    """The parameters of `second` after `first` (OpticalFlow2D::ComposeGlobalMotion, operation for operation)."""
    f, s = [float(q) for q in first], [float(q) for q in second]
    a1 = (1.0 + f[1], f[2], f[4], 1.0 + f[5])
    a2 = (1.0 + s[1], s[2], s[4], 1.0 + s[5])
    a11, a12 = a2[0] * a1[0] + a2[1] * a1[2], a2[0] * a1[1] + a2[1] * a1[3]
    a21, a22 = a2[2] * a1[0] + a2[3] * a1[2], a2[2] * a1[1] + a2[3] * a1[3]
    return np.array([(a2[0] * f[0] + a2[1] * f[3]) + s[0], a11 - 1.0, a12, (a2[2] * f[0] + a2[3] * f[3]) + s[3], a21, a22 - 1.0])


def invert_motion(p):
    """The parameters of the inverse map (for the tests only; plain numpy)."""
    a = np.array([[1 + p[1], p[2]], [p[4], 1 + p[5]]])
    inv = np.linalg.inv(a)
    t = -inv @ np.array([p[0], p[3]])
    return np.array([t[0], inv[0, 0] - 1, inv[0, 1], t[1], inv[1, 0], inv[1, 1] - 1])


# ---- the GPU tests' inputs and their tolerance -------------------------------------------------------------------------------------
SMALL_SHAPES = [(1, 1), (1, 9), (9, 1), (17, 5), (67, 33), (257, 33), (64, 65), (256, 256)]
MASK_MODES = ("none", "binary", "soft")
FITS = [(0.0, 0), (0.5, 0), (0.5, 1), (0.5, 5), (0.0, 5)]  # (sigma, iterations); sigma 0: least squares whatever K


def fit_case(w, h, seed=None):
    """(u, v, {"none": None, "binary": a 0 / 1 mask, "soft": uniform in [-0.5, 1.5] with NaNs}): the flows and masks of
    test_gpu_denoise.random_case -- a translation plus noise, 10 % wild vectors, NaN, +-1e6 and +-3e38 entries."""
    rng = np.random.default_rng(w * 7919 + h * 31 if seed is None else seed)
    _, _, us, vs, occs = random_case(rng, w, h, 2)
    return us[0], vs[0], {"none": None, "binary": occs[0], "soft": occs[1]}


def _measure_spread():
    spread, rel, clean = 0.0, 0.0, 0.0
    for w, h in SMALL_SHAPES:
        u, v, masks = fit_case(w, h)
        big = w * h > 10000  # the twelve sums are the same for every model: one model and one mask at the largest shape
        for mode in (("soft",) if big else MASK_MODES):
            for model in ((AFFINE,) if big else MODELS):
                for sigma, k in (FITS[0], FITS[3]) if big else FITS:
                    got = [global_motion_reference(u, v, masks[mode], model, sigma, k, order) for order in SUMMERS]
                    assert len({g["model_used"] for g in got}) == 1, (w, h, mode, model, sigma, k)
                    ps = np.array([g["p"] for g in got])
                    here = float(np.max(ps.max(0) - ps.min(0)))
                    spread = max(spread, here)
                    if sigma > 0 and k > 0:
                        clean = max(clean, here)
                    sums = [g["weight_sum"] for g in got]
                    if max(sums) > 0:
                        rel = max(rel, (max(sums) - min(sums)) / max(sums))
    return spread, rel, clean


MEASURED_SPREAD, MEASURED_WEIGHT_SPREAD, MEASURED_REWEIGHTED_SPREAD = _measure_spread()
GPU_TOLERANCE = max(1e3 * MEASURED_SPREAD, 1e-11)
GPU_WEIGHT_RTOL = max(1e3 * MEASURED_WEIGHT_SPREAD, 1e-12)


def test_gpu_tolerance_is_what_the_docstring_says():
    print("spread of the parameters %.3g (reweighted fits %.3g), of weight_sum %.3g (relative); GPU_TOLERANCE %.3g" %
          (MEASURED_SPREAD, MEASURED_REWEIGHTED_SPREAD, MEASURED_WEIGHT_SPREAD, GPU_TOLERANCE))
    assert 0 < MEASURED_SPREAD < 1e-9          # sums of ~1e12 in double: a few thousand ulps of parameters in the hundreds
    assert MEASURED_REWEIGHTED_SPREAD < 1e-11  # once the +-1e6 vectors weigh next to nothing
    assert MEASURED_WEIGHT_SPREAD < 1e-11
    assert GPU_TOLERANCE == max(1e3 * MEASURED_SPREAD, 1e-11)


# ---- exports and argument checks ------------------------------------------------------------------------------------------------
def test_new_entries_are_exported(flow2d):
    lib, host = flow2d.hip_lib(), flow2d.host_lib()
    for name in ("flow2d_global_motion_2d", "flow2d_global_motion_workspace_bytes", "flow2d_global_flow_2d", "flow2d_warp_global_2d"):
        assert hasattr(lib, name), name
    for name in ("flow2d_host_global_motion_args_ok", "flow2d_host_compose_global_motion", "flow2d_host_estimate_global_motion",
                 "flow2d_host_estimate_global_motion_device", "flow2d_host_stabilise_sequence",
                 "flow2d_host_stabilise_sequence_device"):
        assert hasattr(host, name), name
    for name in ("global_motion", "global_flow", "warp_global"):
        assert hasattr(flow2d.Context, name), name
    for name in ("estimate_global_motion", "estimate_global_motion_device", "stabilise_sequence", "stabilise_sequence_device"):
        assert hasattr(flow2d.OpticalFlow, name), name
    assert lib.flow2d_abi_version() == 1  # additions: the version stays
    assert ctypes.sizeof(flow2d.GlobalMotion) == flow2d.GLOBAL_MOTION_BYTES == 80
    header = open(os.path.join(ROOT, "include", "flow2d_c_abi.h")).read()
    assert "#define FLOW2D_GLOBAL_MOTION_BYTES 80" in header
    assert (flow2d.MOTION_TRANSLATION, flow2d.MOTION_SIMILARITY, flow2d.MOTION_AFFINE) == MODELS


def test_workspace_bytes(flow2d):
    size = flow2d.hip_lib().flow2d_global_motion_workspace_bytes
    assert size(0, 5, 1) == size(5, 0, 1) == size(5, 5, 0) == 0
    slab = size(1, 1, 1)
    assert slab > 0 and slab % 16 == 0
    assert size(256, 32, 1) == slab and size(257, 32, 1) == 2 * slab and size(256, 33, 1) == 2 * slab
    assert size(1920, 1080, 3) == 3 * 8 * 34 * slab


BASE = 0x1000000


def test_fit_rejects_bad_arguments_without_a_device(flow2d):
    """Every refusal below happens before the context is touched: the context is a zeroed stand-in and the planes are 16-byte
    aligned addresses nothing reads."""
    lib = flow2d.hip_lib()
    fake_ctx = ctypes.create_string_buffer(4096)
    ctx = ctypes.addressof(fake_ctx)
    w, h, pitch = 64, 8, 256
    need = lib.flow2d_global_motion_workspace_bytes(w, h, 1)
    d = dict(ctx=ctx, u=BASE, v=2 * BASE, mask=3 * BASE, w=w, h=h, pitch=pitch, model=AFFINE, sigma=0.5, k=5, motion=4 * BASE,
             ws=5 * BASE, ws_bytes=need)

    def call(**kw):
        a = dict(d, **kw)
        return lib.flow2d_global_motion_2d(a["ctx"], a["u"], a["v"], a["mask"], a["w"], a["h"], a["pitch"], a["model"], a["sigma"],
                                           a["k"], a["motion"], a["ws"], a["ws_bytes"])

    assert call(ctx=None) == 1
    for name in ("u", "v", "motion", "ws"):
        assert call(**{name: None}) == 1, name
    assert call(mask=3 * BASE + 4) == 1                         # an optional plane, given, is checked like the others
    assert call(w=0) == 1 and call(h=0) == 1
    assert call(pitch=8) == 1 and call(pitch=264) == 1 and call(pitch=128) == 1
    for sigma in (-1.0, -1e-30, float("nan"), float("inf"), -float("inf")):
        assert call(sigma=sigma) == 1, sigma
    assert call(k=-1) == 1 and call(k=17) == 1
    assert call(model=-1) == 1 and call(model=3) == 1
    assert call(motion=4 * BASE + 4) == 1 and call(ws=5 * BASE + 8) == 1 and call(ws_bytes=need - 1) == 1 and call(ws_bytes=0) == 1
    for p in (BASE, 2 * BASE, 3 * BASE):                          # the record and the workspace against every input plane
        assert call(motion=p + pitch) == 1 and call(motion=p + h * pitch - 8) == 1, hex(p)
        assert call(ws=p + pitch) == 1 and call(ws=p - need + 16) == 1, hex(p)
    assert call(ws=4 * BASE) == 1 and call(ws=4 * BASE + 64) == 1  # and against each other
    if flow2d.device_count() == 0:
        # arguments that pass every check reach the device guard: no device here, so a device error -- not a refusal
        assert call() == 3 and call(mask=None) == 3 and call(sigma=0.0, k=0) == 3 and call(k=16) == 3
        assert call(mask=None, motion=3 * BASE) == 3              # an absent mask's address is no input
        assert call(w=1, h=1, pitch=16) == 3
        for model in MODELS:
            assert call(model=model) == 3


def test_global_flow_and_warp_reject_bad_arguments_without_a_device(flow2d):
    lib = flow2d.hip_lib()
    fake_ctx = ctypes.create_string_buffer(4096)
    ctx = ctypes.addressof(fake_ctx)
    w, h, pitch = 64, 8, 256
    names = ("motion", "u", "v", "mask", "mu", "mv", "ru", "rv", "weight")
    planes = {n: BASE * (k + 1) for k, n in enumerate(names)}

    def flow(ctx=ctx, w=w, h=h, pitch=pitch, sigma=0.5, **kw):
        p = dict(planes, **kw)
        return lib.flow2d_global_flow_2d(ctx, p["motion"], p["u"], p["v"], p["mask"], w, h, pitch, sigma, p["mu"], p["mv"], p["ru"],
                                         p["rv"], p["weight"])

    assert flow(ctx=None) == 1 and flow(motion=None) == 1 and flow(motion=BASE + 4) == 1
    assert flow(mu=None, mv=None, ru=None, rv=None, weight=None) == 1          # no output at all
    for a, b in (("u", "v"), ("mu", "mv"), ("ru", "rv")):                      # half a pair
        assert flow(**{a: None}) == 1 and flow(**{b: None}) == 1, a
    assert flow(u=None, v=None) == 1 and flow(u=None, v=None, ru=None, rv=None) == 1  # residual / weight without the flow
    assert flow(w=0) == 1 and flow(h=0) == 1 and flow(pitch=8) == 1 and flow(pitch=264) == 1
    assert flow(mask=planes["mask"] + 4) == 1 and flow(weight=planes["weight"] + 8) == 1
    for sigma in (-1.0, float("nan"), float("inf")):
        assert flow(sigma=sigma) == 1, sigma
    for o in ("mu", "mv", "ru", "rv", "weight"):
        for n in ("u", "v", "mask"):
            assert flow(**{o: planes[n] + pitch}) == 1 and flow(**{o: planes[n] - (h - 1) * pitch}) == 1, (o, n)
        assert flow(**{o: planes["motion"] - h * pitch + 64}) == 1, o           # the records
    assert flow(mv=planes["mu"]) == 1 and flow(weight=planes["rv"] + pitch) == 1

    def warp(ctx=ctx, motion=BASE, frame=2 * BASE, w=w, h=h, pitch=pitch, out=3 * BASE, valid=4 * BASE):
        return lib.flow2d_warp_global_2d(ctx, motion, frame, w, h, pitch, ctypes.c_float(0.0), out, valid)

    assert warp(ctx=None) == 1 and warp(motion=None) == 1 and warp(motion=BASE + 4) == 1
    assert warp(frame=None) == 1 and warp(out=None) == 1 and warp(valid=4 * BASE + 4) == 1
    assert warp(w=0) == 1 and warp(h=0) == 1 and warp(pitch=8) == 1 and warp(pitch=264) == 1
    for o in ("out", "valid"):
        assert warp(**{o: 2 * BASE + pitch}) == 1 and warp(**{o: 2 * BASE - (h - 1) * pitch}) == 1, o
        assert warp(**{o: BASE - h * pitch + 64}) == 1, o
    assert warp(valid=3 * BASE) == 1 and warp(valid=3 * BASE + (h - 1) * pitch) == 1
    if flow2d.device_count() == 0:
        assert flow() == 3 and flow(mask=None) == 3 and flow(sigma=0.0) == 3
        assert flow(u=None, v=None, mask=None, ru=None, rv=None, weight=None) == 3   # the model alone needs no flow
        assert flow(mu=None, mv=None) == 3 and flow(mu=None, mv=None, ru=None, rv=None) == 3
        assert warp() == 3 and warp(valid=None) == 3 and warp(w=1, h=1, pitch=16) == 3


def test_host_layer_refuses_bad_arguments_without_a_device(flow2d):
    host = flow2d.host_lib()
    ok = host.flow2d_host_global_motion_args_ok
    assert ok(0, 0.0, 0) == 1 and ok(2, 0.5, 16) == 1 and ok(1, 3.0, 5) == 1
    assert ok(-1, 0.5, 5) == 0 and ok(3, 0.5, 5) == 0 and ok(2, 0.5, -1) == 0 and ok(2, 0.5, 17) == 0
    for s in (-1.0, float("nan"), float("inf")):
        assert ok(2, s, 5) == 0, s
    params = flow2d.OpticalFlow.params(4, 0.5, 3, 5, 35.0, 0.001, 0.001, 5, 1.5)
    frames = np.zeros((3, 8, 8), F32)
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))  # noqa: E731
    rec = (flow2d.GlobalMotion * 3)()
    arr = (ctypes.c_void_p * 3)(0x1000, 0x2000, 0x3000)
    for n, ref, model, s, k in ((1, 0, 2, 0.5, 5), (3, 3, 2, 0.5, 5), (3, 0, 3, 0.5, 5), (3, 0, 2, -1.0, 5), (3, 0, 2, 0.5, 17)):
        assert host.flow2d_host_stabilise_sequence(None, fp(frames), n, ref, model, s, k, 0, 0.0, fp(frames), rec,
                                                   ctypes.byref(params), None) == 1
        assert host.flow2d_host_stabilise_sequence_device(None, arr, n, ref, model, s, k, 0, 0.0, arr, rec, ctypes.byref(params)) == 1
    assert host.flow2d_host_estimate_global_motion(None, fp(frames), fp(frames), 2, 0.5, 5, 0, rec, ctypes.byref(params), None, None,
                                                   None, None, None) == 1
    assert host.flow2d_host_estimate_global_motion_device(None, 0x1000, 0x2000, 5, 0.5, 5, 0, rec, ctypes.byref(params), None, None,
                                                          None, None) == 1


def run_cli(args):
    exe = os.path.join(ROOT, "cuda-flow2d_amd", "host", "flow2d")
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args", [["--global-motion"], ["--global-motion", "homography"], ["--global-motion", ""],
                                  ["--global-motion", "affine", "--global-sigma", "-1"],
                                  ["--global-motion", "affine", "--global-sigma", "nan"],
                                  ["--global-motion", "affine", "--global-sigma"],
                                  ["--global-motion", "affine", "--global-iterations", "17"],
                                  ["--global-motion", "affine", "--global-iterations", "-1"],
                                  ["--global-motion", "affine", "--global-iterations", "2x"]])
def test_cli_refuses_bad_global_motion_options_before_the_device(flow2d, tmp_path, args):
    positional = ["a.raw", "b.raw", "8", "8", str(tmp_path) + "/"]
    trailing = len(args) % 2 == 1  # an option without its value goes last
    r = run_cli(positional + args if trailing else args + positional)
    assert r.returncode == 5, (args, r.stdout, r.stderr)
    assert "--global-" in r.stdout
    assert os.listdir(tmp_path) == []


# ---- the restatements on the analytic scenes ------------------------------------------------------------------------------------
def true_motion(seq):
    """The exact parameters of an affine scene's W, from the scene itself: t = W(c) - c and the columns of A - I."""
    cx, cy = (seq.width - 1) / 2.0, (seq.height - 1) / 2.0
    x0, y0 = seq.trajectory(cx, cy, 1)
    x1, y1 = seq.trajectory(cx + 1, cy, 1)
    x2, y2 = seq.trajectory(cx, cy + 1, 1)
    return np.array([x0 - cx, x1 - x0 - 1, x2 - x0, y0 - cy, y1 - y0, y2 - y0 - 1], F64)


def true_flow(seq):
    """The scene's flow of frame 0 to frame 1 in double (gt_u / gt_v before their rounding to fp32)."""
    ys, xs = np.mgrid[0:seq.height, 0:seq.width].astype(F64)
    px, py = seq.trajectory(xs, ys, 1)
    return px - xs, py - ys


CONTAINED = {"translation": MODELS, "rotation": (SIMILARITY, AFFINE), "zoom": (SIMILARITY, AFFINE), "affine": (AFFINE,)}


@pytest.mark.parametrize("name", sorted(CONTAINED))
def test_affine_scenes_return_their_exact_parameters(name):
    """With the true flow in double every model that contains the motion returns the scene's parameters to 1e-9 (measured: 4e-15
    at most); with the fp32 ground truth planes the bound is the rounding of the vectors, 2^-24 * max|flow|."""
    w, h = 67, 33
    seq = scenes_module().make_sequence(name, 2, w, h, seed=0)
    truth = true_motion(seq)
    u, v = true_flow(seq)
    for model in MODELS:
        for sigma, k in ((0.0, 0), (0.5, 3)):
            rec = global_motion_reference(u, v, None, model, sigma, k)
            err = np.abs(rec["p"] - truth).max()
            print(name, model, sigma, k, "error %.3g" % err)
            assert rec["model_used"] == model and rec["support"] == w * h
            if model in CONTAINED[name]:
                assert err < 1e-9, (name, model, err)
                if k == 0:
                    assert rec["weight_sum"] == w * h
            else:
                assert err > 1e-3, (name, model, err)      # a model that cannot hold the motion does not pretend to
    rec = global_motion_reference(seq.gt_u[0], seq.gt_v[0], None, AFFINE)
    bound = 2.0 ** -24 * max(np.abs(seq.gt_u[0]).max(), np.abs(seq.gt_v[0]).max())
    assert np.abs(rec["p"] - truth).max() < bound


def two_layer(n=64):
    return scenes_module().make_scene("two_layer", n, n, seed=0)


@pytest.mark.parametrize("model", MODELS)
def test_two_layer_background_motion(model):
    """Plain least squares reports the square's 4.5 px diluted over the frame; five reweighted passes find the static background."""
    sc = two_layer()
    plain = global_motion_reference(sc.gt_u, sc.gt_v, None, model, 0.5, 0)
    robust = global_motion_reference(sc.gt_u, sc.gt_v, None, model, 0.5, 5)
    print(model, "least squares p0 %.4f, five passes max|p| %.4g" % (plain["p"][0], np.abs(robust["p"]).max()))
    assert abs(plain["p"][0]) > 0.25
    assert np.abs(robust["p"]).max() < 5e-3
    assert robust["weight_sum"] < plain["weight_sum"] == 64 * 64


def test_thirty_per_cent_outliers():
    w, h = 67, 33
    seq = scenes_module().make_sequence("affine", 2, w, h, seed=0)
    truth = true_motion(seq)
    rng = np.random.default_rng(1)
    u, v = seq.gt_u[0].copy(), seq.gt_v[0].copy()
    bad = rng.random((h, w)) < 0.3
    u[bad] = rng.uniform(-20, 20, bad.sum())
    v[bad] = rng.uniform(-20, 20, bad.sum())
    plain = np.abs(global_motion_reference(u, v, None, AFFINE)["p"] - truth).max()
    robust = np.abs(global_motion_reference(u, v, None, AFFINE, 0.5, 3)["p"] - truth).max()
    print("error of the parameters: least squares %.3g, three passes %.3g" % (plain, robust))
    assert plain > 0.1
    assert robust < 1e-3


def test_masks_leave_their_pixels_out():
    sc = two_layer()
    mask = np.maximum(sc.occlusion, (sc.gt_u != 0).astype(F32))
    for model in MODELS:
        rec = global_motion_reference(sc.gt_u, sc.gt_v, mask, model)
        assert np.abs(rec["p"]).max() < 1e-12 and rec["model_used"] == model
        assert rec["support"] == int((mask == 0).sum()) == rec["weight_sum"]
    # a soft mask weighs, NaN and values above 1 leave out, values below 0 count fully
    u = np.array([[1.0, 3.0, 100.0, 100.0, 5.0]], F32)
    m = np.array([[0.5, -2.0, np.nan, 7.0, 0.0]], F32)
    rec = global_motion_reference(u, 2 * u, m, TRANSLATION)
    assert rec["support"] == 3 and rec["weight_sum"] == 2.5
    assert rec["p"][0] == pytest.approx((0.5 * 1 + 3 + 5) / 2.5, abs=1e-15) and rec["p"][3] == pytest.approx(2 * rec["p"][0], abs=1e-15)


def test_fallbacks():
    one = global_motion_reference(np.array([[2.5]], F32), np.array([[-1.25]], F32), None, AFFINE, 0.5, 3)
    assert one["model_used"] == TRANSLATION and one["support"] == 1
    assert np.array_equal(one["p"], [2.5, 0, 0, -1.25, 0, 0])
    rng = np.random.default_rng(0)
    for shape in ((1, 9), (9, 1)):
        u, v = rng.normal(0, 1, shape).astype(F32), rng.normal(0, 1, shape).astype(F32)
        rec = global_motion_reference(u, v, None, AFFINE)
        assert rec["model_used"] == SIMILARITY       # a line of pixels: no second direction (det = 0 exactly, spread = 20 / 3)
        assert rec["p"][1] == rec["p"][5] and rec["p"][2] == -rec["p"][4]
        assert global_motion_reference(u, v, None, SIMILARITY)["model_used"] == SIMILARITY
        assert global_motion_reference(u, v, None, TRANSLATION)["model_used"] == TRANSLATION
    u = rng.normal(0, 1, (5, 7)).astype(F32)
    for rec in (global_motion_reference(u, u, np.ones((5, 7), F32), AFFINE, 0.5, 2),
                global_motion_reference(np.full((5, 7), np.nan, F32), u, None, AFFINE, 0.5, 2),
                global_motion_reference(u, np.full((5, 7), 3e38, F32), None, SIMILARITY)):
        assert rec["model_used"] == -1 and rec["support"] == 0 and rec["weight_sum"] == 0 and not rec["p"].any()
    # one pixel left of many: a translation equal to its vector
    m = np.ones((5, 7), F32)
    m[2, 3] = 0
    rec = global_motion_reference(u, -u, m, AFFINE)
    assert rec["model_used"] == TRANSLATION and rec["p"][0] == u[2, 3] and rec["p"][3] == -u[2, 3]


def test_composition():
    rng = np.random.default_rng(3)
    a, b, c = (rng.normal(0, 0.05, 6) + [3, 0, 0, -2, 0, 0] for _ in range(3))
    left, right = compose_motion(compose_motion(a, b), c), compose_motion(a, compose_motion(b, c))
    assert np.abs(left - right).max() < 1e-12
    for p in (a, b, c):
        assert np.abs(compose_motion(p, invert_motion(p))).max() < 1e-12
        assert np.abs(compose_motion(invert_motion(p), p)).max() < 1e-12
        assert np.abs(compose_motion(p, np.zeros(6)) - p).max() < 1e-15 and np.abs(compose_motion(np.zeros(6), p) - p).max() < 1e-15
    # the map itself: second(first(x))
    x = np.array([4.0, -7.0])
    step = lambda p, x: x + np.array([p[0] + p[1] * x[0] + p[2] * x[1], p[3] + p[4] * x[0] + p[5] * x[1]])  # noqa: E731
    assert np.abs(step(compose_motion(a, b), x) - step(b, step(a, x))).max() < 1e-12
    # the families are kept bit for bit
    t = compose_motion([1.5, 0, 0, -2.25, 0, 0], [0.3, 0, 0, 0.7, 0, 0])
    assert np.array_equal(t, [1.8, 0, 0, -1.55, 0, 0])
    s1, s2 = [1.0, 0.02, -0.03, 2.0, 0.03, 0.02], [-0.5, -0.01, 0.04, 0.25, -0.04, -0.01]
    s = compose_motion(s1, s2)
    assert s[1] == s[5] and s[2] == -s[4]


def test_compose_global_motion_of_the_host_layer(flow2d):
    """OpticalFlow2D::ComposeGlobalMotion gives the restatement's numbers."""
    rng = np.random.default_rng(5)
    for _ in range(5):
        a, b = rng.normal(0, 0.1, 6), rng.normal(0, 0.1, 6)
        first, second = flow2d.GlobalMotion.from_parameters(a, SIMILARITY), flow2d.GlobalMotion.from_parameters(b, AFFINE)
        second.support, second.weight_sum = 77, 12.5
        got = flow2d.compose_global_motion(first, second)
        assert np.abs(got.parameters - compose_motion(a, b)).max() < 1e-15
        assert got.model_used == AFFINE and got.support == 77 and got.weight_sum == 12.5


def rmse(a, b, where):
    d = (a.astype(F64) - b.astype(F64))[where]
    return float(np.sqrt(np.mean(d * d)))


def test_stabilising_an_affine_sequence_with_true_flows():
    """Every frame of make_sequence("affine", 5) brought back onto frame 0 along the composed fits of the true flows shows frame
    0 again over the pixels the warp covers: the error is the bilinear sample's, no more than 1.5 times that of a warp along the
    exact W^k (the fit's 1e-9 of a pixel does not show)."""
    w, h = 96, 80
    seq = scenes_module().make_sequence("affine", 5, w, h, seed=0)
    truth = true_motion(seq)
    composed, exact = np.zeros(6), np.zeros(6)
    for k in range(1, 5):
        rec = global_motion_reference(seq.gt_u[k - 1], seq.gt_v[k - 1], None, AFFINE, 0.5, 2)
        assert rec["model_used"] == AFFINE
        composed, exact = compose_motion(composed, rec["p"]), compose_motion(exact, truth)
        assert np.abs(composed - exact).max() < 1e-6
        out, valid = warp_global_reference(composed, seq.frames[k], fill=-1.0)
        out_exact, valid_exact = warp_global_reference(exact, seq.frames[k], fill=-1.0)
        assert (out[valid == 0] == -1).all() and 0.5 < valid.mean() < 1
        both = (valid == 1) & (valid_exact == 1)
        got, want = rmse(out, seq.frames[0], both), rmse(out_exact, seq.frames[0], both)
        print("frame %d: rmse %.4f against %.4f along the exact motion, %.0f %% covered" % (k, got, want, 100 * valid.mean()))
        assert got <= 1.5 * want and want < 1.0
        assert rmse(seq.frames[k], seq.frames[0], both) > 5 * got     # it did something


def test_global_flow_and_warp_restatements():
    sc = scenes_module().make_scene("affine", 40, 24, seed=0)
    seq = scenes_module().make_sequence("affine", 2, 40, 24, seed=0)
    p = true_motion(seq)
    planes = global_flow_reference(p, (24, 40), sc.gt_u, sc.gt_v, None, 0.5)
    assert np.abs(planes["model_u"] - sc.gt_u).max() < 1e-6 and np.abs(planes["model_v"] - sc.gt_v).max() < 1e-6
    assert np.abs(planes["residual_u"]).max() < 1e-6 and planes["weight"].min() > 0.999999
    u = sc.gt_u.copy()
    u[3, 4], u[5, 6] = np.nan, 2e9
    u[7, 8] += 1.0
    planes = global_flow_reference(p, (24, 40), u, sc.gt_v, None, 0.5)
    for y, x in ((3, 4), (5, 6)):
        assert planes["residual_u"].view(np.uint32)[y, x] == planes["residual_v"].view(np.uint32)[y, x] == 0x7FC00000
        assert planes["weight"][y, x] == 0
    assert planes["residual_u"][7, 8] == pytest.approx(1.0, abs=1e-6) and planes["weight"][7, 8] == pytest.approx(0.2, abs=1e-6)
    # the warp: frame 1 along the scene's motion is frame 0; the identity returns the frame bit for bit; a far motion fills
    out, valid = warp_global_reference(p, sc.frame_1, fill=-5.0)
    assert rmse(out, sc.frame_0, valid == 1) < 0.5 and (out[valid == 0] == -5).all() and 0 < valid.mean() < 1
    out, valid = warp_global_reference(np.zeros(6), sc.frame_1)
    assert np.array_equal(out, sc.frame_1) and valid.all()
    for far in ([1e30, 0, 0, 0, 0, 0], [0, 0, 0, np.nan, 0, 0], [0, 0, 1e300, 0, 0, 0]):
        out, valid = warp_global_reference(far, sc.frame_1, fill=9.0)
        assert (out == 9).all() and not valid.any()
