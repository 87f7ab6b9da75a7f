"""Frame interpolation, the parts that need no device: the new entries are exported, flow2d_interpolate_2d and the CLI's
--interpolate refuse bad arguments before they touch the device, the numpy restatement of the definition (include/flow2d_c_abi.h,
flow2d_interpolate_2d) -- the checker of tests/test_gpu_interpolation.py -- gives hand-computed answers, and the scenes' new
ground truth (frame_at_time, the backward flow, frame 1's occlusion) is exact while their existing arrays keep their values."""
import ctypes
import hashlib
import importlib
import os
import subprocess

import numpy as np
import pytest

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sample(p, px, py, cx, cy):
    """S(P, p) of flow2d_interpolate_2d: non-finite positions become the pixel itself, then clamped, then the bilinear sample
    of flow2d_consistency_2d (left to right)."""
    h, w = p.shape
    bad = ~(np.isfinite(px) & np.isfinite(py))
    px, py = np.where(bad, cx, px), np.where(bad, cy, py)
    px = np.where(px < F32(0), F32(0), np.where(px > F32(w - 1), F32(w - 1), px))
    py = np.where(py < F32(0), F32(0), np.where(py > F32(h - 1), F32(h - 1), py))
    xi, yi = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    dx, dy = px - xi.astype(F32), py - yi.astype(F32)
    x1, y1 = np.minimum(w - 1, xi + 1), np.minimum(h - 1, yi + 1)
    one = F32(1)
    return ((one - dx) * (one - dy) * p[yi, xi] + dx * (one - dy) * p[yi, x1] + (one - dx) * dy * p[y1, xi] +
            dx * dy * p[y1, x1])


def _side(u, v, frame, occ, f, iterations, max_residual_sq, cx, cy):
    h, w = frame.shape
    px, py = cx, cy
    for _ in range(iterations):
        px, py = cx - f * _sample(u, px, py, cx, cy), cy - f * _sample(v, px, py, cx, cy)
    su, sv = _sample(u, px, py, cx, cy), _sample(v, px, py, cx, cy)
    rx, ry = cx - f * su - px, cy - f * sv - py
    ok = (px >= F32(0)) & (px <= F32(w - 1)) & (py >= F32(0)) & (py <= F32(h - 1)) & (rx * rx + ry * ry <= max_residual_sq)
    a = _sample(frame, px, py, cx, cy)
    c = np.zeros_like(a) if occ is None else _sample(occ, px, py, cx, cy)
    c = np.where(ok, c, F32(0))
    c = np.where(~(c <= F32(1)), F32(1), c)
    c = np.where(~(c >= F32(0)), F32(0), c)
    return a, ok, c, (px, py)


def interpolation_reference(frame_0, frame_1, u, v, bu, bv, t, occ_0=None, occ_1=None, iterations=2, max_residual=0.5,
                            details=False):
    """The output of flow2d_interpolate_2d, operation for operation in fp32.  details=True also returns a dict with ok0 / ok1,
    c0 / c1, a0 / a1 and the fixed points p / q."""
    frame_0, frame_1, u, v, bu, bv = (np.asarray(a, F32) for a in (frame_0, frame_1, u, v, bu, bv))
    occ_0 = None if occ_0 is None else np.asarray(occ_0, F32)
    occ_1 = None if occ_1 is None else np.asarray(occ_1, F32)
    h, w = frame_0.shape
    ys, xs = np.mgrid[0:h, 0:w]
    cx, cy = xs.astype(F32), ys.astype(F32)
    t = F32(t)
    s = F32(1) - t
    mr2 = F32(max_residual) * F32(max_residual)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a0, ok0, c0, p = _side(u, v, frame_0, occ_0, t, iterations, mr2, cx, cy)
        a1, ok1, c1, q = _side(bu, bv, frame_1, occ_1, s, iterations, mr2, cx, cy)
        k0, k1 = ok0.astype(F32), ok1.astype(F32)
        v0, v1 = k0 * (F32(1) - c0), k1 * (F32(1) - c1)
        both = v0 + v1 > F32(0)
        w0 = np.where(both, s * v0, s * k0)
        w1 = np.where(both, t * v1, t * k1)
        den = w0 + w1
        out = np.where(den > F32(0), (w0 * a0 + w1 * a1) / den, s * a0 + t * a1).astype(F32)
    if details:
        return out, {"ok0": ok0, "ok1": ok1, "c0": c0, "c1": c1, "a0": a0, "a1": a1, "p": p, "q": q}
    return out


def zeros(h, w):
    return np.zeros((h, w), F32)


def ramp(h, w, seed=0):
    return np.random.default_rng(seed).uniform(0, 255, (h, w)).astype(F32)


def test_new_entries_are_exported(flow2d):
    assert hasattr(flow2d.hip_lib(), "flow2d_interpolate_2d")
    host = flow2d.host_lib()
    assert hasattr(host, "flow2d_host_interpolate_frames")
    assert hasattr(host, "flow2d_host_interpolate_frames_device")
    assert hasattr(flow2d.Context, "interpolate")
    assert hasattr(flow2d.OpticalFlow, "interpolate_frames")
    assert hasattr(flow2d.OpticalFlow, "interpolate_frames_device")
    assert flow2d.hip_lib().flow2d_abi_version() == 1  # an addition: the version stays


def test_interpolate_rejects_bad_arguments_without_a_device(flow2d):
    """Every refusal below happens before the context is touched: the context is a zeroed stand-in and the planes are
    16-byte aligned addresses nothing reads."""
    lib = flow2d.hip_lib()
    fake_ctx = ctypes.create_string_buffer(4096)
    ctx = ctypes.addressof(fake_ctx)
    w, h, pitch = 64, 8, 256
    names = ("f0", "f1", "u", "v", "bu", "bv", "o0", "o1", "out")
    planes = {n: 0x1000000 * (k + 1) for k, n in enumerate(names)}

    def call(ctx=ctx, w=w, h=h, pitch=pitch, t=0.5, k=2, r=0.5, **kw):
        p = dict(planes, **kw)
        return lib.flow2d_interpolate_2d(ctx, p["f0"], p["f1"], p["u"], p["v"], p["bu"], p["bv"], p["o0"], p["o1"], w, h,
                                         pitch, t, k, r, p["out"])

    assert call(ctx=None) == 1
    for plane in ("f0", "f1", "u", "v", "bu", "bv", "out"):
        assert call(**{plane: None}) == 1, plane
    assert call(o0=planes["o0"] + 4) == 1  # an optional plane, given, is checked like the others
    assert call(w=0) == 1 and call(h=0) == 1
    assert call(pitch=8) == 1 and call(pitch=264) == 1  # narrower than a row; not a multiple of 16
    assert call(w=1, pitch=0) == 1
    for t in (-0.01, 1.01, float("nan"), float("inf"), -float("inf")):
        assert call(t=t) == 1, t
    for k in (0, -1, 17, 1000):
        assert call(k=k) == 1, k
    for r in (-0.5, float("nan"), float("inf")):
        assert call(r=r) == 1, r
    # the output's byte range [out, out + h * pitch) against every input's, the masks included
    for n in ("f0", "f1", "u", "v", "bu", "bv", "o0", "o1"):
        assert call(out=planes[n] + pitch) == 1, n                 # starts inside the input
        assert call(out=planes[n] - (h - 1) * pitch) == 1, n       # ends inside it
    if flow2d.device_count() == 0:
        # arguments that pass every check reach the device guard: no device here, so a device error -- not a refusal
        assert call() == 3
        assert call(o0=None, o1=None, out=planes["o0"]) == 3  # an absent mask's address is no input
        assert call(w=1, h=1, pitch=16, t=0.0, k=1, r=0.0) == 3 and call(t=1.0, k=16) == 3


def run_cli(args):
    exe = os.path.join(ROOT, "cuda-flow2d_amd", "host", "flow2d")
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value", [None, "x", "3.5", "1", "0", "-2", "4x"])
def test_cli_refuses_a_bad_interpolate_count_before_the_device(flow2d, tmp_path, value):
    args = ["--interpolate"] + ([] if value is None else [value])
    r = run_cli(args + ["a.raw", "b.raw", "8", "8", str(tmp_path) + "/"] if value is not None else
                ["a.raw", "b.raw", "8", "8", str(tmp_path) + "/"] + args)
    assert r.returncode == 5, (value, r.stdout, r.stderr)
    assert "--interpolate" in r.stdout
    assert os.listdir(tmp_path) == []


def test_reference_integer_translation():
    """Translation by (+2, 0) with its exact backward flow: every interior pixel of the middle frame is the average of the two
    frames' samples on the trajectory, both sides agree."""
    h, w = 6, 12
    f0 = ramp(h, w, 1)
    f1 = np.zeros_like(f0)
    f1[:, 2:] = f0[:, :-2]
    u, bu = np.full((h, w), 2, F32), np.full((h, w), -2, F32)
    out, d = interpolation_reference(f0, f1, u, zeros(h, w), bu, zeros(h, w), 0.5, details=True)
    # x at t = 0.5 comes from x - 1 in frame 0 and x + 1 in frame 1
    assert np.array_equal(d["p"][0][:, 1:], np.broadcast_to(np.arange(0, w - 1, dtype=F32), (h, w - 1)))
    assert np.array_equal(d["q"][0][:, :-1], np.broadcast_to(np.arange(1, w, dtype=F32), (h, w - 1)))
    assert d["ok0"][:, 1:].all() and d["ok1"][:, :-1].all()
    assert not d["ok0"][:, 0].any() and not d["ok1"][:, -1].any()  # the trajectory starts outside the frame
    mid = out[:, 1:w - 1]
    assert np.array_equal(mid, f0[:, 0:w - 2])  # f1[x + 1] == f0[x - 1]: the weighted mean of equal values
    # a side whose trajectory starts outside alone carries the weight (only side 1 at column 0)
    assert np.array_equal(out[:, 0], f1[:, 1])
    assert np.array_equal(out[:, -1], f0[:, -2])


@pytest.mark.parametrize("iterations", [1, 2, 16])
def test_reference_t0_and_t1_are_the_frames(iterations):
    rng = np.random.default_rng(3)
    h, w = 9, 13
    f0, f1 = ramp(h, w, 4), ramp(h, w, 5)
    u, v, bu, bv = (rng.uniform(-30, 30, (h, w)).astype(F32) for _ in range(4))
    assert np.array_equal(interpolation_reference(f0, f1, u, v, bu, bv, 0.0, iterations=iterations), f0)
    assert np.array_equal(interpolation_reference(f0, f1, u, v, bu, bv, 1.0, iterations=iterations), f1)


def test_reference_nan_flow():
    """A NaN flow: at t = 1 side 1's fixed point is x - 0 * NaN = NaN (0 * NaN breaks q = x), so ok1 is false there and the
    NaN is sampled as the pixel itself.  The definition then falls back to the plain blend s*a0 + t*a1 = frame_1 (finite
    frames): the output stays frame_1, but only through the fallback."""
    h, w = 5, 7
    f0, f1 = ramp(h, w, 6), ramp(h, w, 7)
    u, v, bu, bv = (np.full((h, w), 0.25, F32) for _ in range(4))
    bu[2, 3] = np.nan
    out, d = interpolation_reference(f0, f1, u, v, bu, bv, 1.0, details=True)
    # the NaN reaches (2, 3) and its left / upper neighbours through the bilinear sample's zero weights (0 * NaN)
    bad = ~np.isfinite(d["q"][0])
    assert bad[2, 3] and bad[1, 2] and bad[2, 2] and bad[1, 3] and bad.sum() == 4
    assert not d["ok1"][bad].any() and d["ok1"][~bad].all()
    assert np.array_equal(d["a1"], f1)  # sampled at the pixel itself
    assert np.array_equal(out, f1)
    # with finite flows the same call takes the weighted branch: w1 = 1, w0 = 0
    out2, d2 = interpolation_reference(f0, f1, u, v, np.full((h, w), 0.25, F32), bv, 1.0, details=True)
    assert d2["ok1"].all() and np.array_equal(out2, f1)
    # a NaN in the forward flow at t = 0.5 drops side 0 there: side 1 alone
    u2 = u.copy()
    u2[:, :] = np.nan
    out3, d3 = interpolation_reference(f0, f1, u2, v, bu, bv, 0.5, details=True)
    assert not d3["ok0"].any()
    sel = d3["ok1"]
    assert np.array_equal(out3[sel], d3["a1"][sel])


def test_reference_out_of_frame_side():
    """A flow far out of the frame: side 0 lands outside (ok0 false) and side 1 alone is used; when both sides fail the plain
    blend s*a0 + t*a1 at the clamped positions is the output."""
    h, w = 4, 6
    f0, f1 = ramp(h, w, 8), ramp(h, w, 9)
    far = np.full((h, w), -1e6, F32)
    out, d = interpolation_reference(f0, f1, far, zeros(h, w), zeros(h, w), zeros(h, w), 0.25, details=True)
    assert not d["ok0"].any() and d["ok1"].all()
    assert np.array_equal(out, f1)  # w0 = s * ok0 = 0: frame 1 alone
    # the clamped sample of side 0 is column w - 1 (x + 0.25e6 clamps to the right edge)
    assert np.array_equal(d["a0"], np.repeat(f0[:, -1:], w, 1))
    # both sides out: the plain blend
    out2, d2 = interpolation_reference(f0, f1, far, zeros(h, w), -far, zeros(h, w), 0.25, details=True)
    assert not d2["ok0"].any() and not d2["ok1"].any()
    t, s = F32(0.25), F32(0.75)
    assert np.array_equal(out2, s * d2["a0"] + t * d2["a1"])
    # an overflowing position (inf) is not finite: sampled at the pixel itself, never valid
    huge = np.full((h, w), 3e38, F32)
    out3, d3 = interpolation_reference(f0, f1, huge, huge, huge, huge, 1.0, iterations=1, details=True)
    # p_1 = x - 3e38 is finite, clamped to column 0 and row 0, not replaced; side 1 (s = 0) stays at the pixel
    assert not d3["ok0"].any() and d3["ok1"].all()
    assert np.array_equal(d3["a0"], np.full((h, w), f0[0, 0], F32))
    assert np.array_equal(out3, f1)


def test_reference_residual_bound():
    """A flow that is not constant along the trajectory leaves a residual; max_residual decides whether the side counts."""
    h, w = 1, 8
    f0, f1 = ramp(h, w, 10), ramp(h, w, 11)
    u = np.arange(w, dtype=F32)[None, :]  # u(x) = x: x - t * u(p) has the fixed point x / (1 + t), reached only in the limit
    z = zeros(h, w)
    _, d = interpolation_reference(f0, f1, u, z, z, z, 0.5, iterations=1, max_residual=0.0, details=True)
    assert d["ok0"][0, 0] and not d["ok0"][0, 1:].any()
    _, d = interpolation_reference(f0, f1, u, z, z, z, 0.5, iterations=1, max_residual=100.0, details=True)
    assert d["ok0"].all()


def test_reference_masks():
    """Mask values: 0.5 halves a side's weight, NaN and values above 1 count as occluded, negatives as visible; content seen in
    both frames wins over content seen in one."""
    h, w = 3, 4
    f0, f1 = np.full((h, w), 10, F32), np.full((h, w), 30, F32)
    z = zeros(h, w)
    occ0 = np.full((h, w), 0.5, F32)
    out, d = interpolation_reference(f0, f1, z, z, z, z, 0.5, occ_0=occ0, details=True)
    # v0 = 0.5, v1 = 1: w0 = 0.25, w1 = 0.5 -> (2.5 + 15) / 0.75
    assert np.array_equal(d["c0"], occ0) and np.array_equal(out, np.full((h, w), (F32(2.5) + F32(15)) / F32(0.75), F32))
    for value, want_c in ((np.nan, 1.0), (2.0, 1.0), (-1.0, 0.0), (1.0, 1.0)):
        out, d = interpolation_reference(f0, f1, z, z, z, z, 0.5, occ_0=np.full((h, w), value, F32), details=True)
        assert (d["c0"] == F32(want_c)).all(), value
    # frame 0 occluded everywhere: side 1 alone, the output is frame 1
    out = interpolation_reference(f0, f1, z, z, z, z, 0.5, occ_0=np.ones((h, w), F32))
    assert np.array_equal(out, f1)
    # both occluded: v0 + v1 = 0, the weights fall back to s * ok0, t * ok1: the plain mean
    out = interpolation_reference(f0, f1, z, z, z, z, 0.25, occ_0=np.ones((h, w), F32), occ_1=np.ones((h, w), F32))
    assert np.array_equal(out, np.full((h, w), (F32(0.75) * F32(10) + F32(0.25) * F32(30)) / F32(1), F32))
    # a mask is sampled only where the side is valid: an out-of-frame side has c = 0 whatever the mask holds
    far = np.full((h, w), 1e6, F32)
    _, d = interpolation_reference(f0, f1, far, z, z, z, 0.5, occ_0=np.ones((h, w), F32), details=True)
    assert not d["ok0"].any() and (d["c0"] == 0).all()


def test_reference_both_weights_zero():
    """t = 0 with side 0 invalid and side 1 valid: w0 = s * 0, w1 = t * 1 = 0, so w0 + w1 = 0 and the output is the plain
    blend s*a0 + t*a1 = a0, frame 0 sampled at the pixel itself."""
    h, w = 3, 5
    f0, f1 = ramp(h, w, 12), ramp(h, w, 13)
    nan = np.full((h, w), np.nan, F32)
    z = zeros(h, w)
    out, d = interpolation_reference(f0, f1, nan, z, z, z, 0.0, details=True)
    assert not d["ok0"].any() and d["ok1"].all()
    assert np.array_equal(out, f0)


def scenes_module():
    return importlib.import_module("cuda-flow2d_amd.scenes")


@pytest.mark.parametrize("name", ["translation", "rotation", "zoom", "affine", "two_layer"])
def test_scene_frame_at_time_ends(name):
    s = scenes_module().make_scene(name, 96, 80, seed=3)
    assert np.abs(s.frame_at_time(0.0) - s.frame_0).max() <= 1e-3
    assert np.abs(s.frame_at_time(1.0) - s.frame_1).max() <= 1e-3
    mid = s.frame_at_time(0.5)
    assert mid.dtype == F32 and mid.shape == s.shape
    assert np.abs(mid - s.frame_0).max() > 1.0 and np.abs(mid - s.frame_1).max() > 1.0


@pytest.mark.parametrize("name", ["translation", "rotation", "zoom", "affine", "two_layer"])
def test_scene_backward_ground_truth_is_exact(name):
    """I0(y + w_b(y)) == I1(y) at every visible pixel of frame 1, with the analytic textures in double."""
    s = scenes_module().make_scene(name, 96, 80, seed=3)
    h, w = s.shape
    assert s.gt_back_u.shape == s.gt_back_v.shape == (h, w) and s.gt_back_u.dtype == s.gt_back_v.dtype == F32
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    bu, bv = s.back_flow_at(xs, ys)
    assert np.array_equal(s.gt_back_u, bu.astype(F32)) and np.array_equal(s.gt_back_v, bv.astype(F32))
    visible = np.ones((h, w), bool) if s.occlusion_1 is None else s.occlusion_1 == 0
    i0 = s.frame_0_at(xs + bu, ys + bv)
    assert np.abs(i0 - s.frame_1_at(xs, ys))[visible].max() <= 1e-9
    # the stored float32 flow, as the forward test checks gt_u / gt_v
    i0 = s.frame_0_at(xs + s.gt_back_u.astype(np.float64), ys + s.gt_back_v.astype(np.float64))
    assert np.abs(i0 - s.frame_1)[visible].max() < 1e-4
    assert np.abs(np.hypot(s.gt_back_u, s.gt_back_v)).max() > 0.5


def test_two_layer_occlusion_of_frame_1():
    """Frame 1's occluded pixels are the background the square uncovered; they have no match in frame 0."""
    s = scenes_module().make_scene("two_layer", 128, 96, seed=0)
    h, w = s.shape
    occ = s.occlusion_1 != 0
    shown = (s.gt_back_u != 0) | (s.gt_back_v != 0)
    assert occ.sum() > 0 and not (occ & shown).any()
    assert occ.sum() == (s.occlusion != 0).sum()  # the square covers as much as it uncovers
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    i0 = s.frame_0_at(xs + s.gt_back_u, ys + s.gt_back_v)
    assert np.median(np.abs(i0 - s.frame_1)[occ]) > 1.0
    for name in ("translation", "rotation", "zoom", "affine"):
        assert scenes_module().make_scene(name, 32, 32).occlusion_1 is None


# sha256 of every array the scenes had before frame interpolation (values rounded to 0.01 grey levels / pixels)
EXISTING_HASHES = {
    "translation": "4d67612b64409b2fea903cc04920dedf7f4f295def51fe6d50faa6d8698352a7",
    "rotation": "48441bdd2137e8f5f2da956ddadb5d3664df1262b5c2b54efb84e02bd6f6610f",
    "zoom": "1827cb311b8404886ee6a1cdb92201a8ca9134caa17163c3f676d9c977fb686e",
    "affine": "809618c4a8a92f1b9d35e8f95cc9b4a1ee3e5887620729c1441ac2044f12afaa",
    "two_layer": "a8ba03e2cd86dad11e03fa7171e29427af629052c04da99b76d8dd7eb8ee8fa2",
}


@pytest.mark.parametrize("name", sorted(EXISTING_HASHES))
def test_existing_scene_arrays_are_unchanged(name):
    s = scenes_module().make_scene(name, 96, 80, seed=3)
    h = hashlib.sha256()
    for a in (s.frame_0, s.frame_1, s.gt_u, s.gt_v) + ((s.occlusion,) if s.occlusion is not None else ()):
        h.update(np.round(a.astype(np.float64), 2).tobytes())
    assert h.hexdigest() == EXISTING_HASHES[name]
