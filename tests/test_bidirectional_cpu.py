"""Bidirectional flow and forward-backward occlusion masks, the parts that need no device: the new entries are exported,
flow2d_consistency_2d refuses bad arguments before it touches the device, and the numpy restatement of the mask's definition
(include/flow2d_c_abi.h, flow2d_consistency_2d) -- the checker of tests/test_gpu_bidirectional.py -- gives hand-computed answers."""
import ctypes

import numpy as np
import pytest

F32 = np.float32
ALPHA1, ALPHA2 = 0.01, 0.5


def consistency_reference(u0, v0, u1, v1, alpha1=ALPHA1, alpha2=ALPHA2):
    """The mask of flow2d_consistency_2d, operation for operation in fp32: 1.0 where (u0, v0) and (u1, v1) sampled at the
    pixel the forward vector points to are inconsistent, leave the frame or involve a NaN; 0.0 elsewhere."""
    u0, v0, u1, v1 = (np.asarray(a, F32) for a in (u0, v0, u1, v1))
    h, w = u0.shape
    ys, xs = np.mgrid[0:h, 0:w]
    xf = xs.astype(F32) + u0
    yf = ys.astype(F32) + v0
    with np.errstate(invalid="ignore"):
        inside = (xf >= F32(0)) & (xf <= F32(w - 1)) & (yf >= F32(0)) & (yf <= F32(h - 1))
    xf, yf = np.where(inside, xf, F32(0)), np.where(inside, yf, F32(0))
    xi, yi = np.floor(xf).astype(np.int64), np.floor(yf).astype(np.int64)
    dx, dy = xf - xi.astype(F32), yf - yi.astype(F32)
    x1, y1 = np.minimum(w - 1, xi + 1), np.minimum(h - 1, yi + 1)
    one = F32(1)

    def sample(p):
        return ((one - dx) * (one - dy) * p[yi, xi] + dx * (one - dy) * p[yi, x1] + (one - dx) * dy * p[y1, xi] +
                dx * dy * p[y1, x1])

    with np.errstate(invalid="ignore", over="ignore"):
        bu, bv = sample(u1), sample(v1)
        eu, ev = u0 + bu, v0 + bv
        lhs = eu * eu + ev * ev
        rhs = F32(alpha1) * ((u0 * u0 + v0 * v0) + (bu * bu + bv * bv)) + F32(alpha2)
        consistent = inside & (lhs <= rhs)
    return np.where(consistent, F32(0), F32(1)).astype(F32)


def zeros(h, w):
    return np.zeros((h, w), F32)


def test_new_entries_are_exported(flow2d):
    assert hasattr(flow2d.hip_lib(), "flow2d_consistency_2d")
    host = flow2d.host_lib()
    assert hasattr(host, "flow2d_host_compute_flow_bidirectional")
    assert hasattr(host, "flow2d_host_compute_flow_bidirectional_device")
    assert hasattr(flow2d.Context, "consistency")
    assert hasattr(flow2d.OpticalFlow, "compute_flow_bidirectional")
    assert hasattr(flow2d.OpticalFlow, "compute_flow_bidirectional_device")
    assert flow2d.hip_lib().flow2d_abi_version() == 1  # an addition: the version stays


def test_consistency_rejects_bad_arguments_without_a_device(flow2d):
    """Every refusal below happens before the context is touched: the context is a zeroed stand-in and the planes are
    16-byte aligned addresses nothing reads."""
    lib = flow2d.hip_lib()
    fake_ctx = ctypes.create_string_buffer(4096)
    ctx = ctypes.addressof(fake_ctx)
    w, h, pitch = 64, 8, 256
    u, v, bu, bv, m = (0x1000000 * (k + 1) for k in range(5))

    def call(ctx=ctx, u=u, v=v, bu=bu, bv=bv, w=w, h=h, pitch=pitch, a1=ALPHA1, a2=ALPHA2, m=m):
        return lib.flow2d_consistency_2d(ctx, u, v, bu, bv, w, h, pitch, a1, a2, m)

    assert call(ctx=None) == 1
    for plane in ("u", "v", "bu", "bv", "m"):
        assert call(**{plane: None}) == 1, plane
    assert call(w=0) == 1 and call(h=0) == 1
    assert call(pitch=8) == 1  # narrower than a row
    for a1, a2 in ((-0.01, 0.5), (0.01, -0.5), (float("nan"), 0.5), (0.01, float("nan")), (float("inf"), 0.5)):
        assert call(a1=a1, a2=a2) == 1, (a1, a2)
    # the mask's byte range [m, m + h * pitch) against every input's: overlapping regions at different base pointers
    assert call(m=u + pitch) == 1               # starts inside u
    assert call(m=bv - pitch) == 1              # ends inside bv
    assert call(m=v + (h - 1) * pitch) == 1     # shares v's last row only
    if flow2d.device_count() == 0:
        # arguments that pass every check reach the device guard: no device here, so a device error -- not a refusal
        assert call(m=u + h * pitch) == 3
        assert call(m=u - h * pitch) == 3


def test_reference_opposite_translations_are_consistent():
    """u0 = +1, u1 = -1: the backward vector at x + 1 cancels the forward one; the last column points out of the frame."""
    h, w = 4, 5
    u0, u1 = np.full((h, w), 1, F32), np.full((h, w), -1, F32)
    want = zeros(h, w)
    want[:, w - 1] = 1
    assert np.array_equal(consistency_reference(u0, zeros(h, w), u1, zeros(h, w)), want)
    # the same vertically
    v0, v1 = np.full((h, w), -2, F32), np.full((h, w), 2, F32)
    want = zeros(h, w)
    want[:2, :] = 1
    assert np.array_equal(consistency_reference(zeros(h, w), v0, zeros(h, w), v1), want)


def test_reference_threshold():
    """|u0 + bu|^2 against 0.01 (|u0|^2 + |bu|^2) + 0.5: (2, -1) -> 1 > 0.55 inconsistent; (2, -1.5) -> 0.25 <= 0.5625."""
    h, w = 1, 4
    u0 = np.array([[2, 0, 0, 0]], F32)
    assert consistency_reference(u0, zeros(h, w), np.full((h, w), -1, F32), zeros(h, w))[0, 0] == 1
    assert consistency_reference(u0, zeros(h, w), np.full((h, w), -1.5, F32), zeros(h, w))[0, 0] == 0
    # larger tolerances: the same pair passes with alpha2 = 1
    assert consistency_reference(u0, zeros(h, w), np.full((h, w), -1, F32), zeros(h, w), alpha2=1.0)[0, 0] == 0


def test_reference_vectors_leaving_the_frame():
    h, w = 3, 4
    u0, v0 = zeros(h, w), zeros(h, w)
    u0[0, 1] = -3.0       # x = 1 - 3 < 0
    v0[2, 2] = 0.5        # y = 2.5 > h - 1
    u0[1, 3] = 1e-6       # x just beyond w - 1
    want = zeros(h, w)
    want[0, 1] = want[2, 2] = want[1, 3] = 1
    assert np.array_equal(consistency_reference(u0, v0, zeros(h, w), zeros(h, w)), want)


def test_reference_nan():
    """A NaN forward vector fails the range test; a NaN in the backward flow poisons every sample whose 2 x 2 cell holds it,
    even at weight 0 (NaN * 0 = NaN)."""
    h, w = 4, 5
    u0, u1 = zeros(h, w), zeros(h, w)
    u0[0, 3] = np.nan
    u1[1, 2] = np.nan
    want = zeros(h, w)
    want[0, 3] = 1
    for y, x in ((1, 2), (1, 1), (0, 2), (0, 1)):  # the zero-flow pixels whose cell [y, y + 1] x [x, x + 1] holds (1, 2)
        want[y, x] = 1
    assert np.array_equal(consistency_reference(u0, zeros(h, w), u1, zeros(h, w)), want)


def test_reference_sample_exactly_on_the_last_column_and_row():
    """xf == w - 1 and yf == h - 1 are inside; the cell is clamped to the last column / row."""
    h, w = 3, 4
    u0, v0, u1, v1 = zeros(h, w), zeros(h, w), zeros(h, w), zeros(h, w)
    u0[0, 0], v0[0, 0] = 3.0, 2.0          # lands on (3, 2) exactly
    u1[2, 3], v1[2, 3] = -3.0, -2.0        # ... where the backward vector returns
    u0[1, 0] = 3.0                          # lands on (3, 1): samples u1[1, 3] = 0 -> |3|^2 > 0.01 * 9 + 0.5
    m = consistency_reference(u0, v0, u1, v1)
    assert m[0, 0] == 0 and m[1, 0] == 1
    # the pixel (3, 2) itself: zero flow, samples (-3, -2) at weight 1 -> inconsistent
    assert m[2, 3] == 1
    # bilinear weights: u0 = 0.5 samples halfway between u1 columns 1 and 2
    u0, u1 = zeros(1, 4), np.array([[0, -0.25, -0.75, 0]], F32)
    u0[0, 1] = 0.5
    assert consistency_reference(u0, zeros(1, 4), u1, zeros(1, 4))[0, 1] == 0  # bu = -0.5 exactly: eu = 0
    u1[0, 2] = np.nan
    assert consistency_reference(u0, zeros(1, 4), u1, zeros(1, 4))[0, 1] == 1


@pytest.mark.parametrize("seed", [0, 1])
def test_reference_is_symmetric_for_exact_inverses(seed):
    """Integer translations that are exact inverses: consistent wherever the forward vector stays inside."""
    rng = np.random.default_rng(seed)
    h, w = 9, 11
    dx, dy = (int(t) for t in rng.integers(-3, 4, 2))
    u0, v0 = np.full((h, w), dx, F32), np.full((h, w), dy, F32)
    m = consistency_reference(u0, v0, -u0, -v0)
    ys, xs = np.mgrid[0:h, 0:w]
    inside = (xs + dx >= 0) & (xs + dx <= w - 1) & (ys + dy >= 0) & (ys + dy <= h - 1)
    assert np.array_equal(m, np.where(inside, 0, 1).astype(F32))
