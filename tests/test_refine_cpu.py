"""flow2d_refine_flow_2d restated in numpy from the text of include/flow2d_c_abi.h (np.float32 operations in the stated order,
integer weights), and what can be checked without a device: the properties of the definition, the accuracy and noise
conditions on `two_layer`, and the entry's host-side refusals."""
import ctypes
import importlib

import numpy as np
import pytest

F32 = np.float32
U32 = np.uint32
RECORD_DTYPE = np.dtype([("pixels", "<u8"), ("unfilled", "<u8"), ("filled", "<u8"), ("changed", "<u8")])
assert RECORD_DTYPE.itemsize == 32
SENTINEL = F32(1.666666752e9)  # the unknown-flow value of .flo files: above the 1e9 limit
ONE, ZERO = F32(1), F32(0)


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def shifted(a, dx, dy):
    """a[y + dy, x + dx] with the indices clamped into the frame, and whether (x + dx, y + dy) lies inside it."""
    h, w = a.shape
    ys, xs = np.arange(h) + dy, np.arange(w) + dx
    inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
    return a[np.clip(ys, 0, h - 1)[:, None], np.clip(xs, 0, w - 1)[None, :]], inside


def window_weights(u, v, guide, mask, r, sigma_guide, sigma_space):
    """(values_u, values_v, q) as [(2r+1)^2, h, w] arrays: the samples of every pixel's window and their integer weights, in the
    order and the arithmetic of the definition.  A sample that takes no part has q = 0 and the value 0."""
    u, v = np.ascontiguousarray(u, F32), np.ascontiguousarray(v, F32)
    with np.errstate(invalid="ignore"):
        usable = (np.abs(u) <= F32(1e9)) & (np.abs(v) <= F32(1e9))
    if mask is None:
        base = np.ones(u.shape, F32)
    else:
        m = np.array(mask, F32)
        m[~(m <= 1)] = 1
        m[~(m >= 0)] = 0
        base = ONE - m
    use_guide = guide is not None and sigma_guide > 0
    sg2 = F32(sigma_guide) * F32(sigma_guide)
    ss2 = F32(sigma_space) * F32(sigma_space)
    vu, vv, qs = [], [], []
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                su, inside = shifted(u, dx, dy)
                sv, _ = shifted(v, dx, dy)
                part = inside & shifted(usable, dx, dy)[0]
                wgt = shifted(base, dx, dy)[0].copy()
                if use_guide:
                    g = np.ascontiguousarray(guide, F32)
                    d = (shifted(g, dx, dy)[0] - g).astype(F32)
                    wgt = ((wgt * sg2).astype(F32) / (sg2 + (d * d).astype(F32)).astype(F32)).astype(F32)
                if sigma_space > 0:
                    wgt = ((wgt * ss2).astype(F32) / F32(ss2 + F32(dx * dx + dy * dy))).astype(F32)
                scaled = np.floor((F32(4096) * wgt).astype(F32))
                q = np.where(np.isfinite(wgt) & part, scaled, 0).astype(np.int64)
                assert q.min() >= 0 and q.max() <= 4096
                vu.append(np.where(q > 0, su, ZERO))
                vv.append(np.where(q > 0, sv, ZERO))
                qs.append(q)
    return np.stack(vu), np.stack(vv), np.stack(qs)


def weighted_median(values, q, total):
    """Per pixel the smallest value x_k with q > 0 such that twice the weight of the samples <= x_k is at least `total`."""
    order = np.argsort(values, axis=0, kind="stable")
    sv = np.take_along_axis(values, order, 0)
    cum = np.cumsum(np.take_along_axis(q, order, 0), axis=0)
    first = np.argmax(2 * cum >= total[None], axis=0)  # (total = 0: index 0, replaced by the caller)
    return np.take_along_axis(sv, first[None], 0)[0]


def refine_reference(u, v, guide=None, mask=None, r=1, sigma_guide=0.0, sigma_space=0.0):
    """(u_out, v_out, record): the definition of flow2d_refine_flow_2d; record is one RECORD_DTYPE entry."""
    assert 1 <= r <= 7 and sigma_guide >= 0 and sigma_space >= 0
    u, v = np.ascontiguousarray(u, F32), np.ascontiguousarray(v, F32)
    vu, vv, q = window_weights(u, v, guide, mask, r, sigma_guide, sigma_space)
    total = q.sum(axis=0)
    out = []
    for values, plane in ((vu, u), (vv, v)):
        med = weighted_median(values, q, total) + ZERO  # -0 + 0 = +0
        out.append(np.where(total > 0, med, plane).astype(F32))
    record = np.zeros(1, RECORD_DTYPE)
    record["pixels"] = u.size
    record["unfilled"] = int((total == 0).sum())
    if mask is not None:
        m = np.array(mask, F32)
        m[~(m <= 1)] = 1
        m[~(m >= 0)] = 0
        record["filled"] = int(((m >= F32(0.5)) & (total > 0)).sum())
    record["changed"] = int(((bits(out[0]) != bits(u)) | (bits(out[1]) != bits(v))).sum())
    return out[0], out[1], record


def refine_passes(u, v, guide, mask, r, sigma_guide, sigma_space, iterations):
    record = None
    for _ in range(iterations):
        u, v, record = refine_reference(u, v, guide, mask, r, sigma_guide, sigma_space)
    return u, v, record


def random_case(w, h, seed=3, wild=True, soft=True):
    """A random flow, guide and mask: NaN, infinite and sentinel vectors, mask values outside [0, 1] and NaN, a NaN in the guide."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    u = (rng.standard_normal((h, w)) * 3).astype(F32)
    v = (rng.standard_normal((h, w)) * 3).astype(F32)
    guide = (rng.random((h, w)) * 255).astype(F32)
    r = rng.random((h, w))
    mask = np.where(r < 0.3, 0.5 + 0.5 * rng.random((h, w)), 0.4999 * rng.random((h, w))).astype(F32) if soft else (r < 0.3).astype(F32)
    if wild:
        t = rng.random((h, w))
        u[t < 0.02] = np.nan
        v[(t >= 0.02) & (t < 0.04)] = np.inf
        u[(t >= 0.04) & (t < 0.05)] = -np.inf
        v[(t >= 0.05) & (t < 0.06)] = SENTINEL
        u[(t >= 0.06) & (t < 0.07)] = -0.0
        odd = rng.random((h, w))
        mask[odd < 0.03] = np.nan
        mask[(odd >= 0.03) & (odd < 0.06)] = -2.0
        mask[(odd >= 0.06) & (odd < 0.09)] = 7.0
        guide[rng.random((h, w)) < 0.01] = np.nan
    return u, v, guide, mask


def epe(u, v, scene, where=None):
    e = np.hypot(u.astype(np.float64) - scene.gt_u, v.astype(np.float64) - scene.gt_v)
    return float(e.mean() if where is None else e[where].mean())


@pytest.fixture(scope="module")
def two_layer():
    return importlib.import_module("cuda-flow2d_amd.scenes").make_scene("two_layer", 256, 256, seed=0)


# ---- properties of the definition --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 4, 7])
def test_constant_flow_is_unchanged(r):
    u, v = np.full((9, 13), 2.5, F32), np.full((9, 13), -1.25, F32)
    _, _, guide, mask = random_case(13, 9, wild=False)
    for g, m, sg, ss in ((None, None, 0.0, 0.0), (guide, None, 10.0, 0.0), (guide, mask * F32(0.9), 10.0, 3.0)):
        ou, ov, rec = refine_reference(u, v, g, m, r, sg, ss)
        assert np.array_equal(bits(ou), bits(u)) and np.array_equal(bits(ov), bits(v))
        assert rec["pixels"][0] == 117 and rec["unfilled"][0] == 0 and rec["changed"][0] == 0


@pytest.mark.parametrize("r", [1, 2, 3])
def test_without_weights_it_is_the_plain_lower_median(r):
    w, h = 11, 8
    u, v, _, _ = random_case(w, h, wild=False)
    ou, ov, _ = refine_reference(u, v, None, None, r)
    for plane, got in ((u, ou), (v, ov)):
        for y in range(h):
            for x in range(w):
                win = np.sort(plane[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1].ravel())
                assert got[y, x] == win[(win.size - 1) // 2], (x, y)
    if r == 1:
        win = np.lib.stride_tricks.sliding_window_view(u, (3, 3)).reshape(h - 2, w - 2, 9)
        assert np.array_equal(ou[1:-1, 1:-1], np.median(win, axis=2))


def test_a_single_outlier_is_removed():
    y, x = np.mgrid[0:15, 0:15].astype(F32)
    u, v = F32(0.125) * x, F32(0.25) * y
    u2, v2 = u.copy(), v.copy()
    u2[7, 7], v2[7, 7] = 40.0, -40.0
    ou, ov, rec = refine_reference(u2, v2, None, None, 2)
    assert ou[7, 7] == u[7, 7] and ov[7, 7] == v[7, 7]
    clean = refine_reference(u, v, None, None, 2)
    assert np.abs(ou - clean[0]).max() <= 0.125 and np.abs(ov - clean[1]).max() <= 0.25


def test_nothing_usable_copies_the_input_bits():
    u, v, guide, _ = random_case(7, 5)
    ou, ov, rec = refine_reference(u, v, guide, np.ones_like(u), 3, 5.0, 2.0)
    assert np.array_equal(bits(ou), bits(u)) and np.array_equal(bits(ov), bits(v))
    assert rec["unfilled"][0] == 35 and rec["filled"][0] == 0 and rec["changed"][0] == 0
    # a usable vector in reach fills its whole window, the masked centre included
    mask = np.ones((5, 7), F32)
    mask[2, 3] = 0
    u[2, 3], v[2, 3] = 1.5, -2.5
    ou, ov, rec = refine_reference(u, v, None, mask, 1)
    assert (ou[1:4, 2:5] == 1.5).all() and (ov[1:4, 2:5] == -2.5).all()
    assert rec["unfilled"][0] == 35 - 9 and rec["filled"][0] == 8


def test_negative_zero_comes_out_positive():
    u = np.full((3, 3), -0.0, F32)
    v = np.zeros((3, 3), F32)
    ou, ov, rec = refine_reference(u, v, None, None, 1)
    assert (bits(ou) == 0).all() and (bits(ov) == 0).all() and rec["changed"][0] == 9
    # ... but a copied vector keeps its sign bit
    ou, _, rec = refine_reference(u, v, None, np.ones_like(u), 1)
    assert (bits(ou) == 0x80000000).all() and rec["changed"][0] == 0


@pytest.mark.parametrize("r", [1, 5])
def test_record_counts_add_up(r):
    w, h = 23, 17
    u, v, guide, mask = random_case(w, h)
    ou, ov, rec = refine_reference(u, v, guide, mask, r, 20.0, 4.0)
    rec = rec[0]
    assert rec["pixels"] == w * h and rec["unfilled"] + rec["filled"] <= rec["pixels"] and rec["changed"] <= rec["pixels"] - rec["unfilled"]
    assert rec["filled"] > 0 and rec["changed"] > 0
    # every output is a finite input value of its window (or the copied input)
    assert np.isfinite(ou[np.isfinite(u)]).all()
    assert set(np.unique(ou[np.isfinite(ou)])) <= set(np.unique(u[np.isfinite(u)])) | {F32(0)}


def test_wild_mask_values_clamp():
    u, v, _, _ = random_case(9, 9, wild=False)
    mask = np.zeros((9, 9), F32)
    mask[4, 4], mask[4, 5], mask[5, 4] = np.nan, 7.0, -3.0
    want = mask.copy()
    want[4, 4], want[4, 5], want[5, 4] = 1, 1, 0
    a, b = refine_reference(u, v, None, mask, 2), refine_reference(u, v, None, want, 2)
    assert np.array_equal(bits(a[0]), bits(b[0])) and a[2].tobytes() == b[2].tobytes()


# ---- the conditions of the issue, on two_layer at 256 x 256 -------------------------------------------------------------------
def test_occlusion_fill_in(two_layer):
    """The true flow with the 438 occluded pixels set to the square's motion; mask = the true occlusion, guide = frame 0, r = 5,
    sigma_guide = 25, one pass.  Measured with this restatement: EPE over the occluded pixels 5.031 -> 1.574 (3.94 without the
    mask), over all pixels 0.0336 -> 0.0147."""
    sc = two_layer
    occ = sc.occlusion > 0
    assert int(occ.sum()) == 438
    u, v = sc.gt_u.copy(), sc.gt_v.copy()
    u[occ], v[occ] = 4.5, -2.25
    ou, ov, rec = refine_reference(u, v, sc.frame_0, sc.occlusion, 5, 25.0)
    nu, nv, _ = refine_reference(u, v, sc.frame_0, None, 5, 25.0)
    before = epe(u, v, sc, occ), epe(u, v, sc)
    after = epe(ou, ov, sc, occ), epe(ou, ov, sc)
    unmasked = epe(nu, nv, sc, occ)
    print("occluded EPE %.4f -> %.4f (unmasked %.4f), all pixels %.5f -> %.5f" % (before[0], after[0], unmasked, before[1], after[1]))
    assert after[0] <= 0.5 * before[0]
    assert after[1] < before[1]
    assert after[0] < unmasked
    assert rec["filled"][0] + rec["unfilled"][0] == 438


def test_noise_removal(two_layer):
    """The true flow plus Gaussian noise of 0.5 px, no mask, r = 5, guide sigma 25: measured 0.625 -> 0.087 over all pixels."""
    sc = two_layer
    rng = np.random.default_rng(1)
    u = (sc.gt_u + 0.5 * rng.standard_normal(sc.gt_u.shape)).astype(F32)
    v = (sc.gt_v + 0.5 * rng.standard_normal(sc.gt_v.shape)).astype(F32)
    ou, ov, _ = refine_reference(u, v, sc.frame_0, None, 5, 25.0)
    before, after = epe(u, v, sc), epe(ou, ov, sc)
    print("all-pixel EPE %.4f -> %.4f" % (before, after))
    assert after < before / 3


# ---- the entry's host side ----------------------------------------------------------------------------------------------------
def test_refusals_without_a_device(flow2d):
    lib = flow2d.hip_lib()
    assert hasattr(lib, "flow2d_refine_flow_2d")
    fake = ctypes.create_string_buffer(4096)
    w, h, pitch = 100, 40, 512
    span = pitch * h
    at = lambda k: (1 << 20) + k * (span + 4096)  # noqa: E731  (addresses only: nothing is dereferenced before the device is entered)
    d = dict(ctx=ctypes.addressof(fake), u=at(0), v=at(1), guide=at(2), mask=at(3), w=w, h=h, pitch=pitch, r=3, sg=10.0, ss=2.0,
             ou=at(4), ov=at(5), record=at(6))

    def call(**kw):
        a = dict(d, **kw)
        return lib.flow2d_refine_flow_2d(a["ctx"], a["u"], a["v"], a["guide"], a["mask"], a["w"], a["h"], a["pitch"], a["r"], a["sg"],
                                         a["ss"], a["ou"], a["ov"], a["record"])

    nan = float("nan")
    bad = [dict(ctx=None), dict(u=None), dict(v=None), dict(ou=None), dict(ov=None), dict(w=0), dict(h=0), dict(pitch=pitch + 8),
           dict(pitch=396), dict(r=0), dict(r=8), dict(r=-1), dict(sg=-1.0), dict(ss=-0.5), dict(sg=nan), dict(ss=nan),
           dict(sg=float("inf")), dict(u=at(0) + 4), dict(guide=at(2) + 8), dict(mask=at(3) + 4), dict(ou=at(4) + 4), dict(record=at(6) + 4),
           dict(ou=at(0)), dict(ov=at(1) + pitch), dict(ou=at(2)), dict(ov=at(3) + span - pitch), dict(ou=at(5)), dict(record=at(0) + 64),
           dict(record=at(4) + 8)]
    for kw in bad:
        assert call(**kw) == 1, kw
    # (only refusals here: an accepted call would go on to launch on these made-up addresses where there is a device)


def test_python_record_matches_the_restatement_layout(flow2d):
    rec = flow2d.RefineRecord()
    rec.pixels, rec.unfilled, rec.filled, rec.changed = 9, 1, 2, 3
    a = np.frombuffer(bytes(rec), RECORD_DTYPE)[0]
    assert (a["pixels"], a["unfilled"], a["filled"], a["changed"]) == (9, 1, 2, 3)
    assert ctypes.sizeof(flow2d.RefineRecord) == flow2d.REFINE_RECORD_BYTES == 32
    H = flow2d.host_lib()
    assert H.flow2d_host_refine_args_ok(1, 0.0, 0.0, 1) == 1 and H.flow2d_host_refine_args_ok(7, 25.0, 3.0, 16) == 1
    for r, sg, ss, k in ((0, 1.0, 1.0, 1), (8, 1.0, 1.0, 1), (3, -1.0, 0.0, 1), (3, 0.0, -1.0, 1), (3, float("nan"), 0.0, 1),
                         (3, 1.0, 1.0, 0), (3, 1.0, 1.0, 17)):
        assert H.flow2d_host_refine_args_ok(r, sg, ss, k) == 0, (r, sg, ss, k)
