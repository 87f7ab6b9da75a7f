"""flow2d_correlate_offset_2d and flow2d_validate_nodes_2d restated in numpy from the text of include/flow2d_c_abi.h -- node by node:
the search area around the node's offset cut out of frame 1, exact integer sums, the score in float64; the median test in
np.float32 operations in the stated order --, the chain of OpticalFlow2D::CorrelateMultiPass built from them, and what can be
checked without a device: the restatement against flow2d_correlate_2d's (an independent formulation: summed-area tables over the
whole frame), the predictor's edge values, the median's definition, the test's outcomes, the accuracy on noisy speckle scenes and
the entries' host-side refusals."""
import ctypes

import numpy as np
import pytest

from test_correlate_cpu import (F32, I64, NAN_BITS, U32, bits, correlate_reference, expand_reference, frame_range, grid, quantise,
                                random_frames, scenes_module)

PASS_DTYPE = np.dtype([("nodes", "<u8"), ("invalid", "<u8"), ("rejected", "<u8"), ("unrefined", "<u8"), ("unpredicted", "<u8"),
                       ("candidates", "<u8"), ("reserved", "<u8", (2,))])
VALIDATION_DTYPE = np.dtype([("nodes", "<u8"), ("judged", "<u8"), ("outliers", "<u8"), ("filled", "<u8"), ("unjudged", "<u8"),
                             ("remaining_invalid", "<u8"), ("reserved", "<u8", (2,))])
assert PASS_DTYPE.itemsize == 64 and VALIDATION_DTYPE.itemsize == 64
FLAG, REPLACE = 0, 1
MAX_PASSES = 6


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def word(x):
    """The bits of one float."""
    return bits(x).ravel()[0]


def node_offsets(pred_u, pred_v, w, h, r, s):
    """(ox, oy, unpredicted) per node: the header's rounding of the predictor at the node centres."""
    nw, nh = grid(w, h, r, s)
    if pred_u is None:
        zero = np.zeros((nh, nw), I64)
        return zero, zero.copy(), np.zeros((nh, nw), bool)
    cy, cx = r + np.arange(nh) * s, r + np.arange(nw) * s
    pu, pv = np.asarray(pred_u, F32)[np.ix_(cy, cx)], np.asarray(pred_v, F32)[np.ix_(cy, cx)]
    ok = np.isfinite(pu) & np.isfinite(pv)

    def rounded(p):
        p = np.where(ok, p, F32(0))
        t = np.minimum(np.maximum(p, F32(-32768)), F32(32768)) + F32(0.5)
        assert t.dtype == F32
        return np.floor(t).astype(I64)

    return rounded(pu), rounded(pv), ~ok


def correlate_offset_reference(frame_0, frame_1, lo, scale, r, d, s, min_score=-1.0, pred_u=None, pred_v=None):
    """(u, v, score, record) of flow2d_correlate_offset_2d."""
    q0, q1 = quantise(frame_0, lo, scale), quantise(frame_1, lo, scale)
    h, w = q0.shape
    side, n, reach = 2 * r + 1, (2 * r + 1) ** 2, 2 * d + 1
    nw, nh = grid(w, h, r, s)
    ox, oy, unpredicted = node_offsets(pred_u, pred_v, w, h, r, s)
    u, v = np.full((nh, nw), NAN_BITS, U32), np.full((nh, nw), NAN_BITS, U32)
    score = np.zeros((nh, nw), F32)
    record = np.zeros(1, PASS_DTYPE)
    record["nodes"], record["unpredicted"] = nh * nw, unpredicted.sum()
    dy_of, dx_of = np.mgrid[-d:d + 1, -d:d + 1]
    order = (dx_of * dx_of + dy_of * dy_of) * 10000 + (dy_of + d) * 100 + (dx_of + d)  # the smaller, the more preferred
    for j in range(nh):
        for i in range(nw):
            left, top = i * s, j * s
            a = q0[top:top + side, left:left + side]
            s0, s00 = a.sum(), (a * a).sum()
            v0 = n * s00 - s0 * s0
            if v0 <= 0:
                record["invalid"] += 1
                continue
            # the search area around the offset, 0 outside frame 1
            x1, y1 = left + int(ox[j, i]) - d, top + int(oy[j, i]) - d
            area = np.zeros((side + 2 * d, side + 2 * d), I64)
            xa, xb, ya, yb = max(x1, 0), min(x1 + side + 2 * d, w), max(y1, 0), min(y1 + side + 2 * d, h)
            if xa < xb and ya < yb:
                area[ya - y1:yb - y1, xa - x1:xb - x1] = q1[ya:yb, xa:xb]
            windows = np.lib.stride_tricks.sliding_window_view(area, (side, side))  # [dy + d, dx + d, wy, wx]
            s1, s11 = windows.sum((2, 3)), (windows * windows).sum((2, 3))
            s01 = np.einsum("ijkl,kl->ij", windows, a)
            v1 = n * s11 - s1 * s1
            lx, ly = x1 + d + dx_of, y1 + d + dy_of
            cand = (lx >= 0) & (ly >= 0) & (lx + side <= w) & (ly + side <= h) & (v1 > 0)
            record["candidates"] += np.uint64(int(cand.sum()))
            if not cand.any():
                record["invalid"] += 1
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                c = (n * s01 - s0 * s1).astype(np.float64) / np.sqrt(np.float64(v0) * v1.astype(np.float64))
            c = np.where(cand, c, -np.inf)
            best = c.max()
            tie = np.where(c == best, order, np.iinfo(np.int64).max)
            ky, kx = np.unravel_index(np.argmin(tie), tie.shape)
            bx, by = kx - d, ky - d
            refined = abs(bx) < d and abs(by) < d and cand[ky, kx - 1] and cand[ky, kx + 1] and cand[ky - 1, kx] and cand[ky + 1, kx]
            delta_x = delta_y = 0.0
            if refined:
                den_x, den_y = (c[ky, kx - 1] - 2.0 * best) + c[ky, kx + 1], (c[ky - 1, kx] - 2.0 * best) + c[ky + 1, kx]
                delta_x = (c[ky, kx - 1] - c[ky, kx + 1]) / (2.0 * den_x) if den_x < 0 else 0.0
                delta_y = (c[ky - 1, kx] - c[ky + 1, kx]) / (2.0 * den_y) if den_y < 0 else 0.0
            score[j, i] = F32(best)
            if score[j, i] < F32(min_score):
                record["rejected"] += 1
                continue
            u[j, i] = word(F32(np.float64(int(ox[j, i]) + bx) + delta_x))
            v[j, i] = word(F32(np.float64(int(oy[j, i]) + by) + delta_y))
            record["unrefined"] += np.uint64(not refined)
    return u.view(F32), v.view(F32), score, record


def float_key(x):
    """The order-preserving integer key of the header (-0 < +0)."""
    b = np.asarray(x, F32).view(np.int32).astype(I64)
    return np.where(b < 0, b ^ 0x7FFFFFFF, b)


def median(values):
    """The header's median of k >= 1 floats."""
    a = np.asarray(values, F32)
    a = a[np.argsort(float_key(a), kind="stable")]
    k = a.size
    with np.errstate(over="ignore"):
        return F32(F32(a[(k - 1) // 2] + a[k // 2]) * F32(0.5))


def validate_reference(node_u, node_v, threshold=2.0, epsilon=0.1, min_neighbours=3, mode=REPLACE):
    """(u, v, flag, record) of flow2d_validate_nodes_2d."""
    node_u, node_v = np.ascontiguousarray(node_u, F32), np.ascontiguousarray(node_v, F32)
    nh, nw = node_u.shape
    out_u, out_v = bits(node_u).copy(), bits(node_v).copy()
    flag = np.zeros((nh, nw), F32)
    valid = np.isfinite(node_u) & np.isfinite(node_v)
    record = np.zeros(1, VALIDATION_DTYPE)
    record["nodes"] = nh * nw
    threshold, epsilon = F32(threshold), F32(epsilon)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(nh):
            for i in range(nw):
                ring = [(y, x) for y in (j - 1, j, j + 1) for x in (i - 1, i, i + 1)
                        if (y, x) != (j, i) and 0 <= y < nh and 0 <= x < nw and valid[y, x]]
                if len(ring) < min_neighbours:
                    record["unjudged"] += 1
                    continue
                nu, nv = np.array([node_u[p] for p in ring], F32), np.array([node_v[p] for p in ring], F32)
                mu, mv = median(nu), median(nv)
                if valid[j, i]:
                    record["judged"] += 1
                    ru, rv = median(np.abs(nu - mu)), median(np.abs(nv - mv))
                    tu = np.abs(node_u[j, i] - mu) / F32(ru + epsilon)
                    tv = np.abs(node_v[j, i] - mv) / F32(rv + epsilon)
                    if tu > threshold or tv > threshold:
                        record["outliers"] += 1
                        flag[j, i] = 1
                        out_u[j, i], out_v[j, i] = (word(mu), word(mv)) if mode == REPLACE else (NAN_BITS, NAN_BITS)
                elif mode == REPLACE:
                    record["filled"] += 1
                    flag[j, i] = 2
                    out_u[j, i], out_v[j, i] = word(mu), word(mv)
    out_u, out_v = out_u.view(F32), out_v.view(F32)
    record["remaining_invalid"] = (~(np.isfinite(out_u) & np.isfinite(out_v))).sum()
    return out_u, out_v, flag, record


def multipass_reference(frame_0, frame_1, lo, scale, passes, min_score=-1.0, threshold=2.0, epsilon=0.1, min_neighbours=3, replace=True,
                        validate_last=True, predictor=None):
    """OpticalFlow2D::CorrelateMultiPass: per pass the offset search around the current predictor; between passes the median test
    in REPLACE mode and the expansion to the frame's grid, which is the next predictor; after the last pass the test in the
    caller's mode (validate_last).  Returns (node_u, node_v, score, reports, (dense u, dense v)); reports: per pass (nw, nh, pass
    record, validation record -- zeros where the pass was not validated)."""
    h, w = frame_0.shape
    pu, pv = predictor if predictor is not None else (None, None)
    reports = []
    for k, (r, d, s) in enumerate(passes):
        last = k == len(passes) - 1
        u, v, score, record = correlate_offset_reference(frame_0, frame_1, lo, scale, r, d, s, min_score, pu, pv)
        validation = np.zeros(1, VALIDATION_DTYPE)
        if not last or validate_last:
            u, v, _, validation = validate_reference(u, v, threshold, epsilon, min_neighbours, REPLACE if (not last or replace) else FLAG)
        pu, pv = expand_reference(u, v, r, s, w, h)
        reports.append((u.shape[1], u.shape[0], record, validation))
    return u, v, score, reports, (pu, pv)


# ---- flow2d_correlate_offset_2d ---------------------------------------------------------------------------------------------------
def same(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("w,h,r,d,s", [(40, 31, 3, 4, 5), (33, 29, 2, 6, 1), (29, 45, 7, 3, 8), (7, 7, 3, 5, 3)])
def test_null_and_zero_predictors_give_the_single_pass_bytes(w, h, r, d, s):
    f0, f1 = random_frames(w, h, seed=w)
    if w > 20:
        f0[5:14, 4:15] = 77.0  # invalid nodes, candidates with V1 = 0
        f1[0:9, 20:31] = 12.0
    cut = 0.4
    wu, wv, ws, wrec, _ = correlate_reference(f0, f1, 0.0, 1.0, r, d, s, cut)
    zero = np.zeros((h, w), F32)
    for pred in (None, (zero, zero), (zero - F32(0.0), zero + F32(0.49)), (zero - F32(0.5), zero)):
        u, v, score, rec = correlate_offset_reference(f0, f1, 0.0, 1.0, r, d, s, cut, *(pred or (None, None)))
        assert same(u, wu) and same(v, wv) and same(score, ws)
        assert [int(rec[k][0]) for k in ("nodes", "invalid", "rejected", "unrefined")] == [int(x) for x in wrec[0]]
        assert rec["unpredicted"][0] == 0 and rec["reserved"].sum() == 0
        assert 0 < rec["candidates"][0] <= rec["nodes"][0] * (2 * d + 1) ** 2


def test_predictor_edge_values():
    """NaN and +-inf in either component leave the node unpredicted at offset 0; +-1e30 is finite and clamps to +-32768, which
    pushes every candidate out of the frame: an invalid node.  Halves round up (floor(p + 0.5))."""
    w, h, r, d, s = 41, 23, 2, 2, 6
    f0, f1 = random_frames(w, h, seed=8)
    nw, nh = grid(w, h, r, s)
    base_u, base_v, base_s, _ = correlate_offset_reference(f0, f1, 0.0, 1.0, r, d, s)
    pu, pv = np.zeros((h, w), F32), np.zeros((h, w), F32)
    centre = lambda i, j: (r + j * s, r + i * s)  # noqa: E731
    pu[centre(0, 0)] = np.nan
    pv[centre(1, 0)] = np.inf
    pu[centre(2, 0)], pv[centre(2, 0)] = -np.inf, 1.0
    pu[centre(3, 1)] = 1e30
    pv[centre(4, 1)] = -1e30
    pu[centre(5, 2)], pv[centre(5, 2)] = 1.5, -1.5   # -> (2, -1)
    pu[centre(1, 2)], pv[centre(1, 2)] = 0.49999997, -0.50000006  # -> (1, -1): the sum with 0.5 is rounded to fp32 first
    # beside the centres nothing is read
    pu[r + 1, r], pv[r, r + 1] = 7.0, np.nan
    ox, oy, un = node_offsets(pu, pv, w, h, r, s)
    assert un.sum() == 3 and un[0, 0] and un[0, 1] and un[0, 2]
    assert ox[1, 3] == 32768 and oy[1, 4] == -32768 and (ox[2, 5], oy[2, 5]) == (2, -1) and (ox[2, 1], oy[2, 1]) == (1, -1)
    u, v, score, rec = correlate_offset_reference(f0, f1, 0.0, 1.0, r, d, s, -1.0, pu, pv)
    assert rec["unpredicted"][0] == 3 and rec["invalid"][0] == 2
    assert np.isnan(u[1, 3]) and np.isnan(u[1, 4]) and score[1, 3] == 0 and score[1, 4] == 0
    untouched = np.ones((nh, nw), bool)
    untouched[1, 3] = untouched[1, 4] = untouched[2, 5] = untouched[2, 1] = False
    assert same(u[untouched], base_u[untouched]) and same(v[untouched], base_v[untouched]) and same(score[untouched], base_s[untouched])
    assert abs(u[2, 5] - 2) <= d + 0.5 and abs(v[2, 5] + 1) <= d + 0.5


@pytest.mark.parametrize("shift", [(3, -2), (-5, 4), (0, 7)])
def test_constant_predictor_is_the_search_of_a_shifted_frame(shift):
    """A constant integer predictor (a, b): node by node the search around it is the unoffset search of frame 1 moved back by
    (a, b) -- g[y][x] = frame_1[y + b][x + a] -- plus (a, b), wherever every window either search looks at exists in both, i.e.
    the node's whole search area lies inside frame 1 and inside g's valid part."""
    w, h, r, d, s = 60, 50, 3, 3, 4
    a, b = shift
    f0, f1 = random_frames(w, h, seed=11, shift=(a + 1, b - 1))
    moved = np.full((h, w), 0.0, F32)
    ys, xs = slice(max(0, -b), min(h, h - b)), slice(max(0, -a), min(w, w - a))
    moved[ys, xs] = f1[ys.start + b:ys.stop + b, xs.start + a:xs.stop + a]
    pu, pv = np.full((h, w), a, F32), np.full((h, w), b, F32)
    u, v, score, rec = correlate_offset_reference(f0, f1, 0.0, 1.0, r, d, s, -1.0, pu, pv)
    wu, wv, ws, _, _ = correlate_reference(f0, moved, 0.0, 1.0, r, d, s)
    nw, nh = grid(w, h, r, s)
    cx, cy = r + np.arange(nw) * s, r + np.arange(nh) * s
    reach = r + d
    inside = ((cy - reach >= max(0, -b)) & (cy + reach < min(h, h - b)))[:, None] & ((cx - reach >= max(0, -a)) & (cx + reach < min(w, w - a)))[None, :]
    assert inside.sum() >= 20 and rec["unpredicted"][0] == 0
    # (the offset is added in double before the one rounding to float: equal to the shifted search's vector up to that rounding)
    assert np.abs(u[inside] - (wu[inside].astype(np.float64) + a)).max() < 1e-5 and np.abs(v[inside] - (wv[inside].astype(np.float64) + b)).max() < 1e-5
    assert np.array_equal(np.rint(u[inside] - a), np.rint(wu[inside])) and np.array_equal(np.rint(v[inside] - b), np.rint(wv[inside]))
    assert same(score[inside], ws[inside])
    assert np.median(np.rint(u[inside])) == a + 1 and np.median(np.rint(v[inside])) == b - 1


# ---- flow2d_validate_nodes_2d -------------------------------------------------------------------------------------------------------
def test_median_definition():
    assert float_key(F32(-0.0)) < float_key(F32(0.0)) and float_key(F32(-1.0)) < float_key(F32(-0.0)) < float_key(F32(1e-45))
    assert float_key(F32(-np.inf)) < float_key(F32(-3e38)) and float_key(F32(3e38)) < float_key(F32(np.inf))
    # odd k: the middle one, times two halves; with signed zeros the sign of the key's choice
    assert bits(median([F32(0.0), F32(-0.0), F32(-0.0)])) == bits(F32(-0.0))
    assert bits(median([F32(0.0), F32(-0.0), F32(0.0)])) == bits(F32(0.0))
    # even k: the mean of the two middle ones; -0 and +0 in the middle give +0
    assert bits(median([F32(-0.0), F32(0.0)])) == bits(F32(0.0)) and bits(median([F32(-0.0), F32(-0.0)])) == bits(F32(-0.0))
    assert median([F32(1), F32(5), F32(2), F32(4)]) == 3 and median([F32(7)]) == 7 and median([F32(3), F32(1), F32(2)]) == 2
    assert median(np.arange(8, 0, -1)) == 4.5 and median([F32(1), F32(2)]) == 1.5
    assert np.isinf(median([F32(3e38), F32(3e38)]))  # the sum is rounded before the half


def test_a_lone_spike_is_flagged_and_replaced():
    u = np.add.outer(np.arange(5) * 0.02, np.arange(6) * 0.01).astype(F32)  # (a gentle slope: epsilon covers it at the corners)
    v = (u * F32(-0.5)).astype(F32)
    u[2, 3] += 9
    for mode in (FLAG, REPLACE):
        ou, ov, flag, rec = validate_reference(u, v, mode=mode)
        assert flag[2, 3] == 1 and flag.sum() == 1 and rec["outliers"][0] == 1 and rec["judged"][0] == 30 and rec["filled"][0] == 0
        keep = flag == 0
        assert same(ou[keep], u[keep]) and same(ov[keep], v[keep])
        if mode == FLAG:
            assert bits(ou[2, 3]) == NAN_BITS and bits(ov[2, 3]) == NAN_BITS and rec["remaining_invalid"][0] == 1
        else:
            ring = [(y, x) for y in (1, 2, 3) for x in (2, 3, 4) if (y, x) != (2, 3)]
            assert ou[2, 3] == median([u[p] for p in ring]) and ov[2, 3] == median([v[p] for p in ring])
            assert rec["remaining_invalid"][0] == 0
    # v alone is enough
    u[2, 3] -= 9
    v[0, 0] -= 20
    assert validate_reference(u, v)[2].tolist()[0][0] == 1


def test_nan_nodes_are_filled_or_left():
    u = np.full((4, 5), 1.5, F32)
    v = np.full((4, 5), -2.0, F32)
    u[1, 1] = np.nan
    v[2, 3] = np.inf
    ou, ov, flag, rec = validate_reference(u, v, mode=REPLACE)
    assert flag[1, 1] == 2 and flag[2, 3] == 2 and ou[1, 1] == 1.5 and ov[2, 3] == -2 and ou[2, 3] == 1.5
    assert rec["filled"][0] == 2 and rec["remaining_invalid"][0] == 0 and rec["judged"][0] == 16 and rec["unjudged"][0] == 2 and rec["outliers"][0] == 0  # (two corners see k = 2)
    ou, ov, flag, rec = validate_reference(u, v, mode=FLAG)
    assert flag.sum() == 0 and same(ou, u) and same(ov, v) and rec["filled"][0] == 0 and rec["remaining_invalid"][0] == 2
    # an invalid node is no one's neighbour: a corner beside one has k = 2 < 3
    u2 = u.copy()
    u2[:, :] = 1.5
    u2[0, 1] = np.nan
    _, _, _, rec = validate_reference(u2, np.zeros_like(u2))
    assert rec["unjudged"][0] == 1 and rec["filled"][0] == 1


def test_too_few_neighbours_leave_the_node_untouched():
    u = np.array([[1.0, 100.0]], F32)
    ou, ov, flag, rec = validate_reference(u, u)  # 1 x 2: k = 1
    assert same(ou, u) and flag.sum() == 0 and rec["unjudged"][0] == 2 and rec["judged"][0] == 0
    ou, ov, flag, rec = validate_reference(u, u, min_neighbours=1)
    assert rec["judged"][0] == 2 and rec["outliers"][0] == 2 and ou[0, 0] == 100 and ou[0, 1] == 1  # each the other's median
    u = np.array([[1.0, 1.0], [1.0, 50.0]], F32)  # 2 x 2: k = 3
    ou, _, flag, rec = validate_reference(u, u)
    assert flag[1, 1] == 1 and ou[1, 1] == 1 and rec["judged"][0] == 4
    _, _, _, rec = validate_reference(u, u, min_neighbours=4)
    assert rec["unjudged"][0] == 4
    one = np.array([[np.nan]], F32)
    ou, _, flag, rec = validate_reference(one, one)
    assert bits(ou[0, 0]) == bits(one[0, 0]) and rec["unjudged"][0] == 1 and rec["remaining_invalid"][0] == 1


def test_an_all_nan_grid_stays():
    u = np.full((6, 7), np.nan, F32)
    u[2, 2] = -np.nan
    for mode in (FLAG, REPLACE):
        ou, ov, flag, rec = validate_reference(u, u, mode=mode)
        assert same(ou, u) and same(ov, u) and flag.sum() == 0
        assert [int(rec[k][0]) for k in rec.dtype.names[:6]] == [42, 0, 0, 0, 42, 42]


# ---- accuracy -----------------------------------------------------------------------------------------------------------------------
SCHEDULE = ((15, 12, 16), (7, 3, 8), (4, 2, 4))
SINGLE = (4, 12, 4)
BORDER = 28


def noisy_scene(motion, seed, sigma=30.0, width=160, height=128):
    sc = scenes_module().make_speckle_scene(motion, width, height, seed=seed)
    if sigma == 0:
        return sc, sc.frame_0, sc.frame_1
    rng = np.random.default_rng(100 + seed)
    f0 = (sc.frame_0 + rng.normal(0, sigma, sc.frame_0.shape)).astype(F32)
    f1 = (sc.frame_1 + rng.normal(0, sigma, sc.frame_1.shape)).astype(F32)
    return sc, f0, f1


def border_epe(u, v, scene, r, s, border=BORDER):
    """The endpoint errors of the nodes whose centre is at least `border` pixels from every edge of the frame."""
    h, w = scene.frame_0.shape
    nh, nw = u.shape
    cx, cy = r + np.arange(nw) * s, r + np.arange(nh) * s
    inside = ((cy >= border) & (cy <= h - 1 - border))[:, None] & ((cx >= border) & (cx <= w - 1 - border))[None, :]
    return np.hypot(u - scene.gt_u[np.ix_(cy, cx)], v - scene.gt_v[np.ix_(cy, cx)])[inside]


def accuracy_row(motion, seed, sigma=30.0, single=None, chain=None):
    """The figures of one case: single pass and schedule; `single` / `chain`: callables with the signature of
    correlate_offset_reference / multipass_reference (the device's, in tools/multipass_table.py)."""
    sc, f0, f1 = noisy_scene(motion, seed, sigma)
    lo, scale = frame_range(f0, f1)
    r, d, s = SINGLE
    su, sv, _, srec = (single or correlate_offset_reference)(f0, f1, lo, scale, r, d, s)
    mu, mv, _, reports, _ = (chain or multipass_reference)(f0, f1, lo, scale, SCHEDULE)
    row = {"motion": motion, "seed": seed, "sigma": sigma}
    for name, err, cand, work in (("single", border_epe(su, sv, sc, r, s), int(srec["candidates"][0]), int(srec["candidates"][0]) * (2 * r + 1) ** 2),
                                  ("multi", border_epe(mu, mv, sc, SCHEDULE[-1][0], SCHEDULE[-1][2]),
                                   sum(int(q[2]["candidates"][0]) for q in reports),
                                   sum(int(q[2]["candidates"][0]) * (2 * p[0] + 1) ** 2 for q, p in zip(reports, SCHEDULE)))):
        off = int((~(err <= 1.0)).sum())  # (a NaN node is off)
        row[name] = {"nodes": int(err.size), "epe": "%.4f" % np.nanmean(err), "off_by_1px": off, "candidates": cand, "candidates_x_N": work}
    return row


@pytest.mark.parametrize("motion", ["affine", "large_translation"])
@pytest.mark.parametrize("seed", [0, 1])
def test_three_validated_passes_halve_the_error_under_noise(motion, seed):
    """160 x 128 speckle, Gaussian noise of sigma 30 on both frames, nodes at least 28 px from the border: the schedule
    15:12:16 -> 7:3:8 -> 4:2:4 with validation has at most half the mean endpoint error of one pass (4, 12, 4).  The
    restatement's figures: profiles/multipass/README.md."""
    row = accuracy_row(motion, seed)
    print(row)
    assert row["single"]["nodes"] == row["multi"]["nodes"] == 468
    assert float(row["multi"]["epe"]) <= 0.5 * float(row["single"]["epe"])


# ---- the entries' host side -----------------------------------------------------------------------------------------------------------
def test_refusals_without_a_device(flow2d):
    lib = flow2d.hip_lib()
    fake = ctypes.create_string_buffer(4096)
    w, h, pitch, npitch = 100, 40, 512, 64
    span = pitch * h
    at = lambda k: (1 << 20) + k * (span + 4096)  # noqa: E731  (addresses only: nothing is dereferenced before the device is entered)
    nan, inf = float("nan"), float("inf")
    d = dict(ctx=ctypes.addressof(fake), f0=at(0), f1=at(1), pu=at(6), pv=at(7), w=w, h=h, pitch=pitch, lo=0.0, scale=1.0, r=7, d=8, s=8,
             cut=-1.0, nu=at(2), nv=at(3), ns=at(4), npitch=npitch, record=at(5))

    def call(**kw):
        a = dict(d, **kw)
        return lib.flow2d_correlate_offset_2d(a["ctx"], a["f0"], a["f1"], a["pu"], a["pv"], a["w"], a["h"], a["pitch"], a["lo"], a["scale"],
                                              a["r"], a["d"], a["s"], a["cut"], a["nu"], a["nv"], a["ns"], a["npitch"], a["record"])

    bad = [dict(ctx=None), dict(f0=None), dict(f1=None), dict(nu=None), dict(nv=None), dict(w=0), dict(h=0), dict(pitch=pitch + 8),
           dict(pitch=396), dict(r=0), dict(r=16), dict(r=-1), dict(d=0), dict(d=33), dict(s=0), dict(s=65), dict(scale=0.0),
           dict(scale=-1.0), dict(scale=nan), dict(scale=inf), dict(lo=nan), dict(lo=-inf), dict(cut=nan), dict(w=14), dict(h=14),
           dict(npitch=32), dict(npitch=npitch + 4), dict(f0=at(0) + 4), dict(nu=at(2) + 4), dict(ns=at(4) + 8), dict(record=at(5) + 4),
           dict(nu=at(0)), dict(nv=at(1) + span - pitch), dict(ns=at(0) + pitch), dict(nv=at(2)), dict(ns=at(3) + npitch),
           dict(record=at(0) + 64), dict(record=at(2) + 8),
           # the predictor: one without the other, misaligned, overlapped by a written range
           dict(pu=None), dict(pv=None), dict(pu=at(6) + 4), dict(nu=at(6)), dict(nv=at(7) + span - pitch), dict(ns=at(6) + pitch),
           dict(record=at(7) + 128), dict(pu=at(2)), dict(pv=at(5))]
    for kw in bad:
        assert call(**kw) == 1, kw

    e = dict(ctx=ctypes.addressof(fake), nu=at(0), nv=at(1), nw=11, nh=4, npitch=npitch, t=2.0, eps=0.1, k=3, mode=REPLACE, ou=at(2), ov=at(3),
             flag=at(4), record=at(5))

    def validate(**kw):
        a = dict(e, **kw)
        return lib.flow2d_validate_nodes_2d(a["ctx"], a["nu"], a["nv"], a["nw"], a["nh"], a["npitch"], a["t"], a["eps"], a["k"], a["mode"],
                                            a["ou"], a["ov"], a["flag"], a["record"])

    nspan = npitch * 4
    for kw in [dict(ctx=None), dict(nu=None), dict(nv=None), dict(ou=None), dict(ov=None), dict(nw=0), dict(nh=0), dict(npitch=32),
               dict(npitch=npitch + 4), dict(k=0), dict(k=9), dict(k=-1), dict(t=0.0), dict(t=-1.0), dict(t=nan), dict(t=inf), dict(eps=0.0),
               dict(eps=nan), dict(eps=inf), dict(eps=-0.1), dict(mode=2), dict(mode=-1), dict(ou=at(0)), dict(ov=at(1) + nspan - npitch),
               dict(ov=at(2)), dict(flag=at(0) + npitch), dict(flag=at(3)), dict(record=at(0)), dict(record=at(2) + 8), dict(record=at(5) + 4),
               dict(nu=at(0) + 4), dict(flag=at(4) + 4)]:
        assert validate(**kw) == 1, kw


def test_python_records_match_the_restatement_layout(flow2d):
    rec = flow2d.CorrelationPassRecord()
    rec.nodes, rec.invalid, rec.rejected, rec.unrefined, rec.unpredicted, rec.candidates = 9, 1, 2, 3, 4, 5
    a = np.frombuffer(bytes(rec), PASS_DTYPE)[0]
    assert [int(a[k]) for k in PASS_DTYPE.names[:6]] == [9, 1, 2, 3, 4, 5]
    val = flow2d.ValidationRecord()
    val.nodes, val.judged, val.outliers, val.filled, val.unjudged, val.remaining_invalid = 9, 8, 7, 6, 5, 4
    b = np.frombuffer(bytes(val), VALIDATION_DTYPE)[0]
    assert [int(b[k]) for k in VALIDATION_DTYPE.names[:6]] == [9, 8, 7, 6, 5, 4]
    assert ctypes.sizeof(flow2d.CorrelationPassRecord) == flow2d.CORRELATION_PASS_RECORD_BYTES == 64
    assert ctypes.sizeof(flow2d.ValidationRecord) == flow2d.VALIDATION_RECORD_BYTES == 64
    assert flow2d.CORRELATION_MAX_PASSES == MAX_PASSES and (flow2d.VALIDATE_FLAG, flow2d.VALIDATE_REPLACE) == (FLAG, REPLACE)
    assert rec.summary()["candidates"] == 5 and val.summary()["remaining_invalid"] == 4


def test_schedule_refusals_without_a_device(flow2d):
    ok = flow2d.OpticalFlow.correlation_passes_ok
    assert ok(160, 128, 0.0, 1.0, SCHEDULE) and ok(31, 31, -5.0, 0.25, [(15, 32, 64)] * MAX_PASSES, 0.9, 1.5, 0.01, 8)
    for bad in ([], [(7, 8, 8)] * (MAX_PASSES + 1), [(16, 8, 8)], [(0, 8, 8)], [(7, 33, 8)], [(7, 0, 8)], [(7, 8, 0)], [(7, 8, 65)],
                [(15, 12, 16), (70, 3, 8)]):
        assert not ok(160, 128, 0.0, 1.0, bad), bad
    nan, inf = float("nan"), float("inf")
    for kw in (dict(threshold=0.0), dict(threshold=nan), dict(threshold=inf), dict(epsilon=0.0), dict(epsilon=-1.0), dict(epsilon=nan),
               dict(min_neighbours=0), dict(min_neighbours=9), dict(min_score=nan)):
        assert not ok(160, 128, 0.0, 1.0, SCHEDULE, **kw), kw
    assert not ok(160, 128, 0.0, 0.0, SCHEDULE) and not ok(160, 128, nan, 1.0, SCHEDULE) and not ok(30, 128, 0.0, 1.0, SCHEDULE)
    assert ctypes.sizeof(flow2d.CorrelationPassReport) == 16 + 64 + 64
