"""flow2d_correlate_masked_2d and flow2d_validate_nodes_masked_2d restated in numpy from the text of include/flow2d_c_abi.h -- the
pieces of tests/test_multipass_cpu.py's restatements with the mask: per node the window's sums over m * q, exact integers, the
score in float64; the median test in np.float32 operations over the neighbours that are on the specimen --, the chain of masked
passes built from them, and what can be checked without a device: the restatements against an independent per-node brute force,
the equivalences with the unmasked entries, the order of the states, the off-specimen nodes of the validation, the claim the
entries were built for (edge nodes of a specimen in front of a textured static background), the scene's defaults and the entries'
host-side refusals."""
import ctypes

import numpy as np
import pytest

from test_correlate_cpu import F32, I64, NAN_BITS, U32, bits, expand_reference, grid, peak_order, quantise, random_frames, scenes_module
from test_multipass_cpu import (FLAG, PASS_DTYPE, REPLACE, VALIDATION_DTYPE, correlate_offset_reference, median, node_offsets, same,
                                validate_reference, word)
from test_subset_masked_cpu import random_mask, subset_refine_masked_reference

FLAG_MASKED = 3


def default_min_pixels(r):
    """OpticalFlow2D::ValidationOptions::min_pixels = 0: a quarter of the window, rounded up, and six at least."""
    return max(6, ((2 * r + 1) ** 2 + 3) // 4)


def included(mask):
    """1 where the pixel is not excluded -- m < 0.5 on the float, so a NaN is excluded --, int64."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(mask, F32) < F32(0.5)).astype(I64)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def correlate_masked_reference(frame_0, frame_1, lo, scale, r, d, s, mask, min_pixels, min_score=-1.0, pred_u=None, pred_v=None):
    """(u, v, score, record) of flow2d_correlate_masked_2d; record["reserved"][0, 0] is the count of masked nodes."""
    if mask is None:
        return correlate_offset_reference(frame_0, frame_1, lo, scale, r, d, s, min_score, pred_u, pred_v)
    q0, q1, m = quantise(frame_0, lo, scale), quantise(frame_1, lo, scale), included(mask)
    h, w = q0.shape
    side = 2 * r + 1
    nw, nh = grid(w, h, r, s)
    ox, oy, unpredicted = node_offsets(pred_u, pred_v, w, h, r, s)
    u, v = np.full((nh, nw), NAN_BITS, U32), np.full((nh, nw), NAN_BITS, U32)
    score = np.zeros((nh, nw), F32)
    record = np.zeros(1, PASS_DTYPE)
    record["nodes"] = nh * nw
    dy_of, dx_of = np.mgrid[-d:d + 1, -d:d + 1]
    order = (dx_of * dx_of + dy_of * dy_of) * 10000 + (dy_of + d) * 100 + (dx_of + d)  # the smaller, the more preferred
    for j in range(nh):
        for i in range(nw):
            left, top = i * s, j * s
            mw = m[top:top + side, left:left + side]
            n = int(mw.sum())  # Nv
            if not mw[r, r] or not n >= min_pixels:  # masked: before everything else, the predictor included
                record["reserved"][0, 0] += 1
                continue
            record["unpredicted"] += np.uint64(bool(unpredicted[j, i]))
            a = mw * q0[top:top + side, left:left + side]
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
            s1 = np.einsum("ijkl,kl->ij", windows, mw)
            s11 = np.einsum("ijkl,kl->ij", windows * windows, mw)
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


def off_specimen(mask, nw, nh, r, s):
    """Whether node (j, i) is off the specimen: its centre pixel is excluded."""
    cy, cx = r + np.arange(nh) * s, r + np.arange(nw) * s
    return included(mask)[np.ix_(cy, cx)] == 0


def validate_masked_reference(node_u, node_v, mask, r, s, threshold=2.0, epsilon=0.1, min_neighbours=3, mode=REPLACE):
    """(u, v, flag, record) of flow2d_validate_nodes_masked_2d; mask: the pixel mask of the frame the (r, s) grid lies on;
    record["reserved"][0, 0] is the count of off-specimen nodes."""
    if mask is None:
        return validate_reference(node_u, node_v, threshold, epsilon, min_neighbours, mode)
    node_u, node_v = np.ascontiguousarray(node_u, F32), np.ascontiguousarray(node_v, F32)
    nh, nw = node_u.shape
    assert (nw, nh) == grid(np.shape(mask)[1], np.shape(mask)[0], r, s)
    off = off_specimen(mask, nw, nh, r, s)
    out_u, out_v = bits(node_u).copy(), bits(node_v).copy()
    flag = np.zeros((nh, nw), F32)
    valid = np.isfinite(node_u) & np.isfinite(node_v)
    record = np.zeros(1, VALIDATION_DTYPE)
    record["nodes"] = nh * nw
    threshold, epsilon = F32(threshold), F32(epsilon)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(nh):
            for i in range(nw):
                if off[j, i]:
                    record["reserved"][0, 0] += 1
                    flag[j, i] = FLAG_MASKED
                    out_u[j, i], out_v[j, i] = NAN_BITS, NAN_BITS
                    continue
                ring = [(y, x) for y in (j - 1, j, j + 1) for x in (i - 1, i, i + 1)
                        if (y, x) != (j, i) and 0 <= y < nh and 0 <= x < nw and not off[y, x] and valid[y, x]]
                if len(ring) >= min_neighbours:
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
                else:
                    record["unjudged"] += 1
                fu, fv = out_u[j:j + 1, i:i + 1].view(F32)[0, 0], out_v[j:j + 1, i:i + 1].view(F32)[0, 0]
                record["remaining_invalid"] += np.uint64(not (np.isfinite(fu) and np.isfinite(fv)))
    return out_u.view(F32), out_v.view(F32), flag, record


def masked_multipass_reference(frame_0, frame_1, lo, scale, passes, mask, min_pixels=0, min_score=-1.0, threshold=2.0, epsilon=0.1,
                               min_neighbours=3, replace=True, validate_last=True, predictor=None):
    """OpticalFlow2D::CorrelateMultiPass with ValidationOptions::mask: multipass_reference of tests/test_multipass_cpu.py with the
    two masked entries in every pass (min_pixels 0: the default per pass) and the expansion as it is."""
    h, w = frame_0.shape
    pu, pv = predictor if predictor is not None else (None, None)
    reports = []
    for k, (r, d, s) in enumerate(passes):
        last = k == len(passes) - 1
        u, v, score, record = correlate_masked_reference(frame_0, frame_1, lo, scale, r, d, s, mask, min_pixels or default_min_pixels(r),
                                                         min_score, pu, pv)
        validation = np.zeros(1, VALIDATION_DTYPE)
        if not last or validate_last:
            u, v, _, validation = validate_masked_reference(u, v, mask, r, s, threshold, epsilon, min_neighbours,
                                                            REPLACE if (not last or replace) else FLAG)
        pu, pv = expand_reference(u, v, r, s, w, h)
        reports.append((u.shape[1], u.shape[0], record, validation))
    return u, v, score, reports, (pu, pv)


def counts(record):
    """The eight words of a record."""
    return [int(x) for x in np.frombuffer(record.tobytes(), "<u8")]


# ---- against an independent formulation -------------------------------------------------------------------------------------------
def brute_force(frame_0, frame_1, lo, scale, r, d, s, mask, min_pixels):
    """The textbook form, node by node and displacement by displacement: float64 ZNCC of the mean-free lists of the pixels that
    are not excluded.  Returns the integer peaks, found and masked."""
    q0, q1 = quantise(frame_0, lo, scale).astype(np.float64), quantise(frame_1, lo, scale).astype(np.float64)
    keep = included(mask).astype(bool)
    h, w = q0.shape
    side = 2 * r + 1
    nw, nh = grid(w, h, r, s)
    bx, by = np.zeros((nh, nw), I64), np.zeros((nh, nw), I64)
    found, masked = np.zeros((nh, nw), bool), np.zeros((nh, nw), bool)
    order = peak_order(d)
    for j in range(nh):
        for i in range(nw):
            k = keep[j * s:j * s + side, i * s:i * s + side]
            if not k[r, r] or k.sum() < min_pixels:
                masked[j, i] = True
                continue
            a = q0[j * s:j * s + side, i * s:i * s + side][k]
            a = a - a.mean()
            if not (a != 0).any():
                continue
            best = -np.inf
            for dx, dy in order:
                x, y = i * s + dx, j * s + dy
                if x < 0 or y < 0 or x + side > w or y + side > h:
                    continue
                b = q1[y:y + side, x:x + side][k]
                if b.min() == b.max():
                    continue
                b = b - b.mean()
                c = (a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum())
                if c > best:
                    best, bx[j, i], by[j, i], found[j, i] = c, dx, dy, True
    return bx, by, found, masked


@pytest.mark.parametrize("w,h,r,d,s,min_pixels", [(40, 33, 3, 4, 5, 30), (37, 29, 4, 3, 3, 57), (29, 45, 7, 3, 8, 150)])
def test_restatement_against_the_textbook_form(w, h, r, d, s, min_pixels):
    f0, f1 = random_frames(w, h, seed=w)
    f0[5:14, 4:15] = 77.0  # a flat patch: invalid nodes where the mask leaves enough of it
    mask = random_mask((h, w), seed=w)
    mask[5:14, 4:15] = 0
    mask[0:12, 22:40] = 1  # a block: nodes with the centre excluded, and windows below min_pixels beside it
    u, v, score, record = correlate_masked_reference(f0, f1, 0.0, 1.0, r, d, s, mask, min_pixels)
    bx, by, found, masked = brute_force(f0, f1, 0.0, 1.0, r, d, s, mask, min_pixels)
    assert masked.any() and found.any()
    assert counts(record)[:3] == [found.size, (~found & ~masked).sum(), 0] and counts(record)[6:] == [masked.sum(), 0]
    assert np.array_equal(np.isnan(u), ~found) and np.array_equal(np.isnan(v), ~found) and (score[~found] == 0).all()
    # the integer peak: the sub-pixel part moves a vector by at most a half
    assert (np.abs(u[found] - bx[found]) <= 0.5).all() and (np.abs(v[found] - by[found]) <= 0.5).all()
    assert np.median(bx[found]) == 2 and np.median(by[found]) == -1  # (random_frames' whole-pixel shift)


def test_validation_against_the_unmasked_restatement_on_a_field_without_the_off_nodes():
    """An independent route to the on-specimen nodes: with the off-specimen nodes' vectors replaced by NaN, validate_reference
    sees the same neighbours, so the on-specimen outputs and flags agree."""
    rng = np.random.default_rng(3)
    w, h, r, s = 61, 47, 2, 4
    nw, nh = grid(w, h, r, s)
    u, v = rng.normal(0, 1, (nh, nw)).astype(F32), rng.normal(0, 1, (nh, nw)).astype(F32)
    u[rng.random((nh, nw)) < 0.15] = np.nan
    v[2, 3] = np.inf
    mask = random_mask((h, w), 0.35, seed=9)
    off = off_specimen(mask, nw, nh, r, s)
    assert 0.2 < off.mean() < 0.5
    for mode in (FLAG, REPLACE):
        gu, gv, gf, grec = validate_masked_reference(u, v, mask, r, s, mode=mode)
        wu, wv, wf, wrec = validate_reference(np.where(off, F32(np.nan), u), np.where(off, F32(np.nan), v), mode=mode)
        on = ~off
        assert same(gu[on], wu[on]) and same(gv[on], wv[on]) and same(gf[on], wf[on])
        assert (bits(gu[off]) == NAN_BITS).all() and (bits(gv[off]) == NAN_BITS).all() and (gf[off] == FLAG_MASKED).all()
        c = counts(grec)
        assert c[0] == nw * nh and c[6] == off.sum() and c[7] == 0 and c[1] + c[4] <= on.sum()
        assert c[5] == (~(np.isfinite(gu) & np.isfinite(gv)) & on).sum()
        assert c[2] == (gf == 1).sum() and c[3] == (gf == 2).sum() and c[1] == counts(wrec)[1] and c[2] == counts(wrec)[2]


# ---- equivalences -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,r,d,s", [(40, 31, 3, 4, 5), (29, 45, 7, 3, 8), (7, 7, 3, 5, 3)])
def test_no_mask_and_a_mask_that_excludes_nothing_are_the_unmasked_search(w, h, r, d, s):
    f0, f1 = random_frames(w, h, seed=w)
    if w > 20:
        f0[5:14, 4:15] = 77.0
        f1[0:9, 20:31] = 12.0
    rng = np.random.default_rng(2)
    pu, pv = rng.normal(0, 2, (h, w)).astype(F32), rng.normal(0, 2, (h, w)).astype(F32)
    pu[r, r] = np.nan
    for pred in ((None, None), (pu, pv)):
        want = correlate_offset_reference(f0, f1, 0.0, 1.0, r, d, s, 0.4, *pred)
        none = correlate_masked_reference(f0, f1, 0.0, 1.0, r, d, s, None, -5, 0.4, *pred)
        zero = correlate_masked_reference(f0, f1, 0.0, 1.0, r, d, s, np.zeros((h, w), F32), (2 * r + 1) ** 2, 0.4, *pred)
        low = correlate_masked_reference(f0, f1, 0.0, 1.0, r, d, s, np.full((h, w), 0.49999997, F32), 1, 0.4, *pred)
        for got in (none, zero, low):
            assert all(same(a, b) for a, b in zip(got[:3], want[:3])) and counts(got[3]) == counts(want[3])


def test_no_mask_and_a_mask_that_excludes_no_centre_are_the_unmasked_validation():
    rng = np.random.default_rng(5)
    w, h, r, s = 50, 38, 3, 4
    nw, nh = grid(w, h, r, s)
    u, v = rng.normal(0, 1, (nh, nw)).astype(F32), rng.normal(0, 1, (nh, nw)).astype(F32)
    u[rng.random((nh, nw)) < 0.2] = np.nan
    beside = np.ones((h, w), F32)  # everything excluded but the centres
    beside[r::s, r::s] = 0
    for mode in (FLAG, REPLACE):
        want = validate_reference(u, v, mode=mode)
        for mask in (None, np.zeros((h, w), F32), beside):
            got = validate_masked_reference(u, v, mask, r, s, mode=mode)
            assert all(same(a, b) for a, b in zip(got[:3], want[:3])) and counts(got[3]) == counts(want[3])


# ---- the order of the states ----------------------------------------------------------------------------------------------------------
def test_state_order():
    """Masked comes before everything else: a node whose centre is excluded, or whose window keeps fewer than min_pixels, is
    masked whatever its window and predictor hold -- flat, unpredicted -- and counts in nodes and masked only."""
    w, h, r, d, s = 37, 7, 3, 2, 6  # six nodes in a row, centres at x = 3, 9, ..., 33
    f0, f1 = random_frames(w, h, seed=6, shift=(1, 0))
    side = 2 * r + 1
    min_pixels = 20
    mask = np.zeros((h, w), F32)

    def exclude(i, count):
        """`count` pixels of node i's window, none of them its centre or in a column it shares with a neighbour."""
        cells = [(y, 6 * i + x) for y in range(side) for x in range(1, 6) if (y, x) != (3, 3)]
        for y, x in cells[:count]:
            mask[y, x] = 1

    mask[3, 3] = 1                           # node 0: the centre alone
    exclude(1, side * side - min_pixels + 1)  # node 1: Nv = min_pixels - 1
    exclude(2, side * side - min_pixels)      # node 2: exactly min_pixels
    mask[1, 20] = np.nan                     # node 3: a NaN excludes its pixel
    mask[3, 27] = 1                          # node 4: masked, with a predictor that is not finite
    pu, pv = np.zeros((h, w), F32), np.zeros((h, w), F32)
    pu[3, 27] = np.nan
    pv[3, 33] = np.inf                       # node 5: on the specimen, unpredicted
    nv = [int(included(mask[:, 6 * i:6 * i + side]).sum()) for i in range(6)]
    assert nv[1] == min_pixels - 1 and nv[2] == min_pixels and nv[3] == side * side - 1 and included(mask)[3, 9] and included(mask)[3, 15]
    u, v, score, rec = correlate_masked_reference(f0, f1, 0.0, 1.0, r, d, s, mask, min_pixels, -1.0, pu, pv)
    assert np.isnan(u[0]).tolist() == [True, True, False, False, True, False] and (score[0, [0, 1, 4]] == 0).all()
    assert (bits(u[0, [0, 1, 4]]) == NAN_BITS).all() and (bits(v[0, [0, 1, 4]]) == NAN_BITS).all()
    assert counts(rec)[0] == 6 and counts(rec)[1] == 0 and counts(rec)[4] == 1 and counts(rec)[6] == 3
    # node 3 differs from the unmasked search only through its one excluded pixel; flat windows behind the mask are masked, not invalid
    flat = f0.copy()
    flat[:, 0:7] = 9.0
    _, _, _, rec = correlate_masked_reference(flat, f1, 0.0, 1.0, r, d, s, mask, min_pixels, -1.0, pu, pv)
    assert counts(rec)[1] == 0 and counts(rec)[6] == 3
    # candidates count over the nodes that are neither masked nor flat
    _, _, _, base = correlate_masked_reference(f0, f1, 0.0, 1.0, r, d, s, mask, min_pixels)
    flat2 = f0.copy()
    flat2[:, 30:37] = 9.0
    _, _, _, rec = correlate_masked_reference(flat2, f1, 0.0, 1.0, r, d, s, mask, min_pixels)
    assert counts(rec)[1] == 1 and counts(rec)[5] < counts(base)[5]


def test_excluded_pixels_do_not_reach_the_score():
    """What lies under the mask in frame 0 is not read into a result: any values there give the same bytes."""
    w, h, r, d, s = 40, 33, 3, 4, 5
    f0, f1 = random_frames(w, h, seed=12)
    mask = random_mask((h, w), seed=4)
    want = correlate_masked_reference(f0, f1, 0.0, 1.0, r, d, s, mask, 10)
    g0 = np.where(mask > 0.5, F32(255.0) - f0, f0).astype(F32)
    got = correlate_masked_reference(g0, f1, 0.0, 1.0, r, d, s, mask, 10)
    assert all(same(a, b) for a, b in zip(got[:3], want[:3])) and counts(got[3]) == counts(want[3])
    assert not same(correlate_offset_reference(g0, f1, 0.0, 1.0, r, d, s)[0], correlate_offset_reference(f0, f1, 0.0, 1.0, r, d, s)[0])


# ---- the validation's off-specimen nodes ---------------------------------------------------------------------------------------------
def test_off_specimen_nodes_are_no_neighbours_and_come_out_masked():
    w, h, r, s = 23, 23, 1, 4  # 6 x 6 nodes at 1, 5, ..., 21
    nw, nh = grid(w, h, r, s)
    u = np.full((nh, nw), 0.25, F32)
    v = np.full((nh, nw), -1.0, F32)
    u[2, 2], v[2, 2] = 7.0, 3.0  # on the specimen, far from the ring's vectors
    mask = np.zeros((h, w), F32)
    for y in (1, 2, 3):
        for x in (1, 2, 3):
            if (y, x) != (2, 2):
                mask[r + y * s, r + x * s] = 1  # the ring of (2, 2): off the specimen, with finite vectors
    for mode in (FLAG, REPLACE):
        ou, ov, flag, rec = validate_masked_reference(u, v, mask, r, s, mode=mode)
        # k = 0 < min_neighbours: unjudged, its own bits -- the unmasked test would have replaced it by the ring's median
        assert ou[2, 2] == 7 and ov[2, 2] == 3 and flag[2, 2] == 0
        assert validate_reference(u, v, mode=mode)[2][2, 2] == 1
        off = off_specimen(mask, nw, nh, r, s)
        assert off.sum() == 8 and (flag[off] == FLAG_MASKED).all() and (bits(ou[off]) == NAN_BITS).all() and (bits(ov[off]) == NAN_BITS).all()
        # nodes, judged, outliers, filled, unjudged, remaining_invalid, masked: 36 - 8 on the specimen; besides (2, 2) the border
        # nodes (0, 0), (0, 2) and (2, 0) keep only two neighbours
        assert counts(rec) == [36, 24, 0, 0, 4, 0, 8, 0]
    # an off-specimen node whose vector is NaN already: still flag 3, still not in remaining_invalid
    u[1, 1] = np.nan
    _, _, flag, rec = validate_masked_reference(u, v, mask, r, s, mode=FLAG)
    assert flag[1, 1] == FLAG_MASKED and counts(rec)[5] == 0 and counts(rec)[6] == 8


# ---- the claim ------------------------------------------------------------------------------------------------------------------------
CLAIM_GRID = (7, 10, 8)
CLAIM_SCENE = dict(translation=(6.4, -3.3), background_gain=1.0, background_offset=0.0)


def extremes(frame_0, frame_1):
    """(lo, scale) from the two frames' extremes."""
    lo, hi = F32(min(frame_0.min(), frame_1.min())), F32(max(frame_0.max(), frame_1.max()))
    return lo, F32(255) / (hi - lo)


def claim_case(name, scene_args=CLAIM_SCENE, grid_=CLAIM_GRID):
    """The scene, its mask, and per node: on the specimen, edge (on the specimen with an excluded pixel in the window), the truth."""
    sc, mask = scenes_module().make_speckle_specimen(name, 96, 80, seed=0, **scene_args)
    r, d, s = grid_
    nw, nh = grid(96, 80, r, s)
    cy, cx = r + np.arange(nh) * s, r + np.arange(nw) * s
    m = included(mask)
    on = m[np.ix_(cy, cx)] == 1
    full = np.array([[m[y - r:y + r + 1, x - r:x + r + 1].all() for x in cx] for y in cy])
    return sc, mask, on, on & ~full, sc.gt_u[np.ix_(cy, cx)], sc.gt_v[np.ix_(cy, cx)]


def off_truth(u, v, tu, tv, where, limit=1.5):
    """The nodes of `where` that are more than `limit` px from the truth, a NaN among them."""
    return int((~(np.hypot(u - tu, v - tv)[where] <= limit)).sum())


def claim_counts(name, correlate=None, validate=None, correlate_masked=None, validate_masked=None):
    """The four rows of the issue's table for one scene: (edge nodes off, interior on-specimen nodes off) of the search as it is,
    then validated, of the masked search, then the masked validation.  The callables default to the restatements (the device's,
    in tools/search_mask_table.py)."""
    sc, mask, on, edge, tu, tv = claim_case(name)
    r, d, s = CLAIM_GRID
    lo, scale = extremes(sc.frame_0, sc.frame_1)
    rows = {}
    u, v, _, _ = (correlate or correlate_offset_reference)(sc.frame_0, sc.frame_1, lo, scale, r, d, s)
    rows["search"] = (off_truth(u, v, tu, tv, edge), off_truth(u, v, tu, tv, on & ~edge))
    u, v = (validate or validate_reference)(u, v)[:2]
    rows["search+validate"] = (off_truth(u, v, tu, tv, edge), off_truth(u, v, tu, tv, on & ~edge))
    u, v, _, _ = (correlate_masked or correlate_masked_reference)(sc.frame_0, sc.frame_1, lo, scale, r, d, s, mask, default_min_pixels(r))
    rows["masked"] = (off_truth(u, v, tu, tv, edge), off_truth(u, v, tu, tv, on & ~edge))
    u, v = (validate_masked or validate_masked_reference)(u, v, mask, r, s)[:2]
    rows["masked+validate"] = (off_truth(u, v, tu, tv, edge), off_truth(u, v, tu, tv, on & ~edge))
    return rows, int(edge.sum()), int((on & ~edge).sum())


@pytest.mark.parametrize("name", ["stretch", "rotation"])
def test_edge_nodes_follow_the_specimen_only_with_the_mask(name):
    """The plate with a hole moved by (6.4, -3.3) in front of a static background of the specimen's own contrast, grid (7, 10, 8),
    lo and scale from the frames' extremes, min_pixels 57.  With the masked restatements no on-specimen node is more than 1.5 px
    from the truth; with the unmasked search followed by validate_reference at least one edge node is (the fp32 restatements'
    counts: profiles/search_mask/table_numpy.md)."""
    rows, edges, interior = claim_counts(name)
    print(name, edges, interior, rows)
    assert edges == 29 and interior == 15
    assert rows["masked"] == (0, 0) and rows["masked+validate"] == (0, 0)
    assert rows["search+validate"][0] >= 1


# ---- the whole chain ------------------------------------------------------------------------------------------------------------------
EASY_SCENE = dict(translation=(1.6, -0.7), background_gain=0.3, background_offset=5.0)  # make_speckle_specimen's defaults
CHAIN_SUBSET = dict(R=7, min_pixels=57, max_shift=2.0)


def chain_figures(name, scene_args, mask_search, correlate=None, validate=None, refine=None):
    """Search (7, 10, 8), validation with replacement and the masked refinement (R = 7, min_pixels 57, max_shift 2) of one scene;
    mask_search: the search and the validation are the masked ones (OpticalFlow2D::SubsetOptions::mask_search).  Per class of
    on-specimen nodes -- edge: an excluded pixel in the window; interior: none -- the nodes, the converged ones, and over these
    the mean and the worst endpoint error.  The callables default to the restatements: correlate(f0, f1, lo, scale, r, d, s, mask
    or None, min_pixels), validate(u, v, mask or None, r, s), refine(scene, mask, u0, v0) -> an object with u, v, state."""
    sc, mask, on, edge, tu, tv = claim_case(name, scene_args)
    r, d, s = CLAIM_GRID
    lo, scale = extremes(sc.frame_0, sc.frame_1)
    region = mask if mask_search else None
    correlate = correlate or (lambda f0, f1, lo, scale, r, d, s, m, n: correlate_masked_reference(f0, f1, lo, scale, r, d, s, m, n))
    validate = validate or (lambda u, v, m, r, s: validate_masked_reference(u, v, m, r, s))
    u, v = correlate(sc.frame_0, sc.frame_1, lo, scale, r, d, s, region, default_min_pixels(r))[:2]
    u, v = validate(u, v, region, r, s)[:2]
    if refine is None:
        got = subset_refine_masked_reference(sc.frame_0, sc.frame_1, u, v, None, mask, CHAIN_SUBSET["min_pixels"], r, s, CHAIN_SUBSET["R"],
                                             max_shift=CHAIN_SUBSET["max_shift"])
    else:
        got = refine(sc, mask, u, v)
    err = np.hypot(got.u.astype(np.float64) - tu, got.v.astype(np.float64) - tv)
    out = {}
    for label, where in (("edge", edge), ("interior", on & ~edge)):
        live = where & (got.state >= 1)
        out[label] = dict(nodes=int(where.sum()), converged=int(live.sum()), mean=float(err[live].mean()) if live.any() else float("nan"),
                          worst=float(err[live].max()) if live.any() else float("nan"))
    return out


@pytest.mark.parametrize("name", ["stretch", "rotation"])
def test_the_masked_search_is_not_worse_on_the_interior_nodes(name):
    """On the moved plate and on the committed easy scene: the interior nodes -- every pixel of the window on the specimen -- see
    the same sums with and without the mask, so the search gives them the same vectors; the validation may still hand one another
    start (its neighbours differ), and two refinements that stop at an update below epsilon = 1e-3 from different starts agree to
    that epsilon, which is the bound here.  The edge nodes converge at least as often with the masked search in front (the
    figures: profiles/search_mask/table_numpy.md)."""
    for scene_args in (CLAIM_SCENE, EASY_SCENE):
        plain, masked = chain_figures(name, scene_args, False), chain_figures(name, scene_args, True)
        print(name, scene_args["translation"], plain, masked)
        assert masked["interior"]["converged"] >= plain["interior"]["converged"] == plain["interior"]["nodes"]
        assert masked["interior"]["worst"] <= plain["interior"]["worst"] + 1e-3
        assert masked["edge"]["converged"] >= plain["edge"]["converged"]


# ---- the scene ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stretch", "rotation", "shear"])
def test_scene_defaults_give_the_former_arrays(name):
    """make_speckle_specimen's new keyword arguments at their defaults: the former construction, restated here, bit for bit."""
    sm = scenes_module()
    sc, mask = sm.make_speckle_specimen(name, 64, 48, seed=2)
    explicit, mask2 = sm.make_speckle_specimen(name, 64, 48, seed=2, translation=(1.6, -0.7), background_gain=0.3, background_offset=5.0)
    plain = sm.make_speckle_deformation(name, 64, 48, 2)
    texture, background = sm.Speckle(2), sm.Speckle(9)
    ys, xs = np.mgrid[0:48, 0:64].astype(np.float64)
    c0, c1 = 63 / 2.0, 47 / 2.0
    half_w, half_h, hole = 30.5 * 64 / 96.0, 24.5 * 48 / 80.0, 9.5 * min(64 / 96.0, 48 / 80.0)
    inside = lambda x, y: (np.abs(x - c0) <= half_w) & (np.abs(y - c1) <= half_h) & ((x - c0) ** 2 + (y - c1) ** 2 > hole ** 2)  # noqa: E731
    ground = 0.3 * background(xs, ys) + 5.0
    bu, bv = plain.back_flow_at(xs, ys)
    f0 = np.where(inside(xs, ys), texture(xs, ys), ground).astype(F32)
    f1 = np.where(inside(xs + bu, ys + bv), texture(xs + bu, ys + bv), ground).astype(F32)
    for got in (sc, explicit):
        assert same(got.frame_0, f0) and same(got.frame_1, f1) and same(got.gt_u, plain.gt_u) and same(got.gt_v, plain.gt_v)
    assert same(mask, np.where(inside(xs, ys), 0.0, 1.0).astype(F32)) and same(mask2, mask)
    moved, _ = sm.make_speckle_specimen(name, 64, 48, seed=2, translation=(6.4, -3.3), background_gain=1.0, background_offset=0.0)
    assert abs(float((moved.gt_u - sc.gt_u).mean()) - 4.8) < 1e-4 and abs(float((moved.gt_v - sc.gt_v).mean()) + 2.6) < 1e-4
    assert same(moved.frame_0[mask == 1], background(xs, ys).astype(F32)[mask == 1])


# ---- the entries' host side -----------------------------------------------------------------------------------------------------------
def test_refusals_without_a_device(flow2d):
    lib = flow2d.hip_lib()
    fake = ctypes.create_string_buffer(4096)
    w, h, pitch, npitch = 100, 40, 512, 64
    span = pitch * h
    at = lambda k: (1 << 20) + k * (span + 4096)  # noqa: E731  (addresses only: nothing is dereferenced before the device is entered)
    nan, inf = float("nan"), float("inf")
    d = dict(ctx=ctypes.addressof(fake), f0=at(0), f1=at(1), pu=at(6), pv=at(7), w=w, h=h, pitch=pitch, lo=0.0, scale=1.0, r=7, d=8, s=8,
             cut=-1.0, mask=at(8), minp=57, nu=at(2), nv=at(3), ns=at(4), npitch=npitch, record=at(5))

    def call(**kw):
        a = dict(d, **kw)
        return lib.flow2d_correlate_masked_2d(a["ctx"], a["f0"], a["f1"], a["pu"], a["pv"], a["w"], a["h"], a["pitch"], a["lo"], a["scale"],
                                              a["r"], a["d"], a["s"], a["cut"], a["mask"], a["minp"], a["nu"], a["nv"], a["ns"], a["npitch"],
                                              a["record"])

    bad = [dict(ctx=None), dict(f0=None), dict(f1=None), dict(nu=None), dict(nv=None), dict(w=0), dict(h=0), dict(pitch=pitch + 8),
           dict(pitch=396), dict(r=0), dict(r=16), dict(r=-1), dict(d=0), dict(d=33), dict(s=0), dict(s=65), dict(scale=0.0),
           dict(scale=-1.0), dict(scale=nan), dict(scale=inf), dict(lo=nan), dict(lo=-inf), dict(cut=nan), dict(w=14), dict(h=14),
           dict(npitch=32), dict(npitch=npitch + 4), dict(f0=at(0) + 4), dict(nu=at(2) + 4), dict(ns=at(4) + 8), dict(record=at(5) + 4),
           dict(nu=at(0)), dict(nv=at(1) + span - pitch), dict(ns=at(0) + pitch), dict(nv=at(2)), dict(ns=at(3) + npitch),
           dict(record=at(0) + 64), dict(record=at(2) + 8),
           dict(pu=None), dict(pv=None), dict(pu=at(6) + 4), dict(nu=at(6)), dict(nv=at(7) + span - pitch), dict(ns=at(6) + pitch),
           dict(record=at(7) + 128), dict(pu=at(2)), dict(pv=at(5)),
           # the mask: misaligned, overlapped by a written range; min_pixels outside 1 .. (2r + 1)^2
           dict(mask=at(8) + 4), dict(nu=at(8)), dict(nv=at(8) + span - pitch), dict(ns=at(8) + pitch), dict(record=at(8) + 256),
           dict(mask=at(2)), dict(mask=at(5)), dict(minp=0), dict(minp=-1), dict(minp=226), dict(r=3, minp=50)]
    for kw in bad:
        assert call(**kw) == 1, kw
    # without a mask the call is forwarded: min_pixels is not looked at, and the refusal is the unmasked entry's
    assert call(mask=None, minp=0, f0=None) == 1 and call(mask=None, minp=10 ** 6, r=16) == 1

    e = dict(ctx=ctypes.addressof(fake), nu=at(0), nv=at(1), nw=11, nh=4, npitch=npitch, t=2.0, eps=0.1, k=3, mode=REPLACE, mask=at(8), w=w,
             h=h, pitch=pitch, r=7, s=8, ou=at(2), ov=at(3), flag=at(4), record=at(5))

    def validate(**kw):
        a = dict(e, **kw)
        return lib.flow2d_validate_nodes_masked_2d(a["ctx"], a["nu"], a["nv"], a["nw"], a["nh"], a["npitch"], a["t"], a["eps"], a["k"],
                                                   a["mode"], a["mask"], a["w"], a["h"], a["pitch"], a["r"], a["s"], a["ou"], a["ov"],
                                                   a["flag"], a["record"])

    nspan = npitch * 4
    for kw in [dict(ctx=None), dict(nu=None), dict(nv=None), dict(ou=None), dict(ov=None), dict(nw=0), dict(nh=0), dict(npitch=32),
               dict(npitch=npitch + 4), dict(k=0), dict(k=9), dict(k=-1), dict(t=0.0), dict(t=-1.0), dict(t=nan), dict(t=inf), dict(eps=0.0),
               dict(eps=nan), dict(eps=inf), dict(eps=-0.1), dict(mode=2), dict(mode=-1), dict(ou=at(0)), dict(ov=at(1) + nspan - npitch),
               dict(ov=at(2)), dict(flag=at(0) + npitch), dict(flag=at(3)), dict(record=at(0)), dict(record=at(2) + 8), dict(record=at(5) + 4),
               dict(nu=at(0) + 4), dict(flag=at(4) + 4),
               # the mask and the geometry: the plane rules, the limits, a grid that is not the geometry's, overlaps
               dict(mask=at(8) + 4), dict(w=0), dict(h=0), dict(pitch=396), dict(pitch=pitch + 8), dict(r=0), dict(r=16), dict(s=0), dict(s=65),
               dict(w=14), dict(nw=10), dict(nh=5), dict(s=9), dict(r=3), dict(ou=at(8)), dict(ov=at(8) + span - pitch), dict(flag=at(8) + pitch),
               dict(record=at(8) + 64), dict(mask=at(2)), dict(mask=at(5))]:
        assert validate(**kw) == 1, kw
    assert validate(mask=None, w=0, r=99, nu=None) == 1  # forwarded: the geometry is not looked at


def test_python_names(flow2d):
    rec = flow2d.CorrelationPassRecord()
    rec.reserved[0] = 5
    val = flow2d.ValidationRecord()
    val.reserved[0] = 7
    assert rec.masked == 5 and val.masked == 7 and "masked" not in rec.summary() and flow2d.VALIDATE_FLAG_MASKED == FLAG_MASKED
    assert [flow2d.correlation_min_pixels(r) for r in (1, 2, 7, 15)] == [default_min_pixels(r) for r in (1, 2, 7, 15)] == [6, 7, 57, 241]
    assert np.frombuffer(bytes(rec), PASS_DTYPE)["reserved"][0, 0] == 5 and np.frombuffer(bytes(val), VALIDATION_DTYPE)["reserved"][0, 0] == 7


def test_host_refusals_without_a_device(flow2d):
    """OpticalFlow2D::CorrelationPassesOk: an explicit min_pixels must fit every pass's window; SubsetOptionsOk: mask_search needs a
    mask."""
    ok = flow2d.OpticalFlow.correlation_passes_ok
    schedule = ((15, 12, 16), (7, 3, 8), (4, 2, 4))
    assert ok(160, 128, 0.0, 1.0, schedule) and ok(160, 128, 0.0, 1.0, schedule, min_pixels=1) and ok(160, 128, 0.0, 1.0, schedule, min_pixels=81)
    assert not ok(160, 128, 0.0, 1.0, schedule, min_pixels=82) and not ok(160, 128, 0.0, 1.0, schedule, min_pixels=-1)
    assert ok(160, 128, 0.0, 1.0, schedule[:2], min_pixels=225) and not ok(160, 128, 0.0, 1.0, schedule[:2], min_pixels=226)
    assert not ok(160, 128, 0.0, 1.0, [(16, 8, 8)], min_pixels=57) and not ok(160, 128, 0.0, 1.0, schedule, threshold=0.0, min_pixels=57)
    lib = flow2d.host_lib()
    with_mask = flow2d.SubsetOptions(7, 20, 1e-3, 2.0, 0.5, 1, 0.05, 0, 1)
    without = flow2d.SubsetOptions(7, 20, 1e-3, 2.0, 0.5, 1, 0.05, 0, None)
    second_order = flow2d.SubsetOptions(7, 20, 1e-3, 2.0, 0.5, 2, 0.05, 0, 1)
    assert lib.flow2d_host_subset_mask_search_ok(ctypes.byref(with_mask)) == 1
    assert lib.flow2d_host_subset_mask_search_ok(ctypes.byref(without)) == 0 and lib.flow2d_host_subset_mask_search_ok(None) == 0
    assert lib.flow2d_host_subset_mask_search_ok(ctypes.byref(second_order)) == 0  # (a mask with order 2 is refused as before)
    assert lib.flow2d_host_subset_options_ok(ctypes.byref(without)) == 1  # without the flag: as before
    assert lib.flow2d_host_set_subset_mask_search(None, 1) == 1
