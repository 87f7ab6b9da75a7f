"""flow2d_correlate_2d and flow2d_expand_nodes_2d restated in numpy from the text of include/flow2d_c_abi.h (exact integer window
sums by summed-area tables, the score in float64, the expansion in np.float32 operations in the stated order), and what can be
checked without a device: the restatement against an independent formulation, the tie-break, the quantisation's edge values, the
expansion around invalid nodes, the accuracy on the speckle scenes and the entries' host-side refusals."""
import ctypes
import importlib
import itertools

import numpy as np
import pytest

F32 = np.float32
U32 = np.uint32
I64 = np.int64
RECORD_DTYPE = np.dtype([("nodes", "<u8"), ("invalid", "<u8"), ("rejected", "<u8"), ("unrefined", "<u8")])
assert RECORD_DTYPE.itemsize == 32
NAN_BITS = U32(0x7FC00000)
MAX_RADIUS, MAX_RANGE, MAX_SPACING = 15, 32, 64


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def scenes_module():
    return importlib.import_module("cuda-flow2d_amd.scenes")


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def quantise(frame, lo, scale):
    """q of the header: int64, 0 .. 255."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(frame, F32) - F32(lo)) * F32(scale)
        q = np.zeros(t.shape, I64)
        mid = (t > 0) & (t < 255)
        q[mid] = (t[mid] + F32(0.5)).astype(I64)
        q[t >= 255] = 255
    return q


def grid(width, height, r, s):
    return (width - 2 * r - 1) // s + 1, (height - 2 * r - 1) // s + 1


def window_sums(a, r):
    """The sum of `a` (int64) over every (2r + 1)^2 window that lies inside it: [h - 2r, w - 2r], indexed by the window's first
    pixel.  A summed-area table: exact."""
    side = 2 * r + 1
    t = np.zeros((a.shape[0] + 1, a.shape[1] + 1), I64)
    t[1:, 1:] = a.cumsum(0).cumsum(1)
    return t[side:, side:] - t[:-side, side:] - t[side:, :-side] + t[:-side, :-side]


def score_volume(q0, q1, r, d, s):
    """c of every (dy + d, dx + d, node row, node column), -inf where the displacement is no candidate; and V0 per node."""
    h, w = q0.shape
    side, n = 2 * r + 1, (2 * r + 1) ** 2
    nw, nh = grid(w, h, r, s)
    s0, s00 = window_sums(q0, r)[::s, ::s], window_sums(q0 * q0, r)[::s, ::s]
    v0 = n * s00 - s0 * s0
    b1, b11 = window_sums(q1, r), window_sums(q1 * q1, r)
    top, left = np.arange(nh) * s, np.arange(nw) * s
    volume = np.full((2 * d + 1, 2 * d + 1, nh, nw), -np.inf)
    for dy in range(-d, d + 1):
        oky = (top + dy >= 0) & (top + dy + side <= h)
        for dx in range(-d, d + 1):
            okx = (left + dx >= 0) & (left + dx + side <= w)
            if not oky.any() or not okx.any():
                continue
            # q1 displaced by (dx, dy) on frame 0's grid, 0 where it leaves frame 1 (such windows are no candidates)
            moved = np.zeros_like(q1)
            ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
            moved[ys, xs] = q1[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
            s01 = window_sums(q0 * moved, r)[::s, ::s]
            at = np.ix_(np.clip(top + dy, 0, h - side), np.clip(left + dx, 0, w - side))
            s1, s11 = b1[at], b11[at]
            v1 = n * s11 - s1 * s1
            cand = oky[:, None] & okx[None, :] & (v1 > 0) & (v0 > 0)
            cov = n * s01 - s0 * s1
            with np.errstate(divide="ignore", invalid="ignore"):
                c = cov.astype(np.float64) / np.sqrt(v0.astype(np.float64) * v1.astype(np.float64))
            volume[dy + d, dx + d] = np.where(cand, c, -np.inf)
    return volume, v0


def peak_order(d):
    """The displacements from the most to the least preferred among equal scores."""
    return sorted(((dx, dy) for dy in range(-d, d + 1) for dx in range(-d, d + 1)), key=lambda p: (p[0] ** 2 + p[1] ** 2, p[1], p[0]))


def correlate_reference(frame_0, frame_1, lo, scale, r, d, s, min_score=-1.0):
    """(u, v, score, record, (dx, dy)) of flow2d_correlate_2d; (dx, dy): the integer peaks, 0 where a node is invalid."""
    q0, q1 = quantise(frame_0, lo, scale), quantise(frame_1, lo, scale)
    volume, v0 = score_volume(q0, q1, r, d, s)
    nh, nw = v0.shape
    best = np.full((nh, nw), -np.inf)
    bx, by = np.zeros((nh, nw), I64), np.zeros((nh, nw), I64)
    for dx, dy in peak_order(d):  # a later displacement wins only with a larger score
        c = volume[dy + d, dx + d]
        take = c > best
        best = np.where(take, c, best)
        bx, by = np.where(take, dx, bx), np.where(take, dy, by)
    found = best > -np.inf
    jj, ii = np.mgrid[0:nh, 0:nw]
    padded = np.full((2 * d + 3, 2 * d + 3, nh, nw), -np.inf)
    padded[1:-1, 1:-1] = volume
    at = lambda ox, oy: padded[by + d + 1 + oy, bx + d + 1 + ox, jj, ii]  # noqa: E731
    cxm, cxp, cym, cyp = at(-1, 0), at(1, 0), at(0, -1), at(0, 1)
    refined = found & (np.abs(bx) < d) & (np.abs(by) < d) & (cxm > -np.inf) & (cxp > -np.inf) & (cym > -np.inf) & (cyp > -np.inf)

    def delta(cm, cp):
        with np.errstate(invalid="ignore", divide="ignore"):
            den = (cm - 2.0 * best) + cp
            return np.where(refined & (den < 0), (cm - cp) / (2.0 * den), 0.0)

    with np.errstate(invalid="ignore"):
        score = np.where(found, best, 0.0).astype(F32)
        rejected = found & (score < F32(min_score))
        u = (bx.astype(np.float64) + delta(cxm, cxp)).astype(F32)
        v = (by.astype(np.float64) + delta(cym, cyp)).astype(F32)
    gone = ~found | rejected
    u, v = bits(u).copy(), bits(v).copy()
    u[gone], v[gone] = NAN_BITS, NAN_BITS
    record = np.zeros(1, RECORD_DTYPE)
    record["nodes"], record["invalid"], record["rejected"] = nh * nw, (~found).sum(), rejected.sum()
    record["unrefined"] = (found & ~rejected & ~refined).sum()
    return u.view(F32), v.view(F32), score, record, (np.where(found, bx, 0), np.where(found, by, 0))


def expand_reference(node_u, node_v, r, s, width, height):
    """(u, v) of flow2d_expand_nodes_2d."""
    nh, nw = node_u.shape
    node_u, node_v = np.asarray(node_u, F32), np.asarray(node_v, F32)

    def axis(count, nodes):
        f = (np.arange(count).astype(F32) - F32(r)) / F32(s)
        f = np.minimum(np.maximum(f, F32(0)), F32(nodes - 1))
        i0 = np.floor(f).astype(np.int64)
        return i0, np.minimum(i0 + 1, nodes - 1), f - i0.astype(F32)

    i0, i1, ax = axis(width, nw)
    j0, j1, ay = axis(height, nh)
    ax, ay, one = ax[None, :], ay[:, None], F32(1)
    sw, su, sv = (np.zeros((height, width), F32) for _ in range(3))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for wt, jj, ii in (((one - ax) * (one - ay), j0, i0), (ax * (one - ay), j0, i1), ((one - ax) * ay, j1, i0), (ax * ay, j1, i1)):
            nu, nv = node_u[np.ix_(jj, ii)], node_v[np.ix_(jj, ii)]
            part = np.isfinite(nu) & np.isfinite(nv)
            wt = np.broadcast_to(wt, part.shape).astype(F32)
            sw = np.where(part, sw + wt, sw)
            su = np.where(part, su + wt * nu, su)
            sv = np.where(part, sv + wt * nv, sv)
        some = sw > 0
        u, v = bits(np.where(some, su / sw, F32(0))).copy(), bits(np.where(some, sv / sw, F32(0))).copy()
    u[~some], v[~some] = NAN_BITS, NAN_BITS
    return u.view(F32), v.view(F32)


def random_frames(w, h, seed=1, shift=(2, -1), noise=6.0):
    """A random pair in u8's range: frame 1 is frame 0 moved by `shift` (whole pixels, new random content coming in) plus noise."""
    rng = np.random.default_rng(seed)
    big = rng.uniform(0, 255, (h + 80, w + 80))
    f0 = big[40:40 + h, 40:40 + w]
    f1 = big[40 - shift[1]:40 - shift[1] + h, 40 - shift[0]:40 - shift[0] + w] + rng.normal(0, noise, (h, w))
    return f0.astype(F32), f1.astype(F32)


def interior_epe(u, v, scene, r, d, s):
    """The endpoint errors of the nodes whose whole search lies inside the frame: r + d <= centre <= size - 1 - r - d."""
    h, w = scene.shape
    nh, nw = u.shape
    cx, cy = r + np.arange(nw) * s, r + np.arange(nh) * s
    inside = ((cy >= r + d) & (cy <= h - 1 - r - d))[:, None] & ((cx >= r + d) & (cx <= w - 1 - r - d))[None, :]
    err = np.hypot(u - scene.gt_u[np.ix_(cy, cx)], v - scene.gt_v[np.ix_(cy, cx)])
    return err[inside]


def frame_range(frame_0, frame_1):
    """(lo, scale) as OpticalFlow2D::Correlate chooses them: the identity when the finite samples lie in [0, 255]."""
    both = np.concatenate([frame_0[np.isfinite(frame_0)], frame_1[np.isfinite(frame_1)]])
    lo, hi = F32(both.min()), F32(both.max())
    if lo >= 0 and hi <= 255:
        return F32(0), F32(1)
    return lo, F32(255) / (hi - lo)


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def independent(frame_0, frame_1, lo, scale, r, d, s):
    """The textbook form: float64 ZNCC of mean-free windows, node by node and displacement by displacement."""
    q0, q1 = quantise(frame_0, lo, scale).astype(np.float64), quantise(frame_1, lo, scale).astype(np.float64)
    h, w = q0.shape
    side = 2 * r + 1
    nw, nh = grid(w, h, r, s)
    bx, by = np.zeros((nh, nw), I64), np.zeros((nh, nw), I64)
    found = np.zeros((nh, nw), bool)
    order = peak_order(d)
    for j in range(nh):
        for i in range(nw):
            a = q0[j * s:j * s + side, i * s:i * s + side]
            a = a - a.mean()
            if not (a != 0).any():
                continue
            best = -np.inf
            for dx, dy in order:
                x, y = i * s + dx, j * s + dy
                if x < 0 or y < 0 or x + side > w or y + side > h:
                    continue
                b = q1[y:y + side, x:x + side]
                if b.min() == b.max():
                    continue
                b = b - b.mean()
                c = (a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum())
                if c > best:
                    best, bx[j, i], by[j, i], found[j, i] = c, dx, dy, True
    return bx, by, found


@pytest.mark.parametrize("w,h,r,d,s", [(40, 31, 3, 4, 5), (33, 29, 2, 6, 1), (29, 45, 7, 3, 8)])
def test_restatement_against_the_textbook_form(w, h, r, d, s):
    f0, f1 = random_frames(w, h, seed=w)
    f0[5:14, 4:15] = 77.0  # a flat patch: invalid nodes (r <= 3), candidates with V1 = 0 elsewhere
    f1[0:9, 20:31] = 12.0
    u, v, score, record, (bx, by) = correlate_reference(f0, f1, 0.0, 1.0, r, d, s)
    wx, wy, found = independent(f0, f1, 0.0, 1.0, r, d, s)
    assert np.array_equal(bx, wx) and np.array_equal(by, wy)
    assert record["nodes"][0] == found.size and record["invalid"][0] == (~found).sum() and record["rejected"][0] == 0
    assert np.array_equal(np.isnan(u), ~found) and np.array_equal(np.isnan(v), ~found)
    assert (np.abs(u[found] - bx[found]) <= 0.5).all() and (np.abs(v[found] - by[found]) <= 0.5).all()
    assert (score[~found] == 0).all() and (score >= -1).all() and (score <= 1).all()
    # the true whole-pixel shift, except where it is no candidate (the top row of nodes) or frame 1 is flat
    assert np.median(bx[found]) == 2 and np.median(by[found]) == -1


def test_ties_go_to_the_smallest_displacement():
    """A pattern of period 4 in x and 3 in y, identical in both frames, range 6: every displacement (4a, 3b) scores exactly 1.  The
    nearest one to zero that is a candidate wins -- (0, 0) -- and where the frames differ by a whole period, the shortest."""
    h, w = 40, 44
    y, x = np.mgrid[0:h, 0:w]
    f0 = (40 * (x % 4) + 25 * (y % 3) + 7 * ((x % 4) * (y % 3))).astype(F32)
    u, v, score, record, (bx, by) = correlate_reference(f0, f0, 0.0, 1.0, 3, 6, 2)
    assert (bx == 0).all() and (by == 0).all() and (score == 1).all()
    # moved by (1, 0): the candidates are 1 + 4a: 1 wins over -3 and 5; by (2, 0): -2 and 2 tie in length, the smaller dx wins
    f1 = np.roll(f0, 1, axis=1)
    _, _, _, _, (bx, by) = correlate_reference(f0, f1, 0.0, 1.0, 3, 6, 2)
    assert (bx == 1).all() and (by == 0).all()
    f2 = np.roll(f0, 2, axis=1)
    _, _, _, _, (bx, by) = correlate_reference(f0, f2, 0.0, 1.0, 3, 6, 2)
    inner = slice(2, -2)  # (away from the left edge, where -2 is no candidate)
    assert (bx[:, inner] == -2).all() and (by == 0).all() and (bx[:, 0] == 2).all()
    # a tie between dy and dx of the same length: the smaller dy first.  Period 3 in both directions, moved by (0, 0):
    g = (30 * (x % 3) + 50 * (y % 3)).astype(F32)
    _, _, _, _, (bx, by) = correlate_reference(g, g, 0.0, 1.0, 2, 3, 4)
    assert (bx == 0).all() and (by == 0).all()


def test_quantisation_edge_values():
    nan, inf = np.nan, np.inf
    samples = np.array([[nan, inf, -inf, -0.0, 0.0, 254.5, 255.0, 254.49998, -3.0, 0.49, 0.5, 1e30, 300.0, 17.5]], F32)
    assert quantise(samples, 0.0, 1.0).tolist() == [[0, 255, 0, 0, 0, 255, 255, 254, 0, 0, 1, 255, 255, 18]]
    # lo and scale: t = (I - lo) * scale in float32, each operation rounded
    assert quantise(np.array([[10.0, 9.0, 10.5, 137.5, 138.0]], F32), 10.0, 2.0).tolist() == [[0, 0, 1, 255, 255]]
    t = (F32(0.3) - F32(0.1)) * F32(1000.0)
    assert quantise(np.array([[0.3]], F32), 0.1, 1000.0)[0, 0] == int(t + F32(0.5))
    # just below a half rounds up once the sum is rounded to float32
    below = np.nextafter(F32(0.5), F32(0))
    assert quantise(np.array([[below]], F32), 0.0, 1.0)[0, 0] == 1


def test_non_finite_samples_quantise_and_score():
    f0, f1 = random_frames(30, 26, seed=4)
    f0[3, 4], f0[10, 11], f1[7, 7], f1[20, 2] = np.nan, np.inf, -np.inf, np.nan
    u, v, score, record, _ = correlate_reference(f0, f1, 0.0, 1.0, 3, 3, 4)
    assert np.isfinite(score).all() and record["invalid"][0] == 0 and np.isfinite(u).all()


def test_min_score_rejects_and_keeps_the_score():
    f0, f1 = random_frames(60, 40, seed=9, noise=60.0)
    u0, v0, s0, r0, _ = correlate_reference(f0, f1, 0.0, 1.0, 3, 3, 4)
    cut = float(np.median(s0))
    u1, v1, s1, r1, _ = correlate_reference(f0, f1, 0.0, 1.0, 3, 3, 4, cut)
    assert np.array_equal(bits(s0), bits(s1))
    gone = s0 < F32(cut)
    assert 0 < gone.sum() < gone.size and r1["rejected"][0] == gone.sum() and r1["invalid"][0] == 0
    assert np.isnan(u1[gone]).all() and np.isnan(v1[gone]).all()
    assert np.array_equal(bits(u1)[~gone], bits(u0)[~gone]) and np.array_equal(bits(v1)[~gone], bits(v0)[~gone])
    assert r1["unrefined"][0] <= r0["unrefined"][0]
    assert r1["nodes"][0] == r1["invalid"][0] + r1["rejected"][0] + np.isfinite(u1).sum()


def test_one_window_frame_is_one_unrefined_node():
    f0, f1 = random_frames(7, 7, seed=2, shift=(0, 0))
    u, v, score, record, _ = correlate_reference(f0, f1, 0.0, 1.0, 3, 5, 3)
    assert u.shape == (1, 1) and u[0, 0] == 0 and v[0, 0] == 0 and score[0, 0] > 0.9
    assert record.tolist() == [(1, 0, 0, 1)]
    flat = np.full((7, 7), 9.0, F32)
    u, v, score, record, _ = correlate_reference(flat, f1, 0.0, 1.0, 3, 5, 3)
    assert np.isnan(u[0, 0]) and score[0, 0] == 0 and record.tolist() == [(1, 1, 0, 0)]
    u, v, score, record, _ = correlate_reference(f0, flat, 0.0, 1.0, 3, 5, 3)
    assert np.isnan(u[0, 0]) and score[0, 0] == 0 and record.tolist() == [(1, 1, 0, 0)]


def test_expansion_around_invalid_nodes():
    """Four nodes, every combination of valid and invalid: between them the weights of the valid ones are renormalised, beyond
    them the field is constant, and nothing valid gives NaN."""
    r, s, w, h = 2, 5, 12, 11  # nodes at x = 2, 7 and y = 2, 7
    base_u = np.array([[1.0, 2.0], [3.0, 5.0]], F32)
    base_v = np.array([[-1.0, 0.5], [0.25, 8.0]], F32)
    for valid in itertools.product((True, False), repeat=4):
        m = np.array(valid).reshape(2, 2)
        nu, nv = np.where(m, base_u, F32(np.nan)), np.where(m, base_v, F32(np.nan))
        if not valid[3]:
            nv[1, 1], nu[1, 1] = 8.0, np.inf  # one component unusable is enough
        u, v = expand_reference(nu, nv, r, s, w, h)
        if not m.any():
            assert np.isnan(u).all() and np.isnan(v).all()
            continue
        # on a node: its own value, or, where it is invalid, NaN (every other weight is 0)
        for (j, i), ok in np.ndenumerate(m):
            y, x = 2 + 5 * j, 2 + 5 * i
            assert (u[y, x] == base_u[j, i] and v[y, x] == base_v[j, i]) if ok else np.isnan(u[y, x])
        # beyond the outermost nodes: the edge's value
        assert np.array_equal(bits(u[:, :2]), bits(u[:, 2:3].repeat(2, 1))) and np.array_equal(bits(u[9:, :]), bits(u[7:8, :].repeat(2, 0)))
        if m.all():
            assert np.isfinite(u).all()
            assert abs(u[2, 4] - 1.4) < 1e-6 and abs(v[4, 2] - (-0.5)) < 1e-6
        if valid == (True, False, False, False):
            inner = u[2:7, 2:7]  # only node 00 has weight > 0 strictly inside
            assert (inner == 1.0).all()


def test_expansion_with_one_row_or_column():
    nu = np.array([[1.0, np.nan, 3.0, 4.0]], F32)
    nv = -nu
    u, v = expand_reference(nu, nv, 1, 2, 9, 5)  # nodes at x = 1, 3, 5, 7, one row
    assert (bits(u) == bits(u[0:1])).all() and u[0, 0] == 1 and u[0, 1] == 1 and u[0, 2] == 1 and np.isnan(u[0, 3]) and u[0, 4] == 3
    assert u[0, 6] == 3.5 and u[0, 8] == 4 and np.array_equal(np.isnan(v), np.isnan(u)) and (v[np.isfinite(v)] == -u[np.isfinite(u)]).all()
    uc, vc = expand_reference(nu.T.copy(), nv.T.copy(), 1, 2, 5, 9)
    assert np.array_equal(bits(uc), bits(u.T)) and np.array_equal(bits(vc), bits(v.T))
    one_u, one_v = expand_reference(np.array([[2.5]], F32), np.array([[-1.0]], F32), 3, 4, 7, 7)
    assert (one_u == 2.5).all() and (one_v == -1).all()


@pytest.mark.parametrize("motion,d", [("translation", 6), ("affine", 6), ("large_translation", 12)])
def test_accuracy_on_speckle(motion, d):
    """96 x 80, radius 7, spacing 8: the interior nodes' mean endpoint error is at most 0.15 px (the issue's bound; measured:
    profiles/correlation/README.md)."""
    r, s = 7, 8
    sc = scenes_module().make_speckle_scene(motion, 96, 80, seed=0)
    lo, scale = frame_range(sc.frame_0, sc.frame_1)
    u, v, score, record, _ = correlate_reference(sc.frame_0, sc.frame_1, lo, scale, r, d, s)
    err = interior_epe(u, v, sc, r, d, s)
    print("%s: %d interior nodes, mean EPE %.4f, max %.4f, record %s" % (motion, err.size, err.mean(), err.max(), record))
    assert err.size >= 12 and np.isfinite(err).all()
    assert err.mean() <= 0.15


def test_speckle_scene_is_exact():
    """frame_1 is the analytic texture at the inverse-mapped coordinates, and the ground truth takes frame 0's pixels there."""
    sc = scenes_module().make_speckle_scene("affine", 48, 40, seed=3)
    ys, xs = np.mgrid[5:35, 5:43].astype(np.float64)
    there = sc.frame_1_at(xs + sc.gt_u[5:35, 5:43].astype(np.float64), ys + sc.gt_v[5:35, 5:43].astype(np.float64))
    assert np.abs(there - sc.frame_0[5:35, 5:43]).max() < 1e-3
    assert sc.frame_0.std() > 15 and sc.frame_0.min() >= 20
    other = scenes_module().make_speckle_scene("affine", 48, 40, seed=4)
    assert np.abs(other.frame_0 - sc.frame_0).mean() > 5
    assert "speckle" not in " ".join(scenes_module().SCENES)


# ---- the entries' host side ---------------------------------------------------------------------------------------------------------
def test_grid_helper(flow2d):
    for w, h, r, s in ((7, 7, 3, 3), (8, 7, 3, 1), (96, 80, 7, 8), (300, 200, 15, 5), (65, 17, 1, 1), (31, 40, 15, 64)):
        assert flow2d.correlation_grid(w, h, r, s) == grid(w, h, r, s)
    for w, h, r, s in ((6, 7, 3, 1), (7, 6, 3, 1), (40, 40, 0, 1), (40, 40, 16, 1), (40, 40, 3, 0), (40, 40, 3, 65)):
        with pytest.raises(flow2d.Flow2DError):
            flow2d.correlation_grid(w, h, r, s)


def test_refusals_without_a_device(flow2d):
    lib = flow2d.hip_lib()
    fake = ctypes.create_string_buffer(4096)
    w, h, pitch, npitch = 100, 40, 512, 64
    span = pitch * h
    at = lambda k: (1 << 20) + k * (span + 4096)  # noqa: E731  (addresses only: nothing is dereferenced before the device is entered)
    nan, inf = float("nan"), float("inf")
    d = dict(ctx=ctypes.addressof(fake), f0=at(0), f1=at(1), w=w, h=h, pitch=pitch, lo=0.0, scale=1.0, r=7, d=8, s=8, cut=-1.0,
             nu=at(2), nv=at(3), ns=at(4), npitch=npitch, record=at(5))

    def call(**kw):
        a = dict(d, **kw)
        return lib.flow2d_correlate_2d(a["ctx"], a["f0"], a["f1"], a["w"], a["h"], a["pitch"], a["lo"], a["scale"], a["r"], a["d"],
                                       a["s"], a["cut"], a["nu"], a["nv"], a["ns"], a["npitch"], a["record"])

    bad = [dict(ctx=None), dict(f0=None), dict(f1=None), dict(nu=None), dict(nv=None), dict(w=0), dict(h=0), dict(pitch=pitch + 8),
           dict(pitch=396), dict(r=0), dict(r=16), dict(r=-1), dict(d=0), dict(d=33), dict(s=0), dict(s=65), dict(scale=0.0),
           dict(scale=-1.0), dict(scale=nan), dict(scale=inf), dict(lo=nan), dict(lo=-inf), dict(cut=nan), dict(w=14), dict(h=14),
           dict(npitch=32), dict(npitch=npitch + 4), dict(f0=at(0) + 4), dict(nu=at(2) + 4), dict(ns=at(4) + 8), dict(record=at(5) + 4),
           dict(nu=at(0)), dict(nv=at(1) + span - pitch), dict(ns=at(0) + pitch), dict(nv=at(2)), dict(ns=at(3) + npitch),
           dict(record=at(0) + 64), dict(record=at(2) + 8)]
    for kw in bad:
        assert call(**kw) == 1, kw
    # (only refusals here: an accepted call would go on to launch on these made-up addresses where there is a device)
    assert flow2d.correlation_grid(w, h, 7, 8) == (11, 4)

    e = dict(ctx=ctypes.addressof(fake), nu=at(0), nv=at(1), nw=11, nh=4, npitch=npitch, r=7, s=8, ou=at(2), ov=at(3), w=w, h=h, pitch=pitch)

    def expand(**kw):
        a = dict(e, **kw)
        return lib.flow2d_expand_nodes_2d(a["ctx"], a["nu"], a["nv"], a["nw"], a["nh"], a["npitch"], a["r"], a["s"], a["ou"], a["ov"],
                                          a["w"], a["h"], a["pitch"])

    for kw in [dict(ctx=None), dict(nu=None), dict(nv=None), dict(ou=None), dict(ov=None), dict(nw=0), dict(nh=0), dict(w=0), dict(h=0),
               dict(npitch=32), dict(pitch=396), dict(r=-1), dict(r=16), dict(s=0), dict(s=65), dict(ou=at(0)), dict(ov=at(1) + npitch),
               dict(ov=at(2) + span - pitch), dict(nu=at(0) + 4)]:
        assert expand(**kw) == 1, kw


def test_python_record_matches_the_restatement_layout(flow2d):
    rec = flow2d.CorrelationRecord()
    rec.nodes, rec.invalid, rec.rejected, rec.unrefined = 9, 1, 2, 3
    a = np.frombuffer(bytes(rec), RECORD_DTYPE)[0]
    assert (a["nodes"], a["invalid"], a["rejected"], a["unrefined"]) == (9, 1, 2, 3)
    assert ctypes.sizeof(flow2d.CorrelationRecord) == flow2d.CORRELATION_RECORD_BYTES == 32
    assert (flow2d.CORRELATION_MAX_RADIUS, flow2d.CORRELATION_MAX_RANGE, flow2d.CORRELATION_MAX_SPACING) == (MAX_RADIUS, MAX_RANGE, MAX_SPACING)
