"""flow2d_subset_uncertainty_2d restated in numpy from the text of include/flow2d_c_abi.h: per node the covariance s2 * H^-1 of the
first-order refinement's p, from the Cholesky factor, the samplers, the usable list and the three summation orders of the existing
restatements (tests/test_subset_cpu.py, tests/test_subset_masked_cpu.py, tests/test_subset_spline_cpu.py; the device's order is
"butterfly").  What can be checked without a device: the two exact properties (scaling by two, a pair that matches exactly), the
calibration against the scatter of the refinement's own output under noise -- written to
profiles/subset_uncertainty/calibration.json, which tools/uncertainty_table.py prints --, the degrees of freedom, every early
exit with its count, the agreement of the three orders and the entry's host-side refusals."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from test_correlate_cpu import F32, U32, NAN_BITS, bits, grid
from test_subset_cpu import F64, ORDERS, ROOT, SUMS, cholesky, cubic_sample, interior_mask, make_case_scene, small_case, solve, subset_refine_reference
from test_subset_masked_cpu import MIN_PIXELS, block_mask, default_min_pixels, excluded_plane, random_mask, usable_plane
from test_subset_spline_cpu import bspline_prefilter_reference, bspline_sample

UNCERTAINTY_DTYPE = np.dtype([("nodes", "<u8"), ("evaluated", "<u8"), ("skipped", "<u8"), ("masked", "<u8"), ("outside", "<u8"),
                              ("flat", "<u8"), ("thin", "<u8"), ("reserved", "<u8")])
assert UNCERTAINTY_DTYPE.itemsize == 64
PLANES = ("sigma_u", "sigma_v", "rho", "sigma_ux", "sigma_uy", "sigma_vx", "sigma_vy", "noise")
EVALUATED, SKIPPED, MASKED, OUTSIDE, FLAT, THIN = "evaluated", "skipped", "masked", "outside", "flat", "thin"
PROFILE_DIR = os.path.join(ROOT, "profiles", "subset_uncertainty")
CALIBRATION_PATH = os.path.join(PROFILE_DIR, "calibration.json")
SPREAD_PATH = os.path.join(PROFILE_DIR, "order_spread.json")
SAMPLERS = (cubic_sample, bspline_sample)  # by `interpolation`


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def uncertainty_node(f0, f1, usable, cx, cy, p, R, min_pixels, sample, total):
    """(fate, the eight outputs in float64 or None) of one node that is neither masked by its centre nor skipped: the text from
    3. *Outside* on.  usable None: no mask."""
    h, w = f0.shape
    side = 2 * R + 1
    if not (cx - R >= 0 and cy - R >= 0 and cx + R <= w - 1 and cy + R <= h - 1):
        return OUTSIDE, None
    k = np.arange(side * side)
    if usable is not None:
        k = k[usable[cy + k // side - R, cx + k % side - R]]  # the list, in ascending k
        if not k.size >= min_pixels:
            return MASKED, None
    if not k.size >= 9:
        return THIN, None
    n = F64(k.size)
    kx, ky = k % side - R, k // side - R
    xi, eta = kx.astype(F64), ky.astype(F64)
    xs, ys = cx + kx, cy + ky
    f = f0[ys, xs]
    fx = (f0[ys, np.minimum(xs + 1, w - 1)] - f0[ys, np.maximum(xs - 1, 0)]) * 0.5
    fy = (f0[np.minimum(ys + 1, h - 1), xs] - f0[np.maximum(ys - 1, 0), xs]) * 0.5
    fd = f - total(f) / n
    df2 = total(fd * fd)
    if not df2 > 0:
        return FLAT, None
    df = np.sqrt(df2)
    J = np.stack([fx, fx * xi, fx * eta, fy, fy * xi, fy * eta], axis=1)
    L = cholesky(total(J[:, :, None] * J[:, None, :]))
    if L is None:
        return FLAT, None
    u, ux, uy, v, vx, vy = p
    X = xs.astype(F64) + ((u + ux * xi) + uy * eta)
    Y = ys.astype(F64) + ((v + vx * xi) + vy * eta)
    if not ((X >= 0) & (X <= w - 1) & (Y >= 0) & (Y <= h - 1)).all():
        return OUTSIDE, None
    g = sample(f1, X, Y)
    gd = g - total(g) / n
    dg2 = total(gd * gd)
    if not dg2 > 0:
        return FLAT, None
    res = fd - (df / np.sqrt(dg2)) * gd
    s2 = total(res * res) / F64(k.size - 8)
    x = [solve(L, np.eye(6, dtype=F64)[a]) for a in range(6)]
    d = [x[a][a] for a in range(6)]
    return EVALUATED, np.array([np.sqrt(s2 * d[0]), np.sqrt(s2 * d[3]), x[0][3] / np.sqrt(d[0] * d[3]), np.sqrt(s2 * d[1]), np.sqrt(s2 * d[2]),
                                np.sqrt(s2 * d[4]), np.sqrt(s2 * d[5]), np.sqrt(s2)], F64)


class Uncertainty:
    """The outputs of flow2d_subset_uncertainty_2d: the eight float32 planes of PLANES, the record, the nodes' fates, and out64 --
    the outputs in float64 where a node was evaluated, NaN elsewhere -- for the spread between orders."""

    def planes(self):
        return [getattr(self, name) for name in PLANES]


def subset_uncertainty_reference(frame_0, frame_1, nodes, state, r, s, R, min_state=1, mask=None, min_pixels=None, interpolation=0,
                                 order="butterfly"):
    """nodes = (u, v, ux, uy, vx, vy) float planes and their state plane; frame_1 is frame 1, or with interpolation = 1 its
    coefficients; mask None: min_pixels is not looked at."""
    assert min_state in (0, 1) and interpolation in (0, 1) and 1 <= R <= 15
    f0, f1 = np.asarray(frame_0, F32).astype(F64), np.asarray(frame_1, F32).astype(F64)
    excluded = usable = None
    if mask is not None:
        min_pixels = default_min_pixels(R) if min_pixels is None else min_pixels
        assert MIN_PIXELS <= min_pixels <= (2 * R + 1) ** 2
        excluded, usable = excluded_plane(mask), usable_plane(mask)
        assert excluded.shape == f0.shape
    u, v, ux, uy, vx, vy = (np.asarray(q, F32) for q in nodes)
    start = np.stack([u, ux, uy, v, vx, vy], axis=-1)  # the order of p
    state = np.asarray(state, F32)
    nh, nw = state.shape
    out = Uncertainty()
    planes = np.full((8, nh, nw), np.nan, F32)
    out.out64 = np.full((nh, nw, 8), np.nan)
    out.fate = np.empty((nh, nw), object)
    record = np.zeros(1, UNCERTAINTY_DTYPE)
    record["nodes"] = nh * nw
    with np.errstate(all="ignore"):
        for j in range(nh):
            for i in range(nw):
                cx, cy = r + i * s, r + j * s
                values = None
                if excluded is not None and excluded[cy, cx]:
                    fate = MASKED
                elif not state[j, i] >= F32(min_state) or not np.isfinite(start[j, i]).all():
                    fate = SKIPPED
                else:
                    fate, values = uncertainty_node(f0, f1, usable, cx, cy, start[j, i].astype(F64), R, min_pixels, SAMPLERS[interpolation],
                                                    SUMS[order])
                out.fate[j, i] = fate
                record[fate] += 1
                if values is not None:
                    planes[:, j, i] = values.astype(F32)
                    out.out64[j, i] = values
    words = bits(planes)
    words[np.isnan(planes)] = NAN_BITS
    planes = words.view(F32)
    for name, plane in zip(PLANES, planes):
        setattr(out, name, plane)
    out.record = record
    return out


def all_orders_uncertainty(*args, **kw):
    """(the butterfly order's result, the largest relative spread of an output between the three orders); the orders must agree
    on every node's fate."""
    runs = [subset_uncertainty_reference(*args, order=o, **kw) for o in ORDERS]
    for other in runs[:2]:
        assert np.array_equal(other.fate, runs[2].fate) and other.record.tobytes() == runs[2].record.tobytes()
    stack = np.stack([q.out64 for q in runs])
    live = np.isfinite(stack[2]) & (stack[2] != 0)
    spread = float(((stack.max(0) - stack.min(0))[live] / np.abs(stack[2][live])).max()) if live.any() else 0.0
    return runs[2], spread


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def truth_at_nodes(scene, r, s):
    """The ground truth rounded to whole pixels at the nodes of the grid (r, s): a refinement's start."""
    h, w = scene.frame_0.shape
    nw, nh = grid(w, h, r, s)
    cy, cx = r + np.arange(nh) * s, r + np.arange(nw) * s
    return np.rint(scene.gt_u[np.ix_(cy, cx)]).astype(F32), np.rint(scene.gt_v[np.ix_(cy, cx)]).astype(F32)


def refined_nodes(got):
    return [got.u, got.v, got.ux, got.uy, got.vx, got.vy]


@functools.lru_cache(maxsize=None)
def stretch_field(R):
    """The stretch scene (96 x 80, grid (7, s 8)) refined from the truth rounded to whole pixels."""
    scene = make_case_scene("stretch")
    u0, v0 = truth_at_nodes(scene, 7, 8)
    return scene, subset_refine_reference(scene.frame_0, scene.frame_1, u0, v0, 7, 8, R)


@functools.lru_cache(maxsize=None)
def small_field(R=3):
    """tests/test_subset_cpu.py's small case (50 x 41, grid (3, s 5)) refined: (f0, f1, the six planes, the state plane)."""
    f0, f1, u0, v0, r, s = small_case()
    got = subset_refine_reference(f0, f1, u0, v0, r, s, R)
    return f0, f1, refined_nodes(got), got.state, r, s


# ---- 1, 2: the exact properties -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 7, 11])
def test_both_frames_times_two_scales_nothing_but_the_noise(R):
    """Every operation scales by a power of two: the sigmas and rho keep their bytes, the noise doubles exactly."""
    scene, field = stretch_field(7)
    nodes = refined_nodes(field)
    one = subset_uncertainty_reference(scene.frame_0, scene.frame_1, nodes, field.state, 7, 8, R)
    two = subset_uncertainty_reference(scene.frame_0 * F32(2), scene.frame_1 * F32(2), nodes, field.state, 7, 8, R)
    assert int(one.record["evaluated"][0]) >= 63 and one.record.tobytes() == two.record.tobytes()
    for name in PLANES[:7]:
        assert np.array_equal(bits(getattr(one, name)), bits(getattr(two, name))), name
    live = one.fate == EVALUATED
    assert np.array_equal(two.noise[live], one.noise[live] * F32(2)) and (one.noise[live] > 0).all()


@pytest.mark.parametrize("interpolation", [0, 1])
def test_a_pair_that_matches_exactly_has_sigma_zero(interpolation):
    """Frame 1 is frame 0 rolled by whole pixels and p that shift as exact integers: the Catmull-Rom weights at t = 0 are exactly
    0, 1, 0, 0, so g = f, q = 1, every residual is 0: every sigma and the noise are +0.0, rho is finite.  (The B-spline sample of
    the coefficients gives f back only up to the prefilter's rounding: there the sigmas are tiny, not zero.)"""
    f0 = make_case_scene("stretch").frame_0
    f1 = np.roll(f0, (2, -3), axis=(0, 1))  # frame_1[y][x] = frame_0[y - 2][x + 3]: u = -3, v = 2
    nw, nh = grid(96, 80, 7, 8)
    zero = np.zeros((nh, nw), F32)
    nodes = [np.full((nh, nw), -3, F32), np.full((nh, nw), 2, F32), zero, zero, zero, zero]
    second = bspline_prefilter_reference(f1) if interpolation else f1
    got = subset_uncertainty_reference(f0, second, nodes, np.ones((nh, nw), F32), 7, 8, 3, interpolation=interpolation)
    live = got.fate == EVALUATED
    assert live.sum() >= 63 and set(got.fate[~live]) <= {OUTSIDE}
    assert np.isfinite(got.rho[live]).all() and (np.abs(got.rho[live]) < 1).all()
    if interpolation == 0:
        for name in PLANES[:2] + PLANES[3:]:
            assert (bits(getattr(got, name))[live] == 0).all(), name  # +0.0
    else:
        assert (got.sigma_u[live] < 1e-5).all() and (got.noise[live] < 1e-3).all()


# ---- 3: calibration -------------------------------------------------------------------------------------------------------------------
CALIBRATION_ROWS = (("translation", 2.0, 7), ("stretch", 2.0, 7), ("rotation", 4.0, 7), ("translation", 1.0, 11))
DRAWS, SEED, MARGIN = 24, 1, 6
PARAMETERS = ("u", "v", "ux", "uy", "vx", "vy")
SIGMA_OF = dict(zip(PARAMETERS, ("sigma_u", "sigma_v", "sigma_ux", "sigma_uy", "sigma_vx", "sigma_vy")))


def calibration_row(name, noise_sigma, R, refine=None, evaluate=None):
    """One row of profiles/subset_uncertainty/README.md's table: Gaussian noise of `noise_sigma` grey values on both frames, DRAWS
    draws from default_rng(SEED) (frame 0's noise first), the interior nodes at MARGIN, every draw refined from the truth rounded
    to whole pixels.  ratio = the predicted sigma, an RMS over nodes and draws, over the standard deviation of the refinement's
    output across the draws, pooled as an RMS over the nodes.  refine and evaluate stand in for the two restatements (the device
    rows of tools/uncertainty_table.py)."""
    r, s = 7, 8
    scene = make_case_scene(name)
    h, w = scene.frame_0.shape
    u0, v0 = truth_at_nodes(scene, r, s)
    nh, nw = u0.shape
    inside = interior_mask(nw, nh, w, h, r, MARGIN, s)
    u0 = np.where(inside, u0, F32(np.nan))  # (the other nodes are not refined: no input)
    refine = refine or (lambda f0, f1: subset_refine_reference(f0, f1, u0, v0, r, s, R))
    evaluate = evaluate or (lambda f0, f1, got: subset_uncertainty_reference(f0, f1, refined_nodes(got), got.state, r, s, R))
    rng = np.random.default_rng(SEED)
    found = {p: [] for p in PARAMETERS}
    predicted = {p: [] for p in PARAMETERS}
    noise = []
    for _ in range(DRAWS):
        f0 = (scene.frame_0.astype(F64) + rng.normal(0.0, noise_sigma, scene.frame_0.shape)).astype(F32)
        f1 = (scene.frame_1.astype(F64) + rng.normal(0.0, noise_sigma, scene.frame_1.shape)).astype(F32)
        got = refine(f0, f1)
        assert (got.state[inside] >= 1).all()
        sig = evaluate(f0, f1, got)
        for p in PARAMETERS:
            found[p].append(getattr(got, p)[inside].astype(F64))
            predicted[p].append(getattr(sig, SIGMA_OF[p])[inside].astype(F64))
        noise.append(sig.noise[inside].astype(F64))
    row = dict(scene=name, noise_sigma=noise_sigma, R=R, draws=DRAWS, seed=SEED, nodes=int(inside.sum()), ratio={}, predicted={}, observed={})
    for p in PARAMETERS:
        observed = np.sqrt(np.mean(np.var(np.stack(found[p]), axis=0, ddof=1)))
        pooled = np.sqrt(np.mean(np.stack(predicted[p]) ** 2))
        per_node = np.sqrt(np.mean(np.stack(predicted[p]) ** 2, axis=0)) / np.std(np.stack(found[p]), axis=0, ddof=1)
        row["predicted"][p], row["observed"][p], row["ratio"][p] = float(pooled), float(observed), float(pooled / observed)
        row.setdefault("per_node_ratio", {})[p] = [float(per_node.min()), float(per_node.max())]
    row["noise_over_root_two_sigma"] = float(np.mean(np.stack(noise)) / (np.sqrt(2.0) * noise_sigma))
    return row


@functools.lru_cache(maxsize=None)
def calibration_rows():
    return [calibration_row(*case) for case in CALIBRATION_ROWS]


def test_the_predicted_sigma_is_the_scatter_of_the_refinements_output():
    """The four rows: the pooled ratio of u and of v lies in 0.85 .. 1.30 -- the issue's measured 0.99 .. 1.15 with as much again
    on either side; a missing sqrt(2), a forgotten q or H in the wrong units falls outside.  Per-node ratios are sampling noise at
    24 draws and are not asserted."""
    rows = calibration_rows()
    for row in rows:
        print(json.dumps(row))
    os.makedirs(PROFILE_DIR, exist_ok=True)
    with open(CALIBRATION_PATH, "w") as fh:
        json.dump(dict(source="numpy restatement (tests/test_subset_uncertainty_cpu.py)", rows=rows), fh, indent=1, sort_keys=True)
        fh.write("\n")
    for row in rows:
        assert row["nodes"] == 63
        assert 0.85 <= row["ratio"]["u"] <= 1.30 and 0.85 <= row["ratio"]["v"] <= 1.30, row


# ---- 4: the degrees of freedom ----------------------------------------------------------------------------------------------------------
def test_at_radius_one_the_sigma_is_the_root_of_s_times_x():
    """N = 9, N - 8 = 1: s2 is S itself."""
    scene, field = stretch_field(7)
    nodes = refined_nodes(field)
    got = subset_uncertainty_reference(scene.frame_0, scene.frame_1, nodes, field.state, 7, 8, 1, order="sequential")
    j, i = 4, 5
    assert got.fate[j, i] == EVALUATED
    cx, cy = 7 + 8 * i, 7 + 8 * j
    f0, f1 = scene.frame_0.astype(F64), scene.frame_1.astype(F64)
    ys, xs = np.mgrid[cy - 1:cy + 2, cx - 1:cx + 2]
    ys, xs = ys.ravel(), xs.ravel()
    xi, eta = (xs - cx).astype(F64), (ys - cy).astype(F64)
    f = f0[ys, xs]
    fx, fy = (f0[ys, xs + 1] - f0[ys, xs - 1]) * 0.5, (f0[ys + 1, xs] - f0[ys - 1, xs]) * 0.5
    J = np.stack([fx, fx * xi, fx * eta, fy, fy * xi, fy * eta], axis=1)
    H = J.T @ J
    p = [F64(q[j, i]) for q in nodes]
    g = cubic_sample(f1, xs + (p[0] + p[2] * xi + p[3] * eta), ys + (p[1] + p[4] * xi + p[5] * eta))
    fd, gd = f - f.mean(), g - g.mean()
    res = fd - np.sqrt((fd * fd).sum() / (gd * gd).sum()) * gd
    S = (res * res).sum()
    inverse = np.linalg.inv(H)
    assert got.sigma_u[j, i] == pytest.approx(np.sqrt(S * inverse[0, 0]), rel=1e-5)
    assert got.sigma_v[j, i] == pytest.approx(np.sqrt(S * inverse[3, 3]), rel=1e-5)
    assert got.sigma_uy[j, i] == pytest.approx(np.sqrt(S * inverse[2, 2]), rel=1e-5)
    assert got.noise[j, i] == pytest.approx(np.sqrt(S), rel=1e-5)
    assert got.rho[j, i] == pytest.approx(inverse[0, 3] / np.sqrt(inverse[0, 0] * inverse[3, 3]), rel=1e-4, abs=1e-6)


def thin_mask(shape, cx, cy, usable):
    """Everything excluded but a block around (cx, cy) that leaves `usable` = 8 or 9 usable pixels in a subset of radius 3 or more."""
    rows, cols = {8: (4, 6), 9: (5, 5)}[usable]
    return block_mask(shape, cx, cy, rows, cols)


def test_eight_usable_pixels_are_thin_and_nine_are_evaluated():
    f0, f1, nodes, state, r, s = small_field()
    cx, cy = r + 4 * s, r + 3 * s  # node (3, 4)
    for usable, fate in ((8, THIN), (9, EVALUATED)):
        mask = thin_mask(f0.shape, cx, cy, usable)
        assert usable_plane(mask)[cy - 3:cy + 4, cx - 3:cx + 4].sum() == usable
        got = subset_uncertainty_reference(f0, f1, nodes, state, r, s, 3, mask=mask, min_pixels=6)
        assert got.fate[3, 4] == fate and (got.fate == MASKED).sum() == state.size - 1
        assert int(got.record["thin"][0]) == (usable == 8) and int(got.record["evaluated"][0]) == (usable == 9)
        assert np.isfinite(got.sigma_u[3, 4]) == (usable == 9)
    # min_pixels above Nv: masked before thin
    got = subset_uncertainty_reference(f0, f1, nodes, state, r, s, 3, mask=thin_mask(f0.shape, cx, cy, 8), min_pixels=9)
    assert got.fate[3, 4] == MASKED and int(got.record["masked"][0]) == state.size


# ---- 5: states and record -------------------------------------------------------------------------------------------------------------
def test_every_early_exit_gives_nan_planes_and_its_count():
    f0, f1, nodes, state, r, s = small_field()
    nodes, state = [q.copy() for q in nodes], state.copy()
    nh, nw = state.shape
    base = subset_uncertainty_reference(f0, f1, nodes, state, r, s, 3)
    strayed = int((state < 1).sum())  # (six nodes of the top row strayed in the refinement: skipped here at either min_state)
    assert strayed == 6 and (state[1:] >= 1).all()
    assert np.array_equal(base.fate == EVALUATED, state >= 1) and base.record.tolist() == [(nh * nw, nh * nw - strayed, strayed, 0, 0, 0, 0, 0)]
    state[1, 1], state[1, 2], state[1, 3], state[1, 4], state[1, 5] = -3, 0, np.nan, 65, 66  # strayed, unconverged, NaN; predicted, composed
    nodes[3][2, 2], nodes[0][2, 3] = np.nan, np.inf  # an input that is not finite
    nodes[0][3, 3] = 1e30                            # positions leave frame 1
    f0, f1 = f0.copy(), f1.copy()
    cx, cy = r + 6 * s, r + 5 * s
    f0[cy - 3:cy + 4, cx - 3:cx + 4] = 7.0           # node (5, 6): a constant subset, flat by Df2
    f0[cy - 4, cx - 4:cx + 5], f0[cy + 4, cx - 4:cx + 5], f0[cy - 4:cy + 5, cx - 4], f0[cy - 4:cy + 5, cx + 4] = 7.0, 7.0, 7.0, 7.0
    cx1, cy1 = r + 1 * s, r + 5 * s
    f1[cy1 - 5:cy1 + 6, cx1 - 4:cx1 + 7] = 0.0       # node (5, 1): frame 1 is 0 under its subset (every sample exactly 0), flat by Dg2
    mask = np.zeros(f0.shape, F32)
    mask[r + 6 * s, r + 1 * s] = 1                    # the centre of node (6, 1) ...
    nodes[0][6, 1] = np.nan                           # ... masked comes before skipped
    mask[r + 4 * s - 3:r + 4 * s + 4, r + 7 * s - 3:r + 7 * s + 4] = np.nan
    mask[r + 4 * s, r + 7 * s] = 0                    # node (4, 7): the centre alone is clean, Nv = 0: masked by count
    for min_state, skipped_states in ((1, 3), (0, 2)):
        got = subset_uncertainty_reference(f0, f1, nodes, state, r, s, 3, min_state=min_state, mask=mask, min_pixels=6)
        want = {(1, 1): SKIPPED, (1, 2): SKIPPED if min_state else EVALUATED, (1, 3): SKIPPED, (1, 4): EVALUATED, (1, 5): EVALUATED,
                (2, 2): SKIPPED, (2, 3): SKIPPED, (3, 3): OUTSIDE, (5, 6): FLAT, (5, 1): FLAT, (6, 1): MASKED, (4, 7): MASKED}
        for (j, i), fate in want.items():
            assert got.fate[j, i] == fate, (j, i, got.fate[j, i], fate)
        early = got.fate != EVALUATED
        for plane in got.planes():
            assert (bits(plane)[early] == NAN_BITS).all() and np.isfinite(plane[~early]).all()
        rec = got.record[0]
        assert rec["skipped"] == strayed + skipped_states + 2 and rec["masked"] == 2 and rec["outside"] == 1 and rec["flat"] == 2 and rec["thin"] == 0
        assert rec["evaluated"] == nh * nw - early.sum() and rec["nodes"] == nh * nw and rec["reserved"] == 0
    # R = 6 > r: the border nodes are outside by the frame-0 window test, whatever the mask holds beside their centres
    got = subset_uncertainty_reference(f0, f1, nodes, state, r, s, 6, mask=mask, min_pixels=6)
    assert got.fate[0, 0] == SKIPPED and got.fate[0, 1] == OUTSIDE and got.fate[3, 0] == OUTSIDE and got.fate[6, 1] == MASKED
    assert int(got.record["outside"][0]) >= 8


# ---- 6: the summation order -----------------------------------------------------------------------------------------------------------
def test_the_three_orders_agree_and_their_spread_is_recorded():
    f0, f1, nodes, state, r, s = small_field()
    spreads = {}
    cases = (("small, R = 3", dict()), ("small, R = 3, random mask", dict(mask=random_mask(f0.shape, 0.1), min_pixels=6)),
             ("small, R = 6", dict()))
    for (label, kw), R in zip(cases, (3, 3, 6)):
        got, spreads[label] = all_orders_uncertainty(f0, f1, nodes, state, r, s, R, **kw)
        assert (got.fate == EVALUATED).sum() >= 8
    scene, field = stretch_field(7)
    for interpolation in (0, 1):
        second = bspline_prefilter_reference(scene.frame_1) if interpolation else scene.frame_1
        got, spreads["stretch, R = 7, interpolation %d" % interpolation] = all_orders_uncertainty(
            scene.frame_0, second, refined_nodes(field), field.state, 7, 8, 7, interpolation=interpolation)
        assert np.array_equal(got.fate == EVALUATED, field.state >= 1) and (got.fate == EVALUATED).sum() == 81
    print(json.dumps(spreads))
    os.makedirs(PROFILE_DIR, exist_ok=True)
    with open(SPREAD_PATH, "w") as fh:
        json.dump(dict(what="largest relative spread of an output between the sequential, reversed and butterfly orders", spread=spreads),
                  fh, indent=1, sort_keys=True)
        fh.write("\n")
    assert max(spreads.values()) < 1e-9  # (orders of magnitude below an fp32 ulp: the planes can differ only at a rounding boundary)


# ---- 7: the entry's host side ---------------------------------------------------------------------------------------------------------
def test_uncertainty_refusals_without_a_device(flow2d):
    lib = flow2d.hip_lib()
    fake = ctypes.create_string_buffer(4096)
    w, h, pitch, npitch = 100, 40, 512, 64
    span = pitch * h
    at = lambda k: (1 << 20) + k * (span + 4096)  # noqa: E731  (addresses only: nothing is dereferenced before the device is entered)
    ins = ("u", "v", "ux", "uy", "vx", "vy", "state")
    outs = ("su", "sv", "rho", "sux", "suy", "svx", "svy", "noise")
    d = dict(ctx=ctypes.addressof(fake), f0=at(0), f1=at(1), interpolation=0, w=w, h=h, pitch=pitch, nw=11, nh=4, npitch=npitch, r=7, s=8,
             R=7, min_state=1, mask=at(2), min_pixels=57, record=at(3), **{n: at(4 + k) for k, n in enumerate(ins + outs)})

    def call(**kw):
        a = dict(d, **kw)
        return lib.flow2d_subset_uncertainty_2d(a["ctx"], a["f0"], a["f1"], a["interpolation"], a["w"], a["h"], a["pitch"], *[a[n] for n in ins],
                                                a["nw"], a["nh"], a["npitch"], a["r"], a["s"], a["R"], a["min_state"], a["mask"],
                                                a["min_pixels"], *[a[n] for n in outs], a["record"])

    bad = [dict(ctx=None), dict(f0=None), dict(f1=None), dict(w=0), dict(nh=0), dict(pitch=pitch + 8), dict(npitch=32), dict(r=0), dict(s=65),
           dict(R=0), dict(R=16), dict(nw=12), dict(interpolation=2), dict(interpolation=-1), dict(min_state=2), dict(min_state=-1),
           dict(su=None), dict(sv=None), dict(sux=None), dict(suy=None, svx=None, svy=None), dict(record=at(3) + 4),
           dict(min_pixels=5), dict(min_pixels=226), dict(R=1, min_pixels=10), dict(mask=at(2) + 4)]
    bad += [{n: None} for n in ins]
    bad += [dict(su=at(0)), dict(sv=at(1)), dict(rho=at(2)), dict(noise=d["su"]), dict(svy=d["state"]), dict(sux=d["ux"]),
            dict(record=d["u"]), dict(record=d["noise"]), dict(su=at(2) + span - pitch), dict(record=at(1) + 64)]
    bad += [dict(mask=None, min_pixels=0, **kw) for kw in (dict(f1=None), dict(h=14), dict(su=at(1)), dict(R=16), dict(state=None))]
    for kw in bad:
        assert call(**kw) == 1, kw
    # (only refusals here: an accepted call would go on to launch on these made-up addresses where there is a device)


def test_python_record_and_plane_names(flow2d):
    assert flow2d.SUBSET_UNCERTAINTY_PLANES == PLANES and ctypes.sizeof(flow2d.UncertaintyRecord) == 64
    rec = flow2d.UncertaintyRecord()
    rec.nodes, rec.thin = 9, 4
    assert np.frombuffer(bytes(rec), UNCERTAINTY_DTYPE)["thin"][0] == 4 and list(rec.summary()) == list(UNCERTAINTY_DTYPE.names[:7])
    assert [name for name, _ in flow2d.UncertaintyRecord._fields_] == list(UNCERTAINTY_DTYPE.names)
