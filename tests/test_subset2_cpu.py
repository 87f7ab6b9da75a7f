"""flow2d_subset_refine2_2d restated in numpy from the text of include/flow2d_c_abi.h -- node by node, in float64, every operation of
the header spelled out, the order of a sum over the subset pluggable as in test_subset_cpu (sequential, reversed, the device's
butterfly).  What can be checked without a device: the accuracy on the two bending scenes against the first-order restatement
on the same starts, that an affine scene loses nothing, that the three orders agree on every state (their spread goes to
profiles/subset2/order_spread.json), the degenerate inputs and the entry's host-side refusals."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from test_correlate_cpu import F32, NAN_BITS, bits, correlate_reference, frame_range, grid, random_frames, scenes_module
from test_subset_cpu import FLAT, NO_INPUT, ORDERS, ROOT, STRAYED, SUBSET_DTYPE, SUMS, cubic_sample, subset_refine_reference

F64 = np.float64
SPREAD_PATH = os.path.join(ROOT, "profiles", "subset2", "order_spread.json")
P_NAMES = ("u", "ux", "uy", "uxx", "uxy", "uyy", "v", "vx", "vy", "vxx", "vxy", "vyy")  # the order of p
GRADIENTS, CURVATURES = ("ux", "uy", "vx", "vy"), ("uxx", "uxy", "uyy", "vxx", "vxy", "vyy")


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def cholesky12(H):
    """L of the header, or None where a pivot fails its test."""
    L = np.zeros((12, 12), F64)
    for k in range(12):
        acc = F64(0)
        for m in range(k):
            acc = acc + L[k, m] * L[k, m]
        d = H[k, k] - acc
        if not d > F64(1e-10) * H[k, k]:
            return None
        L[k, k] = np.sqrt(d)
        for i in range(k + 1, 12):
            acc = F64(0)
            for m in range(k):
                acc = acc + L[i, m] * L[k, m]
            L[i, k] = (H[i, k] - acc) / L[k, k]
    return L


def solve12(L, b):
    y, x = np.zeros(12, F64), np.zeros(12, F64)
    for i in range(12):
        acc = F64(0)
        for m in range(i):
            acc = acc + L[i, m] * y[m]
        y[i] = (b[i] - acc) / L[i, i]
    for i in range(11, -1, -1):
        acc = F64(0)
        for m in range(i + 1, 12):
            acc = acc + L[m, i] * x[m]
        x[i] = (y[i] - acc) / L[i, i]
    return x


def rows_ab(q):
    """A(q), B(q) of the header."""
    u, ux, uy, uxx, uxy, uyy, v, vx, vy, vxx, vxy, vyy = q
    return ([F64(0.5) * uxx, uxy, F64(0.5) * uyy, F64(1) + ux, uy, u], [F64(0.5) * vxx, vxy, F64(0.5) * vyy, vx, F64(1) + vy, v])


def compose(p, dp):
    """Step 4 of the header: the new p, or None where a pivot fails its test."""
    a, b = rows_ab(dp)
    two = F64(2)

    def square(a):
        return [a[3] * a[3] + two * (a[0] * a[5]), two * (a[3] * a[4]) + two * (a[1] * a[5]), a[4] * a[4] + two * (a[2] * a[5]),
                two * (a[3] * a[5]), two * (a[4] * a[5]), a[5] * a[5]]

    W = [square(a),
         [(a[3] * b[3] + a[0] * b[5]) + a[5] * b[0], ((a[3] * b[4] + a[4] * b[3]) + a[1] * b[5]) + a[5] * b[1],
          (a[4] * b[4] + a[2] * b[5]) + a[5] * b[2], a[3] * b[5] + a[5] * b[3], a[4] * b[5] + a[5] * b[4], a[5] * b[5]],
         square(b), a, b]
    M = [[W[i][j] for i in range(5)] for j in range(5)]
    rhs = [list(r) for r in rows_ab(p)]
    for k in range(5):
        if not abs(M[k][k]) > 1e-6:
            return None
        for j in range(k + 1, 5):
            f = M[j][k] / M[k][k]
            for i in range(k + 1, 5):
                M[j][i] = M[j][i] - f * M[k][i]
            for r in rhs:
                r[j] = r[j] - f * r[k]
    zs = []
    for r in rhs:
        z = [F64(0)] * 6
        for i in range(4, -1, -1):
            acc = F64(0)
            for m in range(i + 1, 5):
                acc = acc + M[i][m] * z[m]
            z[i] = (r[i] - acc) / M[i][i]
        z[5] = r[5] - ((((z[0] * W[0][5] + z[1] * W[1][5]) + z[2] * W[2][5]) + z[3] * W[3][5]) + z[4] * W[4][5])
        zs.append(z)
    za, zb = zs
    return np.array([za[5], za[3] - F64(1), za[4], two * za[0], za[1], two * za[2],
                     zb[5], zb[3], zb[4] - F64(1), two * zb[0], zb[1], two * zb[2]], F64)


def refine2_node(f0, f1, cx, cy, start, R, K, epsilon, max_shift, max_gradient, max_curvature, total):
    """(state, p, c, iterations begun) of one node with a finite start (float64, the order of p); f0, f1 float64."""
    h, w = f0.shape
    side = 2 * R + 1
    n = F64(side * side)
    k = np.arange(side * side)
    kx, ky = k % side - R, k // side - R
    xi, eta = kx.astype(F64), ky.astype(F64)
    p = np.array(start, F64)
    u0, v0 = p[0], p[6]
    if not (cx - R >= 0 and cy - R >= 0 and cx + R <= w - 1 and cy + R <= h - 1):
        return STRAYED, p, F64(0), 0
    xs, ys = cx + kx, cy + ky
    f = f0[ys, xs]
    fx = (f0[ys, np.minimum(xs + 1, w - 1)] - f0[ys, np.maximum(xs - 1, 0)]) * 0.5
    fy = (f0[np.minimum(ys + 1, h - 1), xs] - f0[np.maximum(ys - 1, 0), xs]) * 0.5
    fd = f - total(f) / n
    df2 = total(fd * fd)
    if not df2 > 0:
        return FLAT, p, F64(0), 0
    df = np.sqrt(df2)
    phi = np.stack([np.ones_like(xi), xi, eta, 0.5 * xi * xi, xi * eta, 0.5 * eta * eta], axis=1)
    pair = phi[:, :, None] * phi[:, None, :]  # exact, and symmetric bit for bit
    H = np.zeros((12, 12), F64)
    H[:6, :6] = total((fx * fx)[:, None, None] * pair)
    H[6:, :6] = total((fx * fy)[:, None, None] * pair)
    H[:6, 6:] = H[6:, :6].T
    H[6:, 6:] = total((fy * fy)[:, None, None] * pair)
    L = cholesky12(H)
    if L is None:
        return FLAT, p, F64(0), 0
    J = np.concatenate([fx[:, None] * phi, fy[:, None] * phi], axis=1)
    c = F64(0)
    radius = F64(R)
    r2 = F64(R * R)
    hr2 = F64(0.5) * r2
    scale = np.array([1, radius, radius, hr2, r2, hr2] * 2, F64)
    for it in range(1, K + 1):
        X = xs.astype(F64) + (((((p[0] + p[1] * phi[:, 1]) + p[2] * phi[:, 2]) + p[3] * phi[:, 3]) + p[4] * phi[:, 4]) + p[5] * phi[:, 5])
        Y = ys.astype(F64) + (((((p[6] + p[7] * phi[:, 1]) + p[8] * phi[:, 2]) + p[9] * phi[:, 3]) + p[10] * phi[:, 4]) + p[11] * phi[:, 5])
        if not ((X >= 0) & (X <= w - 1) & (Y >= 0) & (Y <= h - 1)).all():
            return STRAYED, p, c, it
        g = cubic_sample(f1, X, Y)
        gd = g - total(g) / n
        dg2 = total(gd * gd)
        if not dg2 > 0:
            return FLAT, p, c, it
        dg = np.sqrt(dg2)
        c = total(fd * gd) / (df * dg)
        res = fd - (df / dg) * gd
        dp = -solve12(L, total(J * res[:, None]))
        new = compose(p, dp)
        if new is None:
            return STRAYED, p, c, it
        p = new
        if not (abs(p[0] - u0) <= max_shift and abs(p[6] - v0) <= max_shift and all(abs(p[i]) <= max_gradient for i in (1, 2, 7, 8)) and
                all(abs(p[i]) <= max_curvature for i in (3, 4, 5, 9, 10, 11))):
            return STRAYED, p, c, it
        t = scale * dp
        acc = t[0] * t[0]
        for i in range(1, 12):
            acc = acc + t[i] * t[i]
        if np.sqrt(acc) < epsilon:
            return it, p, c, it
    return 0, p, c, K


class Refined2:
    """The outputs of flow2d_subset_refine2_2d: the twelve planes by the names of P_NAMES, score, state (float32), the record, and
    p64 -- p in float64 where the state is >= 0, NaN elsewhere -- for the spread between orders."""
    NAMES = P_NAMES + ("score", "state")

    def planes(self):
        return [getattr(self, name) for name in self.NAMES]


def subset_refine2_reference(frame_0, frame_1, node_u0, node_v0, r, s, R, K=20, epsilon=1e-3, max_shift=2.0, max_gradient=0.5,
                             max_curvature=0.05, start_gradients=None, start_curvatures=None, order="butterfly"):
    f0, f1 = np.asarray(frame_0, F32).astype(F64), np.asarray(frame_1, F32).astype(F64)
    node_u0 = np.asarray(node_u0, F32)
    nh, nw = node_u0.shape
    given = {"u": node_u0, "v": np.asarray(node_v0, F32)}
    given.update(zip(GRADIENTS, start_gradients or ()))
    given.update(zip(CURVATURES, start_curvatures or ()))
    start = np.stack([np.asarray(given.get(name, np.zeros((nh, nw), F32)), F32) for name in P_NAMES])
    epsilon, max_shift, max_gradient, max_curvature = (F64(F32(x)) for x in (epsilon, max_shift, max_gradient, max_curvature))
    out = Refined2()
    planes = np.zeros((14, nh, nw), F32)
    out.p64 = np.full((nh, nw, 12), np.nan)
    record = np.zeros(1, SUBSET_DTYPE)
    record["nodes"] = nh * nw
    with np.errstate(all="ignore"):
        for j in range(nh):
            for i in range(nw):
                if not np.isfinite(start[:, j, i]).all():
                    planes[:12, j, i] = np.nan
                    planes[13, j, i] = NO_INPUT
                    record["no_input"] += 1
                    continue
                state, p, c, begun = refine2_node(f0, f1, r + i * s, r + j * s, start[:, j, i].astype(F64), R, K, epsilon, max_shift,
                                                  max_gradient, max_curvature, SUMS[order])
                record["iterations"] += begun
                planes[13, j, i] = state
                if state >= 0:
                    planes[:12, j, i] = p.astype(F32)
                    planes[12, j, i] = F32(c)
                    out.p64[j, i] = p
                    record["converged" if state >= 1 else "unconverged"] += 1
                else:
                    planes[:12, j, i] = start[:, j, i]
                    record["flat" if state == FLAT else "strayed"] += 1
    nan = bits(planes[:12])
    nan[np.isnan(planes[:12])] = NAN_BITS
    planes[:12] = nan.view(F32)
    for name, plane in zip(Refined2.NAMES, planes):
        setattr(out, name, plane)
    out.record = record
    return out


def all_orders2(frame_0, frame_1, node_u0, node_v0, r, s, R, **kw):
    """(the butterfly order's result, the largest spread of p between the three orders); the orders must agree on every state."""
    runs = [subset_refine2_reference(frame_0, frame_1, node_u0, node_v0, r, s, R, order=o, **kw) for o in ORDERS]
    for other in runs[:2]:
        assert np.array_equal(other.state, runs[2].state) and other.record.tobytes() == runs[2].record.tobytes()
    stack = np.stack([q.p64 for q in runs])
    live = np.isfinite(stack[2])
    spread = float((stack.max(0) - stack.min(0))[live].max()) if live.any() else 0.0
    return runs[2], spread


# ---- the scenes -------------------------------------------------------------------------------------------------------------------
BENDING_CASES = [("bend", 7), ("bend", 11), ("bulge", 7), ("bulge", 11)]
GRID_R, GRID_S, SEARCH = 7, 8, 6


def scored_mask(nw, nh, width, height, R):
    """The nodes whose subset, grown by the search range, lies inside the frame."""
    cx, cy = GRID_R + np.arange(nw) * GRID_S, GRID_R + np.arange(nh) * GRID_S
    m = R + SEARCH
    return ((cy >= m) & (cy <= height - 1 - m))[:, None] & ((cx >= m) & (cx <= width - 1 - m))[None, :]


def node_epe(u, v, scene):
    nh, nw = u.shape
    cy, cx = GRID_R + np.arange(nh) * GRID_S, GRID_R + np.arange(nw) * GRID_S
    return np.hypot(u.astype(F64) - scene.gt_u[np.ix_(cy, cx)], v.astype(F64) - scene.gt_v[np.ix_(cy, cx)])


def make_scene(name):
    sc = scenes_module()
    return sc.make_speckle_bending(name) if name in ("bend", "bulge") else sc.make_speckle_deformation(name)


@functools.lru_cache(maxsize=None)
def scene_starts(name):
    scene = make_scene(name)
    lo, scale = frame_range(scene.frame_0, scene.frame_1)
    u0, v0, _, _, _ = correlate_reference(scene.frame_0, scene.frame_1, lo, scale, GRID_R, SEARCH, GRID_S)
    return scene, u0, v0


def scene_figures(name, R, refine2=None):
    """The figures of one row of profiles/subset2/table*.md: order 1 (the restatement of flow2d_subset_refine_2d) and order 2 on the
    same starts; refine2: the device's refinement in place of the restatement's (tools/subset2_table.py)."""
    scene, u0, v0 = scene_starts(name)
    first = subset_refine_reference(scene.frame_0, scene.frame_1, u0, v0, GRID_R, GRID_S, R)
    if refine2 is None:
        second, spread = all_orders2(scene.frame_0, scene.frame_1, u0, v0, GRID_R, GRID_S, R)
    else:
        second, spread = refine2(scene.frame_0, scene.frame_1, u0, v0, GRID_R, GRID_S, R), None
    nh, nw = u0.shape
    scored = scored_mask(nw, nh, 96, 80, R)
    e1, e2 = node_epe(first.u, first.v, scene)[scored], node_epe(second.u, second.v, scene)[scored]
    s1, s2 = first.state[scored], second.state[scored]
    curvature = {name: float(getattr(second, name)[scored].astype(F64).mean()) for name in CURVATURES}
    return dict(scene=name, R=R, nodes=int(scored.sum()), order1_mean_epe=float(e1.mean()), order1_max_epe=float(e1.max()),
                order2_mean_epe=float(e2.mean()), order2_max_epe=float(e2.max()), order1_converged=int((s1 >= 1).sum()),
                order2_converged=int((s2 >= 1).sum()), order1_iterations=float(s1[s1 >= 1].mean()) if (s1 >= 1).any() else 0.0,
                order2_iterations=float(s2[s2 >= 1].mean()) if (s2 >= 1).any() else 0.0, mean_curvature=curvature, spread=spread)


@functools.lru_cache(maxsize=None)
def scene_rows(name, R):
    return scene_figures(name, R)


@pytest.mark.parametrize("name,R", BENDING_CASES)
def test_accuracy_on_the_bending_scenes(name, R):
    """96 x 80 speckle, kappa = 0.004, translation (1.6, -0.7), the grid (7, s 8), starts from flow2d_correlate_2d's restatement at
    d = 6 with zero gradients and curvatures, scored on the nodes whose subset grown by d lies inside the frame: every scored
    node converges at order 2, whose mean endpoint error is below half the first-order restatement's on the same starts and
    below 0.02 px; the three summation orders give the same state at every node (all_orders2 asserts it)."""
    row = scene_rows(name, R)
    print(json.dumps(row))
    assert row["nodes"] == (63 if R == 7 else 35) and row["order2_converged"] == row["nodes"]
    assert row["order2_mean_epe"] < 0.5 * row["order1_mean_epe"]
    assert row["order2_mean_epe"] < 0.02
    assert row["spread"] < 1e-9


def test_an_affine_scene_loses_nothing():
    """make_speckle_deformation("stretch"): order 2 converges every interior node and its mean endpoint error is at most twice
    order 1's."""
    row = scene_rows("stretch", 7)
    print(json.dumps(row))
    assert row["order2_converged"] == row["nodes"] == 63
    assert row["order2_mean_epe"] <= 2.0 * row["order1_mean_epe"]


def test_order_spread_is_recorded():
    """The largest spread of p under the three orders, per scene and R, printed and written to profiles/subset2/order_spread.json."""
    spread = {"%s R=%d" % (name, R): float("%.3e" % scene_rows(name, R)["spread"]) for name, R in BENDING_CASES + [("stretch", 7)]}
    print(json.dumps(spread))
    text = json.dumps({"what": "largest |p(order a) - p(order b)| over the nodes with state >= 0, float64; orders: " + ", ".join(ORDERS),
                       "grid": "96 x 80, r = 7, s = 8", "spread": spread}, indent=1, sort_keys=True) + "\n"
    if not os.path.exists(SPREAD_PATH) or open(SPREAD_PATH).read() != text:
        try:  # (the committed file holds these figures already; a tree that cannot be written keeps it)
            os.makedirs(os.path.dirname(SPREAD_PATH), exist_ok=True)
            with open(SPREAD_PATH, "w") as out:
                out.write(text)
        except OSError as e:
            print("not written: %s" % e)
    assert max(spread.values()) < 1e-9


def test_bending_scenes():
    sc = scenes_module()
    assert sc.SPECKLE_BENDINGS == ("bend", "bulge")
    assert not set(sc.SPECKLE_BENDINGS) & (set(sc.SPECKLE_MOTIONS) | set(sc.SPECKLE_DEFORMATIONS))
    for name in sc.SPECKLE_BENDINGS:
        scene = sc.make_speckle_bending(name, 48, 40, seed=2, kappa=0.004)
        # the centre moves by the translation (and kappa times a product of offsets of a pixel or two: below 0.02), and frame 1
        # holds frame 0's content at the ground truth
        assert abs(scene.gt_u[19:21, 23:25].mean() - 1.6) < 0.02 and abs(scene.gt_v[19:21, 23:25].mean() + 0.7) < 0.02
        ys, xs = np.mgrid[5:35, 5:43].astype(F64)
        there = scene.frame_1_at(xs + scene.gt_u[5:35, 5:43].astype(F64), ys + scene.gt_v[5:35, 5:43].astype(F64))
        assert np.abs(there - scene.frame_0[5:35, 5:43]).max() < 1e-3
        # the second derivatives of the displacement are kappa where the field has them
        gu, gv = scene.gt_u.astype(F64), scene.gt_v.astype(F64)
        uxx, vyy = np.gradient(np.gradient(gu, axis=1), axis=1)[10:30, 10:38], np.gradient(np.gradient(gv, axis=0), axis=0)[10:30, 10:38]
        uxy, vxx = np.gradient(np.gradient(gu, axis=1), axis=0)[10:30, 10:38], np.gradient(np.gradient(gv, axis=1), axis=1)[10:30, 10:38]
        want = dict(bend=(0.0, 0.004, -0.004, 0.0), bulge=(0.004, 0.0, 0.0, 0.004))[name]
        for got, w in zip((uxx, uxy, vxx, vyy), want):
            assert abs(got.mean() - w) < 4e-4, (name, got.mean(), w)
    with pytest.raises(ValueError):
        sc.make_speckle_bending("stretch")


# ---- degenerate inputs ------------------------------------------------------------------------------------------------------------
def small_case(seed=17, w=50, h=41, r=3, s=5):
    f0, f1 = random_frames(w, h, seed=seed, shift=(1, 0), noise=2.0)
    nw, nh = grid(w, h, r, s)
    return f0, f1, np.full((nh, nw), 1, F32), np.zeros((nh, nw), F32), r, s


def test_degenerate_inputs():
    f0, f1, u0, v0, r, s = small_case()
    zero = np.zeros_like(u0)
    # a constant frame 0: flat everywhere, the start copied (absent values 0), score 0
    got = subset_refine2_reference(np.full_like(f0, 7.0), f1, u0, v0, r, s, 3)
    assert (got.state == FLAT).all() and np.array_equal(bits(got.u), bits(u0)) and (got.score == 0).all()
    assert all((getattr(got, n) == 0).all() and not np.signbit(getattr(got, n)).any() for n in GRADIENTS + CURVATURES)
    assert got.record.tolist() == [(u0.size, 0, 0, 0, u0.size, 0, 0, 0)]
    # f1 = f0 with a zero start: the residual is exactly 0, the node converges at n = 1 with p = 0 and score 1
    for order in ORDERS:
        got = subset_refine2_reference(f0, f0, zero, zero, r, s, 3, order=order)
        assert (got.state == 1).all() and (got.score == 1).all() and got.record["iterations"][0] == u0.size
        assert all((getattr(got, n) == 0).all() for n in P_NAMES)
    # a NaN in each start plane in turn: that node alone has no input, all twelve NaN
    base = subset_refine2_reference(f0, f1, u0, v0, r, s, 3, start_gradients=[zero] * 4, start_curvatures=[zero] * 6)
    assert (base.state[1:-1, 1:-1] >= 1).all()
    for which in range(12):
        start = [u0.copy() if n == "u" else zero.copy() for n in P_NAMES]
        start[which][3, 4] = np.nan if which % 2 else np.inf
        got = subset_refine2_reference(f0, f1, start[0], start[6], r, s, 3, start_gradients=[start[k] for k in (1, 2, 7, 8)],
                                       start_curvatures=[start[k] for k in (3, 4, 5, 9, 10, 11)])
        assert got.state[3, 4] == NO_INPUT and got.record["no_input"][0] == 1 and got.score[3, 4] == 0
        assert all(bits(getattr(got, n))[3, 4] == NAN_BITS for n in P_NAMES)
        others = np.ones_like(u0, bool)
        others[3, 4] = False
        assert all(np.array_equal(bits(getattr(got, n))[others], bits(getattr(base, n))[others]) for n in Refined2.NAMES)
    # a start curvature beyond the bound strays in iteration 1 and comes back bit for bit
    far = zero.copy()
    far[3, 4] = 0.2
    got = subset_refine2_reference(f0, f1, u0, v0, r, s, 3, start_gradients=[zero] * 4, start_curvatures=[zero, far, zero, zero, zero, zero])
    assert got.state[3, 4] == STRAYED and got.uxy[3, 4] == F32(0.2) and got.u[3, 4] == 1 and got.uxx[3, 4] == 0 and got.score[3, 4] == 0
    # epsilon = 0: exactly K iterations, state 0
    got = subset_refine2_reference(f0, f1, u0, v0, r, s, 3, K=5, epsilon=0.0)
    inner = got.state[1:-1, 1:-1]
    assert (inner == 0).all() and got.record["converged"][0] == 0 and got.record["iterations"][0] >= 5 * inner.size
    assert got.record["nodes"][0] == sum(int(got.record[k][0]) for k in ("converged", "unconverged", "strayed", "flat", "no_input"))


def test_the_three_orders_agree_on_the_gpu_tests_input():
    f0, f1, u0, v0, r, s = small_case()
    got, spread = all_orders2(f0, f1, u0, v0, r, s, 3)
    print("spread %.3e" % spread)
    assert spread < 1e-9


def test_with_zero_curvature_the_update_is_the_affine_one():
    """The truncated 6 x 6 algebra with all curvatures 0 is the composition of two affine maps, up to rounding."""
    rng = np.random.default_rng(3)
    for _ in range(20):
        p, dp = rng.uniform(-0.2, 0.2, 12), rng.uniform(-0.05, 0.05, 12)
        p[[3, 4, 5, 9, 10, 11]] = dp[[3, 4, 5, 9, 10, 11]] = 0
        got = compose(p, dp)
        full = lambda q: np.array([[1 + q[1], q[2], q[0]], [q[7], 1 + q[8], q[6]], [0, 0, 1]])  # noqa: E731
        want = full(p) @ np.linalg.inv(full(dp))
        assert np.allclose([got[1] + 1, got[2], got[0], got[7], got[8] + 1, got[6]], want[:2].ravel(), atol=1e-12)
        assert np.abs(got[[3, 4, 5, 9, 10, 11]]).max() < 1e-15


# ---- the entry's host side ----------------------------------------------------------------------------------------------------------
def test_refusals_without_a_device(flow2d):
    lib = flow2d.hip_lib()
    fake = ctypes.create_string_buffer(4096)
    w, h, pitch, npitch = 100, 40, 512, 64
    span = pitch * h
    at = lambda k: (1 << 20) + k * (span + 4096)  # noqa: E731  (addresses only: nothing is dereferenced before the device is entered)
    nan, inf = float("nan"), float("inf")
    d = dict(ctx=ctypes.addressof(fake), f0=at(0), f1=at(1), w=w, h=h, pitch=pitch, u0=at(2), v0=at(3), sg=None, sc=None, nw=11, nh=4,
             npitch=npitch, r=7, s=8, R=7, K=20, eps=1e-3, shift=2.0, grad=0.5, curv=0.05, u=at(4), v=at(5),
             g=[at(6), at(7), at(8), at(9)], c=[at(10), at(11), at(12), at(13), at(14), at(15)], score=at(16), state=at(17), record=at(18))
    sg, sc = [at(20 + k) for k in range(4)], [at(24 + k) for k in range(6)]

    def group(planes):
        return None if planes is None else (ctypes.c_void_p * len(planes))(*planes)

    def call(**kw):
        a = dict(d, **kw)
        return lib.flow2d_subset_refine2_2d(a["ctx"], a["f0"], a["f1"], a["w"], a["h"], a["pitch"], a["u0"], a["v0"], group(a["sg"]), group(a["sc"]),
                                            a["nw"], a["nh"], a["npitch"], a["r"], a["s"], a["R"], a["K"], a["eps"], a["shift"], a["grad"],
                                            a["curv"], a["u"], a["v"], group(a["g"]), group(a["c"]), a["score"], a["state"], a["record"])

    def without(planes, k, value=None):
        return planes[:k] + [value] + planes[k + 1:]

    bad = [dict(ctx=None), dict(f0=None), dict(u0=None), dict(u=None), dict(v=None), dict(w=0), dict(nh=0), dict(pitch=pitch + 8), dict(npitch=32),
           dict(r=0), dict(s=65), dict(R=1), dict(R=0), dict(R=16), dict(K=0), dict(K=65), dict(eps=nan), dict(shift=0.0), dict(grad=inf),
           dict(curv=0.0), dict(curv=-0.05), dict(curv=nan), dict(curv=inf), dict(nw=12), dict(h=14), dict(record=at(18) + 4),
           # the planes of a group in part
           dict(g=without(d["g"], 0)), dict(g=without(d["g"], 3)), dict(c=without(d["c"], 0)), dict(c=without(d["c"], 5)),
           dict(c=without(d["c"], 2), g=None), dict(sg=without(sg, 1)), dict(sg=sg, sc=without(sc, 4)),
           # start curvatures without start gradients
           dict(sc=sc), dict(sc=sc, sg=[None] * 4),
           # planes that break the rules, and aliases: an output with a frame, a start plane or another output
           dict(c=without(d["c"], 1, at(11) + 4)), dict(sg=without(sg, 2, at(22) + 8)), dict(u=at(0)), dict(c=without(d["c"], 3, at(1) + span - pitch)),
           dict(sg=sg, u=sg[0]), dict(sg=sg, sc=sc, c=without(d["c"], 4, sc[1] + npitch)), dict(sg=sg, sc=sc, g=without(d["g"], 0, sc[5])),
           dict(sg=sg, score=sg[3]), dict(c=without(d["c"], 0, at(4))), dict(c=without(d["c"], 0, at(6))), dict(state=at(15) + npitch),
           dict(record=at(12) + 8), dict(sg=sg, sc=sc, record=sc[0])]
    for kw in bad:
        assert call(**kw) == 1, kw
    # (only refusals here: an accepted call would go on to launch on these made-up addresses where there is a device)
