"""flow2d_subset_refine_2d restated in numpy from the text of include/flow2d_c_abi.h -- node by node, in float64, every operation
of the header spelled out, with the one thing the header leaves open, the order of a sum over the subset, pluggable: sequential,
reversed, and the device's (a lane's partial over its pixels lane, lane + 64, ... from 0, then the xor butterfly 32, 16, ... 1).
What can be checked without a device: the accuracy on the speckle scenes against the parabola of flow2d_correlate_2d, that the
three orders agree on every state (their spread goes to profiles/subset/order_spread.json), the degenerate inputs, the edges of
the two stopping modes and the entry's host-side refusals."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from test_correlate_cpu import F32, U32, NAN_BITS, bits, correlate_reference, frame_range, grid, interior_epe, random_frames, scenes_module

F64 = np.float64
SUBSET_DTYPE = np.dtype([("nodes", "<u8"), ("converged", "<u8"), ("unconverged", "<u8"), ("strayed", "<u8"), ("flat", "<u8"),
                         ("no_input", "<u8"), ("iterations", "<u8"), ("reserved", "<u8")])
assert SUBSET_DTYPE.itemsize == 64
NO_INPUT, FLAT, STRAYED = -1, -2, -3
MAX_RADIUS, MAX_ITERATIONS = 15, 64
ORDERS = ("sequential", "reversed", "butterfly")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPREAD_PATH = os.path.join(ROOT, "profiles", "subset", "order_spread.json")


# ---- the sum over the subset, three ways ----------------------------------------------------------------------------------------------
def sum_sequential(x):
    return np.cumsum(x, axis=0)[-1]  # (accumulate adds strictly in order)


def sum_reversed(x):
    return np.cumsum(x[::-1], axis=0)[-1]


def sum_butterfly(x):
    """The device's order: lane l adds its terms l, l + 64, ... to 0 in ascending order (a lane without a term keeps 0), then
    x += x[lane ^ o] for o = 32, 16, 8, 4, 2, 1.  Every lane ends with the same bits; lane 0's are returned."""
    n, rows = x.shape[0], -(-x.shape[0] // 64)
    terms = np.zeros((rows * 64,) + x.shape[1:], F64)
    terms[:n] = x
    lanes = np.cumsum(np.concatenate([np.zeros((1, 64) + x.shape[1:], F64), terms.reshape((rows, 64) + x.shape[1:])]), axis=0)[-1]
    other = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[other ^ o]
    return lanes[0]


SUMS = {"sequential": sum_sequential, "reversed": sum_reversed, "butterfly": sum_butterfly}


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def cubic_weights(t):
    return (((-0.5 * t + 1.0) * t - 0.5) * t, ((1.5 * t - 2.5) * t) * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t, ((0.5 * t - 0.5) * t) * t)


def cubic_sample(frame, x, y):
    """g of the header at positions inside the frame (float64 arrays)."""
    h, w = frame.shape
    fx, fy = np.floor(x), np.floor(y)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    wx, wy = cubic_weights(x - fx), cubic_weights(y - fy)
    cols = [np.clip(ix - 1 + i, 0, w - 1) for i in range(4)]
    rows = []
    for j in range(4):
        row = np.clip(iy - 1 + j, 0, h - 1)
        a = [frame[row, c] for c in cols]
        rows.append(((wx[0] * a[0] + wx[1] * a[1]) + wx[2] * a[2]) + wx[3] * a[3])
    return ((wy[0] * rows[0] + wy[1] * rows[1]) + wy[2] * rows[2]) + wy[3] * rows[3]


def cholesky(H):
    """L of the header, or None where a pivot fails its test."""
    L = np.zeros((6, 6), F64)
    for k in range(6):
        acc = F64(0)
        for m in range(k):
            acc = acc + L[k, m] * L[k, m]
        d = H[k, k] - acc
        if not d > F64(1e-10) * H[k, k]:
            return None
        L[k, k] = np.sqrt(d)
        for i in range(k + 1, 6):
            acc = F64(0)
            for m in range(k):
                acc = acc + L[i, m] * L[k, m]
            L[i, k] = (H[i, k] - acc) / L[k, k]
    return L


def solve(L, b):
    y, x = np.zeros(6, F64), np.zeros(6, F64)
    for i in range(6):
        acc = F64(0)
        for m in range(i):
            acc = acc + L[i, m] * y[m]
        y[i] = (b[i] - acc) / L[i, i]
    for i in range(5, -1, -1):
        acc = F64(0)
        for m in range(i + 1, 6):
            acc = acc + L[m, i] * x[m]
        x[i] = (y[i] - acc) / L[i, i]
    return x


def refine_node(f0, f1, cx, cy, u0, v0, R, K, epsilon, max_shift, max_gradient, total):
    """(state, p, c, iterations begun) of one node with finite (u0, v0); f0, f1 float64."""
    h, w = f0.shape
    side = 2 * R + 1
    n = F64(side * side)
    k = np.arange(side * side)
    kx, ky = k % side - R, k // side - R
    xi, eta = kx.astype(F64), ky.astype(F64)
    p = np.array([u0, 0, 0, v0, 0, 0], F64)
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
    J = np.stack([fx, fx * xi, fx * eta, fy, fy * xi, fy * eta], axis=1)
    L = cholesky(total(J[:, :, None] * J[:, None, :]))
    if L is None:
        return FLAT, p, F64(0), 0
    c = F64(0)
    radius = F64(R)
    for it in range(1, K + 1):
        u, ux, uy, v, vx, vy = p
        X = xs.astype(F64) + ((u + ux * xi) + uy * eta)
        Y = ys.astype(F64) + ((v + vx * xi) + vy * eta)
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
        x = solve(L, total(J * res[:, None]))
        du, dux, duy, dv, dvx, dvy = -x
        ma, mb, mc, md = 1.0 + dux, duy, dvx, 1.0 + dvy
        det = ma * md - mb * mc
        if not abs(det) > 1e-12:
            return STRAYED, p, c, it
        ia, ib, ic, id_ = md / det, (-mb) / det, (-mc) / det, ma / det
        tx, ty = -(ia * du + ib * dv), -(ic * du + id_ * dv)
        p11, p12, p21, p22 = 1.0 + ux, uy, vx, 1.0 + vy
        p = np.array([(p11 * tx + p12 * ty) + u, (p11 * ia + p12 * ic) - 1.0, p11 * ib + p12 * id_,
                      (p21 * tx + p22 * ty) + v, p21 * ia + p22 * ic, (p21 * ib + p22 * id_) - 1.0], F64)
        if not (abs(p[0] - u0) <= max_shift and abs(p[3] - v0) <= max_shift and abs(p[1]) <= max_gradient and
                abs(p[2]) <= max_gradient and abs(p[4]) <= max_gradient and abs(p[5]) <= max_gradient):
            return STRAYED, p, c, it
        step = np.sqrt(((((du * du + (radius * dux) * (radius * dux)) + (radius * duy) * (radius * duy)) + dv * dv) +
                        (radius * dvx) * (radius * dvx)) + (radius * dvy) * (radius * dvy))
        if step < epsilon:
            return it, p, c, it
    return 0, p, c, K


class Refined:
    """The outputs of flow2d_subset_refine_2d: planes u, v, ux, uy, vx, vy, score, state (float32), the record, and p64 -- p in
    float64 where the state is >= 0, NaN elsewhere -- for the spread between orders."""
    NAMES = ("u", "v", "ux", "uy", "vx", "vy", "score", "state")

    def planes(self):
        return [getattr(self, name) for name in self.NAMES]


def subset_refine_reference(frame_0, frame_1, node_u0, node_v0, r, s, R, K=20, epsilon=1e-3, max_shift=2.0, max_gradient=0.5,
                            order="butterfly"):
    f0, f1 = np.asarray(frame_0, F32).astype(F64), np.asarray(frame_1, F32).astype(F64)
    node_u0, node_v0 = np.asarray(node_u0, F32), np.asarray(node_v0, F32)
    nh, nw = node_u0.shape
    epsilon, max_shift, max_gradient = (F64(F32(x)) for x in (epsilon, max_shift, max_gradient))
    out = Refined()
    planes = np.zeros((8, nh, nw), F32)
    out.p64 = np.full((nh, nw, 6), np.nan)
    record = np.zeros(1, SUBSET_DTYPE)
    record["nodes"] = nh * nw
    with np.errstate(all="ignore"):
        for j in range(nh):
            for i in range(nw):
                u0, v0 = node_u0[j, i], node_v0[j, i]
                if not (np.isfinite(u0) and np.isfinite(v0)):
                    planes[:6, j, i] = np.nan
                    planes[7, j, i] = NO_INPUT
                    record["no_input"] += 1
                    continue
                state, p, c, begun = refine_node(f0, f1, r + i * s, r + j * s, F64(u0), F64(v0), R, K, epsilon, max_shift, max_gradient,
                                                 SUMS[order])
                record["iterations"] += begun
                planes[7, j, i] = state
                if state >= 0:
                    planes[:6, j, i] = p[[0, 3, 1, 2, 4, 5]].astype(F32)
                    planes[6, j, i] = F32(c)
                    out.p64[j, i] = p
                    record["converged" if state >= 1 else "unconverged"] += 1
                else:
                    planes[0, j, i], planes[1, j, i] = u0, v0
                    record["flat" if state == FLAT else "strayed"] += 1
    nan = bits(planes[:6])
    nan[np.isnan(planes[:6])] = NAN_BITS
    planes[:6] = nan.view(F32)
    for name, plane in zip(Refined.NAMES, planes):
        setattr(out, name, plane)
    out.record = record
    return out


def all_orders(frame_0, frame_1, node_u0, node_v0, r, s, R, **kw):
    """(the butterfly order's result, the largest spread of p between the three orders); the orders must agree on every state."""
    runs = [subset_refine_reference(frame_0, frame_1, node_u0, node_v0, r, s, R, order=o, **kw) for o in ORDERS]
    for other in runs[:2]:
        assert np.array_equal(other.state, runs[2].state) and other.record.tobytes() == runs[2].record.tobytes()
    stack = np.stack([q.p64 for q in runs])
    live = np.isfinite(stack[2])
    spread = float((stack.max(0) - stack.min(0))[live].max()) if live.any() else 0.0
    return runs[2], spread


# ---- the six scenes ---------------------------------------------------------------------------------------------------------------
SCENE_CASES = [("translation", 6), ("affine", 6), ("large_translation", 12), ("rotation", 8), ("stretch", 8), ("shear", 8)]


def make_case_scene(name, width=96, height=80):
    sc = scenes_module()
    return sc.make_speckle_scene(name, width, height, seed=0) if name in sc.SPECKLE_MOTIONS else sc.make_speckle_deformation(name, width, height, seed=0)


def interior_mask(nw, nh, width, height, r, d, s):
    cx, cy = r + np.arange(nw) * s, r + np.arange(nh) * s
    return ((cy >= r + d) & (cy <= height - 1 - r - d))[:, None] & ((cx >= r + d) & (cx <= width - 1 - r - d))[None, :]


@functools.lru_cache(maxsize=None)
def scene_rows(name, d):
    """The accuracy figures of one scene, restated: what tools/subset_table.py prints (its device rows come from the same
    function with the device's refinement in place of the restatement's)."""
    return scene_figures(name, d, None)


def scene_figures(name, d, refine):
    r = R = 7
    s = 8
    sc = make_case_scene(name)
    lo, scale = frame_range(sc.frame_0, sc.frame_1)
    u0, v0, _, _, _ = correlate_reference(sc.frame_0, sc.frame_1, lo, scale, r, d, s)
    if refine is None:
        got, spread = all_orders(sc.frame_0, sc.frame_1, u0, v0, r, s, R)
    else:
        got, spread = refine(sc.frame_0, sc.frame_1, u0, v0, r, s, R), None
    nh, nw = u0.shape
    inside = interior_mask(nw, nh, 96, 80, r, d, s)
    cy, cx = r + np.arange(nh) * s, r + np.arange(nw) * s
    truth = [np.gradient(sc.gt_u.astype(F64), axis=1), np.gradient(sc.gt_u.astype(F64), axis=0),
             np.gradient(sc.gt_v.astype(F64), axis=1), np.gradient(sc.gt_v.astype(F64), axis=0)]
    grad = np.stack([np.abs(g.astype(F64) - t[np.ix_(cy, cx)]) for g, t in zip((got.ux, got.uy, got.vx, got.vy), truth)])[:, inside]
    states = got.state[inside]
    return dict(scene=name, range=d, nodes=int(nh * nw), interior=int(inside.sum()),
                parabola_mean_epe=float(interior_epe(u0, v0, sc, r, d, s).mean()),
                subset_mean_epe=float(interior_epe(got.u, got.v, sc, r, d, s).mean()),
                subset_max_epe=float(interior_epe(got.u, got.v, sc, r, d, s).max()),
                gradient_mean_error=float(np.sqrt((grad * grad).sum(0)).mean()), gradient_max_error=float(grad.max()),
                interior_converged=int((states >= 1).sum()), iterations_mean=float(states[states >= 1].mean()) if (states >= 1).any() else 0.0,
                iterations_max=int(states.max()), record={k: int(got.record[k][0]) for k in SUBSET_DTYPE.names[:7]}, spread=spread)


@pytest.mark.parametrize("name,d", SCENE_CASES)
def test_accuracy_on_the_six_scenes(name, d):
    """96 x 80, r = R = 7, s = 8, started from flow2d_correlate_2d's vectors: every interior node converges, the mean interior
    endpoint error is at most a third of the parabola's, the mean error of the gradients against np.gradient of the ground
    truth -- per node the root of the four squared errors, the stricter reading -- is at most 0.004, and the three summation orders give the same state at every node (all_orders asserts it)."""
    row = scene_rows(name, d)
    print(json.dumps(row))
    assert row["interior"] >= 12 and row["interior_converged"] == row["interior"]
    assert row["subset_mean_epe"] <= row["parabola_mean_epe"] / 3.0
    assert row["gradient_mean_error"] <= 0.004
    assert row["spread"] < 1e-9  # (orders of magnitude below an fp32 ulp of a displacement: the planes can differ only at a rounding boundary)


def test_order_spread_is_recorded():
    """The largest spread of p under the three orders, per scene, printed and written to profiles/subset/order_spread.json."""
    spread = {name: float("%.3e" % scene_rows(name, d)["spread"]) for name, d in SCENE_CASES}
    print(json.dumps(spread))
    text = json.dumps({"what": "largest |p(order a) - p(order b)| over the nodes with state >= 0, float64; orders: " + ", ".join(ORDERS),
                       "grid": "96 x 80, r = R = 7, s = 8", "spread": spread}, indent=1, sort_keys=True) + "\n"
    if not os.path.exists(SPREAD_PATH) or open(SPREAD_PATH).read() != text:
        try:  # (the committed file holds these figures already; a tree that cannot be written keeps it)
            os.makedirs(os.path.dirname(SPREAD_PATH), exist_ok=True)
            with open(SPREAD_PATH, "w") as out:
                out.write(text)
        except OSError as e:
            print("not written: %s" % e)
    assert max(spread.values()) < 1e-9


# ---- degenerate inputs, mode edges ------------------------------------------------------------------------------------------------
def small_case(seed=17, w=50, h=41, r=3, s=5):
    f0, f1 = random_frames(w, h, seed=seed, shift=(1, 0), noise=2.0)
    nw, nh = grid(w, h, r, s)
    return f0, f1, np.full((nh, nw), 1, F32), np.zeros((nh, nw), F32), r, s


def test_degenerate_inputs():
    f0, f1, u0, v0, r, s = small_case()
    base = subset_refine_reference(f0, f1, u0, v0, r, s, 3)
    assert (base.state[1:-1, 1:-1] >= 1).all() and base.record["nodes"][0] == u0.size
    # a constant frame 0: flat everywhere, u0 and v0 copied, gradients and score 0
    got = subset_refine_reference(np.full_like(f0, 7.0), f1, u0, v0, r, s, 3)
    assert (got.state == FLAT).all() and np.array_equal(bits(got.u), bits(u0)) and (got.ux == 0).all() and (got.score == 0).all()
    assert got.record.tolist() == [(u0.size, 0, 0, 0, u0.size, 0, 0, 0)]
    # a NaN in frame 0 makes the nodes whose window or gradient stencil holds it flat; one in frame 1 those that sample it
    for which in (0, 1):
        g0, g1 = f0.copy(), f1.copy()
        (g0, g1)[which][18, 23] = np.nan
        got = subset_refine_reference(g0, g1, u0, v0, r, s, 3)
        hit = got.state == FLAT
        assert 1 <= hit.sum() <= 6 and hit[3, 4] and np.isfinite(got.u).all()
        assert np.array_equal(bits(got.u)[~hit], bits(base.u)[~hit]) and (got.state[~hit] == base.state[~hit]).all()
    # nodes without input, and one far away
    a0, b0 = u0.copy(), v0.copy()
    a0[2, 2], b0[3, 3], a0[4, 4] = np.nan, np.inf, 1e30
    got = subset_refine_reference(f0, f1, a0, b0, r, s, 3)
    assert got.state[2, 2] == NO_INPUT and got.state[3, 3] == NO_INPUT and got.state[4, 4] == STRAYED
    assert bits(got.u)[2, 2] == NAN_BITS and bits(got.vy)[3, 3] == NAN_BITS and got.score[2, 2] == 0
    assert bits(got.u)[4, 4] == bits(F32(1e30)) and got.ux[4, 4] == 0 and got.record["no_input"][0] == 2
    # R > r: the border nodes' subsets leave frame 0
    got = subset_refine_reference(f0, f1, u0, v0, r, s, 6)
    cy, cx = r + np.arange(u0.shape[0]) * s, r + np.arange(u0.shape[1]) * s
    leaves = ~(((cy - 6 >= 0) & (cy + 6 <= 40))[:, None] & ((cx - 6 >= 0) & (cx + 6 <= 49))[None, :])
    assert leaves.sum() == 15 and (got.state[leaves] == STRAYED).all() and (got.state[2:-2, 2:-2] >= 1).all()
    assert got.record["nodes"][0] == sum(int(got.record[k][0]) for k in ("converged", "unconverged", "strayed", "flat", "no_input"))


def test_mode_edges():
    f0, f1, u0, v0, r, s = small_case()
    # epsilon = 0: exactly K iterations, state 0
    got = subset_refine_reference(f0, f1, u0, v0, r, s, 3, K=5, epsilon=0.0)
    inner = got.state[1:-1, 1:-1]
    assert (inner == 0).all() and got.record["converged"][0] == 0
    assert got.record["iterations"][0] >= 5 * inner.size and got.record["unconverged"][0] >= inner.size
    # f1 = f0 with u0 = 0: the residual is exactly 0, so the first step is and the node converges at n = 1 with u = v = 0
    zero = np.zeros_like(u0)
    for order in ORDERS:
        got = subset_refine_reference(f0, f0, zero, zero, r, s, 3, order=order)
        assert (got.state == 1).all() and (got.u == 0).all() and (got.v == 0).all() and (got.ux == 0).all() and (got.vy == 0).all()
        assert (got.score == 1).all() and got.record["iterations"][0] == u0.size
    # K = 1 delivers the first step
    one = subset_refine_reference(f0, f1, u0, v0, r, s, 3, K=1)
    assert set(np.unique(one.state[1:-1, 1:-1])) <= {0.0, 1.0}


def test_the_three_orders_agree_on_the_gpu_tests_input():
    f0, f1, u0, v0, r, s = small_case()
    got, spread = all_orders(f0, f1, u0, v0, r, s, 3)
    print("spread %.3e" % spread)
    assert spread < 1e-9


# ---- the entry's host side ----------------------------------------------------------------------------------------------------------
def test_deformation_scenes():
    sc = scenes_module()
    assert sc.SPECKLE_DEFORMATIONS == ("rotation", "stretch", "shear") and sc.SPECKLE_MOTIONS == ("translation", "affine", "large_translation")
    for name, matrix in (("rotation", None), ("stretch", [[1.06, 0], [0, 0.97]]), ("shear", [[1, 0.08], [0, 1]])):
        scene = sc.make_speckle_deformation(name, 48, 40, seed=2)
        cx, cy = 23.5, 19.5
        ux, vy = np.gradient(scene.gt_u.astype(F64), axis=1), np.gradient(scene.gt_v.astype(F64), axis=0)
        if matrix is not None:
            assert abs(ux.mean() - (matrix[0][0] - 1)) < 1e-5 and abs(vy.mean() - (matrix[1][1] - 1)) < 1e-5
        else:
            assert abs(ux.mean() - (np.cos(np.radians(5.0)) - 1)) < 1e-5
        # the centre moves by the translation alone
        assert abs(scene.gt_u[19:21, 23:25].mean() - 1.6) < 1e-5 and abs(scene.gt_v[19:21, 23:25].mean() + 0.7) < 1e-5
        ys, xs = np.mgrid[5:35, 5:43].astype(F64)
        there = scene.frame_1_at(xs + scene.gt_u[5:35, 5:43].astype(F64), ys + scene.gt_v[5:35, 5:43].astype(F64))
        assert np.abs(there - scene.frame_0[5:35, 5:43]).max() < 1e-3
    with pytest.raises(ValueError):
        sc.make_speckle_deformation("translation")


def test_refusals_without_a_device(flow2d):
    lib = flow2d.hip_lib()
    fake = ctypes.create_string_buffer(4096)
    w, h, pitch, npitch = 100, 40, 512, 64
    span = pitch * h
    at = lambda k: (1 << 20) + k * (span + 4096)  # noqa: E731  (addresses only: nothing is dereferenced before the device is entered)
    nan, inf = float("nan"), float("inf")
    d = dict(ctx=ctypes.addressof(fake), f0=at(0), f1=at(1), w=w, h=h, pitch=pitch, u0=at(2), v0=at(3), nw=11, nh=4, npitch=npitch, r=7,
             s=8, R=7, K=20, eps=1e-3, shift=2.0, grad=0.5, u=at(4), v=at(5), ux=at(6), uy=at(7), vx=at(8), vy=at(9), score=at(10),
             state=at(11), record=at(12))

    def call(**kw):
        a = dict(d, **kw)
        return lib.flow2d_subset_refine_2d(a["ctx"], a["f0"], a["f1"], a["w"], a["h"], a["pitch"], a["u0"], a["v0"], a["nw"], a["nh"],
                                           a["npitch"], a["r"], a["s"], a["R"], a["K"], a["eps"], a["shift"], a["grad"], a["u"], a["v"],
                                           a["ux"], a["uy"], a["vx"], a["vy"], a["score"], a["state"], a["record"])

    bad = [dict(ctx=None), dict(f0=None), dict(f1=None), dict(u0=None), dict(v0=None), dict(u=None), dict(v=None), dict(w=0), dict(h=0),
           dict(nw=0), dict(nh=0), dict(pitch=pitch + 8), dict(pitch=396), dict(npitch=32), dict(npitch=npitch + 4), dict(r=0), dict(r=16),
           dict(s=0), dict(s=65), dict(R=0), dict(R=16), dict(R=-1), dict(K=0), dict(K=65), dict(eps=-1e-3), dict(eps=nan), dict(eps=inf),
           dict(shift=0.0), dict(shift=-1.0), dict(shift=nan), dict(shift=inf), dict(grad=0.0), dict(grad=nan), dict(grad=inf),
           dict(nw=12), dict(nh=5), dict(w=14), dict(h=14), dict(ux=None), dict(uy=None), dict(vx=None), dict(vy=None),
           dict(ux=None, uy=None, vx=None), dict(f0=at(0) + 4), dict(u0=at(2) + 4), dict(score=at(10) + 8), dict(record=at(12) + 4),
           dict(u=at(0)), dict(v=at(1) + span - pitch), dict(ux=at(2)), dict(vy=at(3) + npitch), dict(score=at(4)), dict(state=at(9) + npitch),
           dict(record=at(0) + 64), dict(record=at(6) + 8), dict(uy=at(6))]
    for kw in bad:
        assert call(**kw) == 1, kw
    # (only refusals here: an accepted call would go on to launch on these made-up addresses where there is a device)


def subset_entries(lib):
    """Every subset refinement entry as a function of one dictionary of arguments (g, c: the out gradients and curvatures; sg, sc:
    the start's, lists or None), each entry taking those it has."""
    def group(planes, n):
        return (ctypes.c_void_p * n)(*planes) if planes is not None else None

    def order_1(entry, start, mask):
        def call(a):
            sg = a["sg"] if a["sg"] is not None else [None] * 4
            return entry(a["ctx"], a["f0"], a["f1"], a["w"], a["h"], a["pitch"], a["u0"], a["v0"], *(sg if start else []), a["nw"], a["nh"],
                         a["npitch"], a["r"], a["s"], a["R"], a["K"], a["eps"], a["shift"], a["grad"],
                         *([a["mask"] if mask == "mask" else None, a["min_pixels"]] if mask else []), a["u"], a["v"], *a["g"], a["score"],
                         a["state"], a["record"])
        return call

    def order_2(entry):
        def call(a):
            return entry(a["ctx"], a["f0"], a["f1"], a["w"], a["h"], a["pitch"], a["u0"], a["v0"], group(a["sg"], 4), group(a["sc"], 6),
                         a["nw"], a["nh"], a["npitch"], a["r"], a["s"], a["R"], a["K"], a["eps"], a["shift"], a["grad"], a["curv"], a["u"],
                         a["v"], group(a["g"], 4), group(a["c"], 6), a["score"], a["state"], a["record"])
        return call

    return {"plain": order_1(lib.flow2d_subset_refine_2d, False, None), "from": order_1(lib.flow2d_subset_refine_from_2d, True, None),
            "masked": order_1(lib.flow2d_subset_refine_masked_2d, True, "mask"),
            "masked, no mask": order_1(lib.flow2d_subset_refine_masked_2d, True, "none"),
            "spline": order_1(lib.flow2d_subset_refine_spline_2d, True, "mask"),
            "spline, no mask": order_1(lib.flow2d_subset_refine_spline_2d, True, "none"),
            "order 2": order_2(lib.flow2d_subset_refine2_2d), "order 2, spline": order_2(lib.flow2d_subset_refine2_spline_2d)}


NODES_2_31 = dict(w=(1 << 16) + 4, h=(1 << 15) + 4, pitch=4 * ((1 << 16) + 4), nw=1 << 16, nh=1 << 15, npitch=4 << 16, r=2, s=1, R=2, min_pixels=6)


@pytest.mark.parametrize("change,status", [
    (dict(R=0), 1), (dict(K=0), 1), (dict(eps=float("nan")), 1), (dict(record="misaligned"), 1), (dict(nw=12), 1), (dict(g="partial"), 1),
    (dict(u="frame 1"), 1), (NODES_2_31, 5), (dict(NODES_2_31, f0="misaligned"), 1), (dict(NODES_2_31, v=None), 1)],
    ids=["radius 0", "no iteration", "NaN epsilon", "misaligned record", "nw beyond the grid", "gradient planes in part",
         "an out plane in frame 1", "2^31 nodes", "2^31 nodes, a misaligned frame", "2^31 nodes, no out_v"])
def test_every_entry_refuses_alike(flow2d, change, status):
    """One invalid argument to every subset refinement entry: the same status from each.  FLOW2D_ERR_UNSUPPORTED (5), the node count,
    comes behind every plane check.  Nothing is launched: an accepted call would go on to made-up addresses."""
    fake = ctypes.create_string_buffer(4096)
    w, h, pitch, npitch = 100, 40, 512, 64
    at = lambda k: (1 << 20) + k * (pitch * h + 4096)  # noqa: E731  (addresses only: nothing is dereferenced before the device is entered)
    a = dict(ctx=ctypes.addressof(fake), f0=at(0), f1=at(1), w=w, h=h, pitch=pitch, u0=at(2), v0=at(3), sg=[at(20 + k) for k in range(4)],
             sc=[at(24 + k) for k in range(6)], nw=11, nh=4, npitch=npitch, r=7, s=8, R=7, K=20, eps=1e-3, shift=2.0, grad=0.5, curv=0.05,
             mask=at(19), min_pixels=57, u=at(4), v=at(5), g=[at(6 + k) for k in range(4)], c=[at(10 + k) for k in range(6)], score=at(16),
             state=at(17), record=at(18))
    named = {"misaligned": lambda key: a[key] + 4, "partial": lambda key: [None] + a[key][1:], "frame 1": lambda key: at(1) + pitch}
    a.update({key: named[value](key) if isinstance(value, str) else value for key, value in change.items()})
    got = {name: call(a) for name, call in subset_entries(flow2d.hip_lib()).items()}
    print(got)
    assert got == dict.fromkeys(got, status)


def test_python_record_matches_the_restatement_layout(flow2d):
    rec = flow2d.SubsetRecord()
    rec.nodes, rec.converged, rec.unconverged, rec.strayed, rec.flat, rec.no_input, rec.iterations = 9, 1, 2, 3, 4, 5, 6
    a = np.frombuffer(bytes(rec), SUBSET_DTYPE)[0]
    assert a.tolist() == (9, 1, 2, 3, 4, 5, 6, 0)
    assert ctypes.sizeof(flow2d.SubsetRecord) == flow2d.SUBSET_RECORD_BYTES == SUBSET_DTYPE.itemsize
    assert (flow2d.SUBSET_MAX_RADIUS, flow2d.SUBSET_MAX_ITERATIONS) == (MAX_RADIUS, MAX_ITERATIONS)
    assert (flow2d.SUBSET_NO_INPUT, flow2d.SUBSET_FLAT, flow2d.SUBSET_STRAYED) == (NO_INPUT, FLAT, STRAYED)
    assert list(rec.summary()) == list(SUBSET_DTYPE.names[:7])
