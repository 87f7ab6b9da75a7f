"""flow2d_node_strain_2d restated in numpy from the text of include/flow2d_c_abi.h (np.float64 operations in the stated order,
vectorised over the nodes with a Python loop over the window's offsets in raster order, so that every node's sums have the
stated order), with its record, and what can be checked without a device: exact recovery of affine and quadratic fields,
the noise a window fit lets through, the sparse and degenerate cases, the direct form and the record."""
import numpy as np
import pytest

from test_deformation_cpu import F32, GREEN, NAN, PLANES, SMALL, STAT_NAMES, STATS_DTYPE, U32, bits

F64 = np.float64
CENTRE, SPARSE, DEGENERATE = 0, 1, 2  # reserved[0 .. 2] of the record; -1 in "reason" is a valid node
MAX_WINDOW = 7  # FLOW2D_NODE_STRAIN_MAX_WINDOW


def basis(order, di, dj):
    """phi over a window offset, the products formed in int."""
    return (1, di, dj) if order == 1 else (1, di, dj, di * di, di * dj, dj * dj)


def usable_nodes(u, v, state, grads, min_state):
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(u) & np.isfinite(v)
        if state is not None:
            ok &= np.asarray(state, F32) >= F32(min_state)
        for g in grads or ():
            ok &= np.isfinite(g)
    return ok


def strain_quantities(a, b, c, d, measure):
    """The nine quantities in double from double gradients, each cast to float once."""
    with np.errstate(all="ignore"):
        if measure == SMALL:
            exx, eyy, exy = a, d, 0.5 * (b + c)
        else:
            assert measure == GREEN
            exx = a + 0.5 * (a * a + c * c)
            eyy = d + 0.5 * (b * b + d * d)
            exy = 0.5 * ((b + c) + (a * b + c * d))
        mean, half = 0.5 * (exx + eyy), 0.5 * (exx - eyy)
        shear = np.sqrt(half * half + exy * exy)
        q = dict(divergence=a + d, vorticity=c - b, dilatation=(a + d) + (a * d - b * c), exx=exx, eyy=eyy, exy=exy, e1=mean + shear,
                 e2=mean - shear, max_shear=shear)
        return {name: np.asarray(x, F64).astype(F32) for name, x in q.items()}


def window_fit(u, v, usable, s, m, order, min_nodes):
    """(a, b, c, d, reason) of the window fit for every node."""
    nh, nw = u.shape
    k = 3 if order == 1 else 6
    pad = lambda x, fill: np.pad(x, m, constant_values=fill)  # noqa: E731
    pu, pv, pok = pad(u.astype(F64), 0.0), pad(v.astype(F64), 0.0), pad(usable, False)
    uc, vc = u.astype(F64), v.astype(F64)
    M = np.zeros((k, k, nh, nw), np.int64)
    bu, bv = np.zeros((k, nh, nw), F64), np.zeros((k, nh, nw), F64)
    with np.errstate(all="ignore"):
        for dj in range(-m, m + 1):
            for di in range(-m, m + 1):
                sl = (slice(m + dj, m + dj + nh), slice(m + di, m + di + nw))
                ok = pok[sl]
                wu, wv = pu[sl] - uc, pv[sl] - vc
                phi = basis(order, di, dj)
                for a in range(k):
                    for b in range(k):
                        M[a, b] += ok * np.int64(phi[a] * phi[b])
                    # a skipped tap adds nothing: + 0.0 leaves a sum that started at +0 as it is, bit for bit
                    bu[a] += np.where(ok, F64(phi[a]) * wu, 0.0)
                    bv[a] += np.where(ok, F64(phi[a]) * wv, 0.0)
        n = M[0, 0]
        H = M.astype(F64)
        L = np.zeros_like(H)
        degenerate = np.zeros((nh, nw), bool)
        for kk in range(k):
            total = np.zeros((nh, nw), F64)
            for j in range(kk):
                total = total + L[kk, j] * L[kk, j]
            d = H[kk, kk] - total
            degenerate |= ~(d > 1e-10 * H[kk, kk])
            L[kk, kk] = np.sqrt(d)
            for i in range(kk + 1, k):
                inner = np.zeros((nh, nw), F64)
                for j in range(kk):
                    inner = inner + L[i, j] * L[kk, j]
                L[i, kk] = (H[i, kk] - inner) / L[kk, kk]

        def solve(b):
            y, x = np.zeros_like(b), np.zeros_like(b)
            for i in range(k):
                total = np.zeros((nh, nw), F64)
                for j in range(i):
                    total = total + L[i, j] * y[j]
                y[i] = (b[i] - total) / L[i, i]
            for i in range(k - 1, -1, -1):
                total = np.zeros((nh, nw), F64)
                for j in range(i + 1, k):
                    total = total + L[j, i] * x[j]
                x[i] = (y[i] - total) / L[i, i]
            return x

        cu, cv = solve(bu), solve(bv)
        sd = F64(s)
        grad = (cu[1] / sd, cu[2] / sd, cv[1] / sd, cv[2] / sd)
    reason = np.where(~usable, CENTRE, np.where(~(n >= min_nodes), SPARSE, np.where(degenerate, DEGENERATE, -1)))
    return grad + (reason,)


def node_strain_reference(u, v, state=None, grads=None, s=8, m=2, order=1, min_nodes=None, min_state=1, measure=SMALL):
    """{plane name: [nh, nw] float32} for the nine planes, "gradient" (a, b, c, d in double), "valid", "reason" (-1 valid, else
    CENTRE / SPARSE / DEGENERATE) and "stats" (one STATS_DTYPE record) with "abs_sum" / "abs_sum_sq".  min_nodes None: k + 1."""
    u, v = np.ascontiguousarray(u, F32), np.ascontiguousarray(v, F32)
    assert 1 <= s <= 64 and 0 <= m <= MAX_WINDOW and min_state in (0, 1)
    if m == 0:
        assert grads is not None and len(grads) == 4
        usable = usable_nodes(u, v, state, grads, min_state)
        a, b, c, d = (np.asarray(g, F32).astype(F64) for g in grads)
        reason = np.where(usable, -1, CENTRE)
    else:
        assert order in (1, 2)
        k = 3 if order == 1 else 6
        min_nodes = k + 1 if min_nodes is None else min_nodes
        assert k <= min_nodes <= (2 * m + 1) ** 2
        usable = usable_nodes(u, v, state, None, min_state)
        a, b, c, d, reason = window_fit(u, v, usable, s, m, order, min_nodes)
    valid = reason == -1
    q = strain_quantities(a, b, c, d, measure)
    out = {name: np.where(valid, q[name], NAN).astype(F32) for name in PLANES}
    stats = np.zeros(1, STATS_DTYPE)
    n = int(valid.sum())
    stats["valid"], stats["invalid"] = n, valid.size - n
    for r in (CENTRE, SPARSE, DEGENERATE):
        stats["reserved"][0][r] = int((reason == r).sum())
    out["abs_sum"], out["abs_sum_sq"] = {}, {}
    for name in STAT_NAMES:
        x = out[name][valid].astype(F64)  # raster order
        stats[name]["sum"], stats[name]["sum_sq"] = x.sum(), (x * x).sum()
        if n:
            stats[name]["min"], stats[name]["max"] = x.min(), x.max()
        out["abs_sum"][name], out["abs_sum_sq"][name] = float(np.abs(x).sum()), float((x * x).sum())
    out.update(gradient=(a, b, c, d), valid=valid, reason=reason, stats=stats)
    return out


def node_positions(nw, nh, s, r=0):
    """Pixel coordinates (x, y) of the nodes of an nw x nh grid."""
    j, i = np.mgrid[0:nh, 0:nw]
    return (r + i * s).astype(F64), (r + j * s).astype(F64)


def affine_field(nw, nh, s, g=(0.003, -0.002, 0.0015, 0.0025), r=7):
    x, y = node_positions(nw, nh, s, r)
    a, b, c, d = g
    return (0.25 + a * x + b * y).astype(F32), (-0.5 + c * x + d * y).astype(F32)


def node_case(nw, nh, seed, holes=0.2):
    """A smooth field with noise, a `holes` share of the nodes lost (state 0, -1, -2, -3 or NaN), some predicted (65) and some
    unconverged (0) nodes, a NaN and an infinity at nodes whose state says usable, and four gradient planes with a NaN."""
    rng = np.random.default_rng(seed + 1000 * nw + nh)
    u, v = affine_field(nw, nh, 8)
    u = (u + 0.01 * rng.standard_normal((nh, nw))).astype(F32)
    v = (v + 0.01 * rng.standard_normal((nh, nw))).astype(F32)
    state = rng.integers(1, 21, (nh, nw)).astype(F32)
    lost = rng.random((nh, nw)) < holes
    state[lost] = rng.choice(np.array([0, 0, -1, -2, -3, np.nan], F32), int(lost.sum()))
    state[rng.random((nh, nw)) < 0.05] = 65
    grads = [(0.01 * rng.standard_normal((nh, nw))).astype(F32) for _ in range(4)]
    flat = rng.permutation(nw * nh)
    if nw * nh >= 4:
        u.flat[flat[0]] = np.nan
        v.flat[flat[1]] = np.inf
        grads[2].flat[flat[2]] = np.nan
        for q in flat[:3]:
            state.flat[q] = 3
    return u, v, state, grads


def test_affine_field_with_holes_is_recovered():
    """50 x 40, s = 8, m = 2, 20 % of the nodes unusable: every valid node gives the field's gradients to 1e-7, the bound the
    fp32 rounding of the inputs sets (|u| < 2: half an ulp is 6e-8, and the fit divides by s = 8)."""
    nw, nh, s = 50, 40, 8
    g = (0.003, -0.002, 0.0015, 0.0025)
    u, v = affine_field(nw, nh, s, g)
    rng = np.random.default_rng(3)
    state = np.where(rng.random((nh, nw)) < 0.2, 0, 5).astype(F32)
    for order in (1, 2):
        ref = node_strain_reference(u, v, state, None, s, 2, order)
        valid = ref["valid"]
        assert valid.sum() > 0.7 * nw * nh and not valid[state == 0].any()
        worst = max(float(np.abs(got[valid] - want).max()) for got, want in zip(ref["gradient"], g))
        print("order %d: %d valid nodes, worst gradient error %.3g" % (order, valid.sum(), worst))
        assert worst <= 1e-7
        assert np.isnan(ref["exx"][~valid]).all() and np.array_equal(bits(ref["exx"][valid]), bits(ref["gradient"][0][valid].astype(F32)))


def test_quadratic_field():
    """u = 1e-4 x^2 on a full 12 x 9 grid, s = 8, m = 2: order 2 is right everywhere, order 1 at the interior columns (a
    symmetric window's slope does not see the quadratic term) and off by 1e-4 * s * m at the border column, where the window
    holds the columns 0 .. m only: the least-squares slope of t^2 over t = 0 .. m is m."""
    nw, nh, s, m, c2 = 12, 9, 8, 2, 1e-4
    x, _ = node_positions(nw, nh, s)
    u, v = (c2 * x * x).astype(F32), np.zeros((nh, nw), F32)
    true = 2 * c2 * x
    second = node_strain_reference(u, v, None, None, s, m, 2)
    assert second["valid"].all()
    e2 = np.abs(second["gradient"][0] - true).max()
    first = node_strain_reference(u, v, None, None, s, m, 1)
    assert first["valid"].all()
    e1 = np.abs(first["gradient"][0] - true)
    print("order 2: worst %.3g; order 1: interior worst %.3g, border column %.6g" % (e2, e1[:, m:nw - m].max(), e1[:, 0].max()))
    assert e2 <= 1e-7
    assert e1[:, m:nw - m].max() <= 1e-7
    assert np.abs(first["gradient"][0][:, 0] - (true[:, 0] + c2 * s * m)).max() <= 1e-7
    assert np.abs(first["gradient"][0][:, -1] - (true[:, -1] - c2 * s * m)).max() <= 1e-7
    for k in (1, 2, 3):
        assert np.abs(first["gradient"][k]).max() <= 1e-7 and np.abs(second["gradient"][k]).max() <= 1e-7


@pytest.mark.parametrize("m", [1, 2, 3])
def test_noise_through_a_window(m):
    """An affine field plus Gaussian noise sigma on a full 50 x 40 grid, s = 8: over a whole window the slope is
    sum(di * w) / (s * sum(di^2)), so its standard deviation is sigma / (s * sqrt((2m + 1) * m (m + 1)(2m + 1) / 3))."""
    nw, nh, s, sigma = 50, 40, 8, 0.01
    g = (0.003, -0.002, 0.0015, 0.0025)
    u, v = affine_field(nw, nh, s, g)
    rng = np.random.default_rng(0)
    u = (u + sigma * rng.standard_normal((nh, nw))).astype(F32)
    v = (v + sigma * rng.standard_normal((nh, nw))).astype(F32)
    ref = node_strain_reference(u, v, None, None, s, m, 1)
    assert ref["valid"].all()
    a = ref["gradient"][0][m:nh - m, m:nw - m]
    want = sigma / (s * np.sqrt((2 * m + 1) * m * (m + 1) * (2 * m + 1) / 3.0))
    got = float(a.std())
    print("m = %d: std of a %.4g, predicted %.4g (%.1f %%)" % (m, got, want, 100 * (got / want - 1)))
    assert abs(got / want - 1) <= 0.15
    assert abs(float(a.mean()) - g[0]) <= 3 * want / np.sqrt(a.size / (2 * m + 1) ** 2)


def reasons(ref):
    return [int(ref["stats"]["reserved"][0][r]) for r in (CENTRE, SPARSE, DEGENERATE)]


def test_sparse_and_degenerate_grids():
    one = node_strain_reference(np.ones((1, 1), F32), np.ones((1, 1), F32), None, None, 8, 1, 1, 3)
    assert not one["valid"].any() and reasons(one) == [0, 1, 0]
    x, _ = node_positions(5, 1, 8)
    u, v = (0.01 * x).astype(F32), np.zeros((1, 5), F32)
    # a row of nodes is collinear: whatever the window, the fit has no slope along y
    for m, order, min_nodes, want in ((2, 1, 3, [0, 0, 5]), (1, 1, 3, [0, 2, 3]), (2, 1, 4, [0, 2, 3]), (2, 2, 6, [0, 5, 0]),
                                      (7, 1, 3, [0, 0, 5])):
        ref = node_strain_reference(u, v, None, None, 8, m, order, min_nodes)
        assert not ref["valid"].any() and reasons(ref) == want, (m, order, min_nodes)
        assert int(ref["stats"]["invalid"][0]) == 5 and all(np.isnan(ref[name]).all() for name in PLANES)
    # a lost centre goes before everything else; its neighbours lose a node: 1, -, 2, 3, 2 usable nodes in the windows
    state = np.array([[1, 0, 1, 1, 1]], F32)
    assert reasons(node_strain_reference(u, v, state, None, 8, 1, 1, 3)) == [1, 3, 1]


def test_exactly_k_nodes():
    """Three usable nodes that are not collinear -- the centre, its right and its lower neighbour -- determine the plane: valid
    at min_nodes = 3 with the exact differences, sparse at 4."""
    u = np.array([[9, 9, 9], [9, 1.0, 1.5], [9, 0.75, 9]], F32)
    v = np.array([[9, 9, 9], [9, -2.0, -1.0], [9, -2.5, 9]], F32)
    state = np.array([[0, 0, 0], [0, 1, 1], [0, 1, 0]], F32)
    ref = node_strain_reference(u, v, state, None, 4, 1, 1, 3)
    assert ref["reason"][1, 1] == -1 and reasons(ref)[0] == 6
    got = [float(g[1, 1]) for g in ref["gradient"]]
    assert np.allclose(got, [0.125, -0.0625, 0.25, -0.125], rtol=0, atol=1e-15), got
    # the two other usable nodes see the same three nodes, which do not surround them: still three, still not collinear
    assert ref["valid"].sum() == 3
    ref = node_strain_reference(u, v, state, None, 4, 1, 1, 4)
    assert not ref["valid"].any() and reasons(ref) == [6, 3, 0]
    # collinear: the lower neighbour replaced by the left one; the outer two see two nodes only
    state = np.array([[0, 0, 0], [1, 1, 1], [0, 0, 0]], F32)
    assert reasons(node_strain_reference(u, v, state, None, 4, 1, 1, 3)) == [6, 2, 1]


@pytest.mark.parametrize("measure", [SMALL, GREEN])
def test_direct_form_is_the_strain_of_the_input_gradients(measure):
    nw, nh = 9, 7
    u, v, state, grads = node_case(nw, nh, seed=4)
    ref = node_strain_reference(u, v, state, grads, 8, 0, measure=measure)
    ok = np.isfinite(u) & np.isfinite(v) & (state >= 1) & np.all([np.isfinite(g) for g in grads], axis=0)
    assert np.array_equal(ref["valid"], ok) and 0 < ok.sum() < nw * nh
    a, b, c, d = (g.astype(F64) for g in grads)
    with np.errstate(all="ignore"):
        if measure == SMALL:
            exx, eyy, exy = a, d, (b + c) / 2
        else:
            exx, eyy, exy = a + (a * a + c * c) / 2, d + (b * b + d * d) / 2, ((b + c) + (a * b + c * d)) / 2
        shear = np.sqrt(((exx - eyy) / 2) ** 2 + exy ** 2)
        want = dict(divergence=a + d, vorticity=c - b, dilatation=(1 + a) * (1 + d) - b * c - 1, exx=exx, eyy=eyy, exy=exy,
                    e1=(exx + eyy) / 2 + shear, e2=(exx + eyy) / 2 - shear, max_shear=shear)
    for name in PLANES:
        assert np.isnan(ref[name][~ok]).all(), name
        assert np.abs(ref[name][ok] - want[name][ok]).max() <= 1e-8, name  # fp32 of values below 0.1: half an ulp is 4e-9
    # min_state 0 takes the unconverged nodes too
    more = node_strain_reference(u, v, state, grads, 8, 0, min_state=0, measure=measure)
    assert more["valid"].sum() == (ok | ((state == 0) & np.isfinite(u) & np.isfinite(v) &
                                         np.all([np.isfinite(g) for g in grads], axis=0))).sum() > ok.sum()


def test_record():
    nw, nh = 21, 13
    u, v, state, _ = node_case(nw, nh, seed=9, holes=0.55)
    ref = node_strain_reference(u, v, state, None, 8, 2, 2, measure=GREEN)
    rec = ref["stats"][0]
    valid = ref["valid"]
    assert rec["valid"] == valid.sum() and rec["invalid"] == nw * nh - valid.sum()
    assert sum(reasons(ref)) == rec["invalid"] and reasons(ref)[0] == (~usable_nodes(u, v, state, None, 1)).sum()
    assert all(c > 0 for c in reasons(ref)[:2]) and not rec["reserved"][3:].any()
    for name in STAT_NAMES:
        x = ref[name][valid]
        assert rec[name]["min"] == x.min() and rec[name]["max"] == x.max(), name
        assert rec[name]["sum"] == pytest.approx(float(x.astype(F64).sum()), rel=1e-12)
        assert rec[name]["sum_sq"] == pytest.approx(float((x.astype(F64) ** 2).sum()), rel=1e-12)
    assert (ref["e1"][valid] >= ref["e2"][valid]).all() and (ref["max_shear"][valid] >= 0).all()
    assert U32(0x7FC00000) == bits(ref["e1"][~valid]).max() == bits(ref["e1"][~valid]).min()
    empty = node_strain_reference(u, v, np.zeros_like(state), None, 8, 2, 1)
    assert empty["stats"]["valid"][0] == 0 and reasons(empty) == [nw * nh, 0, 0] and empty["stats"]["e1"]["min"][0] == 0
