"""flow2d_node_strain_weighted_2d restated in numpy from the text of include/flow2d_c_abi.h (np.float64 operations in the stated
order, vectorised over the nodes with Python loops over the passes and over the window's offsets in raster order; the Cholesky
factorisation, Solve and the window walk in the form of tests/test_node_strain_cpu.py and tests/test_node_strain_robust_cpu.py),
with its diagnostic planes, its nine sigma planes and its record, and what can be checked without a device: the two exact
properties of the header, every early exit with its reason and count, a planted outlier rejected at three sigmas, the
Green-Lagrange sigmas against a finite-difference Jacobian, the calibration of the predicted sigma and the gain over the plain
fit on independent synthetic node noise, and the refusals of the entry, the host layer and the CLI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_deformation_cpu import F32, GREEN, NAN, PLANES, SMALL, STAT_NAMES, STATS_DTYPE, bits
from test_node_strain_cpu import (CENTRE, DEGENERATE, F64, MAX_WINDOW, SPARSE, affine_field, basis, node_case, node_strain_reference,
                                  strain_quantities, usable_nodes)
from test_node_strain_robust_cpu import DIAGNOSTICS, MAX_ITERATIONS, REJECTED, SUSPECT, TOUCHED

SIGMAS = ("sigma_ux", "sigma_uy", "sigma_vx", "sigma_vy", "sigma_divergence", "sigma_vorticity", "sigma_exx", "sigma_eyy", "sigma_exy")
UNWEIGHABLE = 6  # reserved[6] of the record


def cholesky(H, degenerate):
    """The factor of the header for every node at once; a failed pivot test is recorded in `degenerate`."""
    k = H.shape[0]
    zeros = lambda: np.zeros(H.shape[2:], F64)  # noqa: E731
    L = np.zeros_like(H)
    for kk in range(k):
        total = zeros()
        for j in range(kk):
            total = total + L[kk, j] * L[kk, j]
        d = H[kk, kk] - total
        degenerate |= ~(d > 1e-10 * H[kk, kk])
        L[kk, kk] = np.sqrt(d)
        for i in range(kk + 1, k):
            inner = zeros()
            for j in range(kk):
                inner = inner + L[i, j] * L[kk, j]
            L[i, kk] = (H[i, kk] - inner) / L[kk, kk]
    return L


def solve(L, b):
    k = L.shape[0]
    zeros = lambda: np.zeros(L.shape[2:], F64)  # noqa: E731
    y, x = np.zeros_like(b), np.zeros_like(b)
    for i in range(k):
        total = zeros()
        for j in range(i):
            total = total + L[i, j] * y[j]
        y[i] = (b[i] - total) / L[i, i]
    for i in range(k - 1, -1, -1):
        total = zeros()
        for j in range(i + 1, k):
            total = total + L[j, i] * x[j]
        x[i] = (y[i] - total) / L[i, i]
    return x


def weighted_window_fit(u, v, usable, su, sv, s, m, order, min_nodes, floor, threshold, passes):
    """A dict of the weighted window fit for every node: the gradients, the six covariances, reason, n, kept, the sum of the kept
    r2, the centre's r2, finished and weighable."""
    nh, nw = u.shape
    k = 3 if order == 1 else 6
    top = 2 * order
    f2 = F64(F32(floor)) * F64(F32(floor))
    t2 = F64(F32(threshold)) * F64(F32(threshold))
    zeros = lambda *shape: np.zeros(shape + (nh, nw), F64)  # noqa: E731
    with np.errstate(all="ignore"):
        vu = su.astype(F64) * su.astype(F64) + f2
        vv = sv.astype(F64) * sv.astype(F64) + f2
        weighable = usable & (vu > 0) & (vv > 0) & (vu < np.inf) & (vv < np.inf)
        inv_u, inv_v = np.where(weighable, 1.0 / vu, 0.0), np.where(weighable, 1.0 / vv, 0.0)
    pad = lambda x, fill: np.pad(x, m, constant_values=fill)  # noqa: E731
    pu, pv, pok = pad(u.astype(F64), 0.0), pad(v.astype(F64), 0.0), pad(weighable, False)
    ppu, ppv = pad(inv_u, 0.0), pad(inv_v, 0.0)
    uc, vc = u.astype(F64), v.astype(F64)
    cu, cv = zeros(k), zeros(k)
    degenerate = np.zeros((nh, nw), bool)
    n = np.zeros((nh, nw), np.int64)
    kept = np.zeros((nh, nw), np.int64)
    kept_r2, centre_r2 = zeros(), zeros()
    exps = [(a in (1, 4)) + 2 * (a == 3) for a in range(6)], [(a in (2, 4)) + 2 * (a == 5) for a in range(6)]
    Lu = Lv = None
    with np.errstate(all="ignore"):
        for t in range(passes + 2):
            fit = t <= passes
            Su = {(p, q): zeros() for p in range(top + 1) for q in range(top + 1 - p)}
            Sv = {key: zeros() for key in Su}
            bu, bv = zeros(k), zeros(k)
            for dj in range(-m, m + 1):
                for di in range(-m, m + 1):
                    sl = (slice(m + dj, m + dj + nh), slice(m + di, m + di + nw))
                    ok = pok[sl]
                    wu, wv = pu[sl] - uc, pv[sl] - vc
                    qu, qv = ppu[sl], ppv[sl]
                    phi = basis(order, di, dj)
                    c, r2 = np.ones((nh, nw), F64), zeros()
                    if t > 0:
                        fu, fv = zeros(), zeros()
                        for a in range(k):
                            fu = fu + cu[a] * F64(phi[a])
                            fv = fv + cv[a] * F64(phi[a])
                        ru, rv = wu - fu, wv - fv
                        r2 = (ru * ru) * qu + (rv * rv) * qv
                        c = t2 / (t2 + r2)
                    if fit:
                        if t == 0:
                            n += ok
                        # a skipped tap adds nothing: + 0.0 leaves a sum that started at +0 as it is, bit for bit
                        for S, b, p, w in ((Su, bu, c * qu, wu), (Sv, bv, c * qv, wv)):
                            for (e, f) in S:
                                S[e, f] += np.where(ok, p * F64(di ** e * dj ** f), 0.0)
                            for a in range(k):
                                b[a] += np.where(ok, (p * F64(phi[a])) * w, 0.0)
                    else:
                        keep = ok & (r2 <= t2) if t2 > 0 else ok
                        kept += keep
                        kept_r2 += np.where(keep, r2, 0.0)
                        if di == 0 and dj == 0:
                            centre_r2 = r2
            if not fit:
                break
            matrix = lambda S: np.array([[S[exps[0][a] + exps[0][b], exps[1][a] + exps[1][b]] for b in range(k)] for a in range(k)])  # noqa: E731
            Lu, Lv = cholesky(matrix(Su), degenerate), cholesky(matrix(Sv), degenerate)
            cu, cv = solve(Lu, bu), solve(Lv, bv)
        sd = F64(s)
        ss = sd * sd
        grad = (cu[1] / sd, cu[2] / sd, cv[1] / sd, cv[2] / sd)
        e1, e2 = zeros(k), zeros(k)
        e1[1], e2[2] = 1.0, 1.0
        xu1, xu2, xv1, xv2 = solve(Lu, e1), solve(Lu, e2), solve(Lv, e1), solve(Lv, e2)
        cov = dict(Vaa=xu1[1] / ss, Vab=xu1[2] / ss, Vbb=xu2[2] / ss, Vcc=xv1[1] / ss, Vcd=xv1[2] / ss, Vdd=xv2[2] / ss)
    # (a node that is sparse by its n is never factored; one that turned degenerate in a pass takes no further pass)
    reason = np.where(~weighable, CENTRE, np.where(~(n >= min_nodes), SPARSE,
                                                   np.where(degenerate, DEGENERATE, np.where(~(kept >= min_nodes), SPARSE, -1))))
    return dict(cov, gradient=grad, reason=reason, n=n, kept=kept, kept_r2=kept_r2, centre_r2=centre_r2,
                finished=weighable & (n >= min_nodes) & ~degenerate, weighable=weighable, t2=t2)


def strain_sigmas(a, b, c, d, V, measure):
    """The nine standard deviations in double from the gradients and the six covariances, each cast to float once."""
    Vaa, Vab, Vbb, Vcc, Vcd, Vdd = (V[name] for name in ("Vaa", "Vab", "Vbb", "Vcc", "Vcd", "Vdd"))
    with np.errstate(all="ignore"):
        if measure == SMALL:
            Vexx, Veyy, Vexy = Vaa, Vdd, 0.25 * (Vbb + Vcc)
        else:
            assert measure == GREEN
            ja, jd = 1.0 + a, 1.0 + d
            Vexx = (ja * ja) * Vaa + (c * c) * Vcc
            Veyy = (b * b) * Vbb + (jd * jd) * Vdd
            Qu = ((b * b) * Vaa + (2.0 * (b * ja)) * Vab) + (ja * ja) * Vbb
            Qv = ((jd * jd) * Vcc + (2.0 * (jd * c)) * Vcd) + (c * c) * Vdd
            Vexy = 0.25 * (Qu + Qv)
        q = dict(sigma_ux=Vaa, sigma_uy=Vbb, sigma_vx=Vcc, sigma_vy=Vdd, sigma_divergence=Vaa + Vdd, sigma_vorticity=Vbb + Vcc,
                 sigma_exx=Vexx, sigma_eyy=Veyy, sigma_exy=Vexy)
        return {name: np.sqrt(np.asarray(x, F64)).astype(F32) for name, x in q.items()}


def node_strain_weighted_reference(u, v, su, sv, state=None, s=8, m=2, order=1, min_nodes=None, min_state=1, measure=SMALL, floor=0.0,
                                   threshold=0.0, iterations=0):
    """What node_strain_robust_reference gives -- the nine planes, DIAGNOSTICS (residual and centre in sigmas), "gradient", "valid",
    "reason", "stats", "finished", "suspect" -- with the planes of SIGMAS, "covariance", "weighable" and the record's reserved[6]."""
    u, v, su, sv = (np.ascontiguousarray(x, F32) for x in (u, v, su, sv))
    assert 1 <= s <= 64 and 1 <= m <= MAX_WINDOW and min_state in (0, 1) and order in (1, 2)
    assert np.isfinite(floor) and floor >= 0 and np.isfinite(threshold) and threshold >= 0
    assert 0 <= iterations <= MAX_ITERATIONS and (iterations == 0 or threshold > 0)
    k = 3 if order == 1 else 6
    min_nodes = k + 1 if min_nodes is None else min_nodes
    assert k <= min_nodes <= (2 * m + 1) ** 2
    usable = usable_nodes(u, v, state, None, min_state)
    fit = weighted_window_fit(u, v, usable, su, sv, s, m, order, min_nodes, floor, threshold, iterations)
    a, b, c, d = fit["gradient"]
    reason, n, kept, finished = fit["reason"], fit["n"], fit["kept"], fit["finished"]
    valid = reason == -1
    q = strain_quantities(a, b, c, d, measure)
    out = {name: np.where(valid, q[name], NAN).astype(F32) for name in PLANES}
    sg = strain_sigmas(a, b, c, d, fit, measure)
    out.update({name: np.where(valid, sg[name], NAN).astype(F32) for name in SIGMAS})
    with np.errstate(all="ignore"):
        out["residual"] = np.where(valid, np.sqrt(fit["kept_r2"] / kept.astype(F64)).astype(F32), NAN).astype(F32)
        out["rejected"] = np.where(valid, (n - kept).astype(F32), NAN).astype(F32)
        out["centre"] = np.where(valid, np.sqrt(fit["centre_r2"]).astype(F32), NAN).astype(F32)
        suspect = finished & ~(fit["centre_r2"] <= fit["t2"]) if fit["t2"] > 0 else np.zeros_like(finished)
    stats = np.zeros(1, STATS_DTYPE)
    count = int(valid.sum())
    stats["valid"], stats["invalid"] = count, valid.size - count
    for r in (CENTRE, SPARSE, DEGENERATE):
        stats["reserved"][0][r] = int((reason == r).sum())
    rejected = np.where(finished, n - kept, 0)
    stats["reserved"][0][TOUCHED] = int((rejected > 0).sum())
    stats["reserved"][0][REJECTED] = int(rejected.sum())
    stats["reserved"][0][SUSPECT] = int(suspect.sum())
    stats["reserved"][0][UNWEIGHABLE] = int((usable & ~fit["weighable"]).sum())
    out["abs_sum"], out["abs_sum_sq"] = {}, {}
    for name in STAT_NAMES:
        x = out[name][valid].astype(F64)  # raster order
        stats[name]["sum"], stats[name]["sum_sq"] = x.sum(), (x * x).sum()
        if count:
            stats[name]["min"], stats[name]["max"] = x.min(), x.max()
        out["abs_sum"][name], out["abs_sum_sq"][name] = float(np.abs(x).sum()), float((x * x).sum())
    out.update(gradient=(a, b, c, d), valid=valid, reason=reason, stats=stats, finished=finished, suspect=suspect, n=n, kept=kept,
               covariance={name: fit[name] for name in ("Vaa", "Vab", "Vbb", "Vcc", "Vcd", "Vdd")}, weighable=fit["weighable"],
               usable=usable)
    return out


def weighted_words(ref):
    return [int(ref["stats"]["reserved"][0][r]) for r in (TOUCHED, REJECTED, SUSPECT, UNWEIGHABLE)]


def sigma_case(nw, nh, seed, decade=True):
    """Two sigma planes, log-uniform over 0.005 .. 0.05 px, independent per node."""
    rng = np.random.default_rng(7000 + seed + 100 * nw + nh)
    span = np.log(10.0) if decade else 0.0
    return tuple((0.005 * np.exp(span * rng.random((nh, nw)))).astype(F32) for _ in range(2))


def record_without_weighted_words(ref):
    rec = ref["stats"].copy()
    rec["reserved"][0][TOUCHED:UNWEIGHABLE + 1] = 0
    return rec.tobytes()


@pytest.mark.parametrize("measure", [SMALL, GREEN])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("nw,nh,m", [(1, 1, 1), (3, 3, 1), (5, 1, 2), (21, 13, 2), (30, 9, 7)])
def test_property_a_unit_sigmas_give_the_plain_entry(nw, nh, m, order, measure):
    """Both sigma planes 1.0f, floor 0 and T = 0: every weight is 1.0, the sums are the plain entry's."""
    u, v, state, _ = node_case(nw, nh, seed=m + order)
    one = np.ones((nh, nw), F32)
    for st in (state, None):
        plain = node_strain_reference(u, v, st, None, 8, m, order, measure=measure)
        got = node_strain_weighted_reference(u, v, one, one, st, 8, m, order, measure=measure)
        for name in PLANES:
            assert np.array_equal(bits(got[name]), bits(plain[name])), name
        assert np.array_equal(got["reason"], plain["reason"])
        assert record_without_weighted_words(got) == plain["stats"].tobytes() and weighted_words(got) == [0, 0, 0, 0]
        valid = got["valid"]
        assert (got["rejected"][valid] == 0).all() and all(np.isnan(got[name][~valid]).all() for name in SIGMAS + DIAGNOSTICS)
        assert all(np.isfinite(got[name][valid]).all() for name in SIGMAS)


@pytest.mark.parametrize("measure", [SMALL, GREEN])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("nw,nh,m", [(9, 7, 1), (21, 13, 2), (30, 9, 7)])
def test_property_b_doubled_sigmas_double_the_strain_sigmas(nw, nh, m, order, measure):
    """T = 0: both sigma planes and the floor times 2 scale every sum by 1/4, a power of two -- no byte of `out` changes and
    every sigma plane doubles exactly."""
    u, v, state, _ = node_case(nw, nh, seed=m + order)
    su, sv = sigma_case(nw, nh, seed=m)
    for floor in (0.0, 0.0078125):
        once = node_strain_weighted_reference(u, v, su, sv, state, 8, m, order, measure=measure, floor=floor)
        twice = node_strain_weighted_reference(u, v, 2 * su, 2 * sv, state, 8, m, order, measure=measure, floor=2 * floor)
        assert once["valid"].any() and np.array_equal(once["reason"], twice["reason"])
        for name in PLANES:
            assert np.array_equal(bits(once[name]), bits(twice[name])), name
        for name in SIGMAS:
            assert np.array_equal(bits((2 * once[name]).astype(F32)), bits(twice[name])), name
        assert once["stats"].tobytes() == twice["stats"].tobytes()


def test_early_exits_reasons_and_counts():
    """A full 9 x 7 affine field, m = 1: nodes that are not weighable leave the windows like lost nodes, are invalid with the
    reason *centre* and are counted in reserved[6]; a sigma of +0 is weighable as soon as there is a floor."""
    nw, nh, s = 9, 7, 8
    u, v = affine_field(nw, nh, s)
    su, sv = (np.full((nh, nw), 0.01, F32) for _ in range(2))
    su[1, 1] = np.nan
    sv[1, 2] = np.inf
    su[3, 4] = 0.0
    sv[5, 7] = -0.01  # only the square of a sigma is looked at
    state = np.ones((nh, nw), F32)
    state[4, 0] = 0  # not usable: centre, but not counted as unweighable
    su[4, 0] = np.nan
    got = node_strain_weighted_reference(u, v, su, sv, state, s, 1, 1)
    unweighable = np.zeros((nh, nw), bool)
    unweighable[1, 1] = unweighable[1, 2] = unweighable[3, 4] = True
    assert np.array_equal(got["usable"] & ~got["weighable"], unweighable)
    assert np.array_equal(got["reason"] == CENTRE, unweighable | (state == 0))
    assert weighted_words(got) == [0, 0, 0, 3] and int(got["stats"]["reserved"][0][CENTRE]) == 4
    assert got["valid"][5, 7] and got["n"][3, 3] == 8 and got["n"][0, 0] == 3 and got["n"][2, 1] == 7
    # three taps are fewer than min_nodes = 4: sparse, before anything is factored
    assert got["reason"][0, 0] == SPARSE and int(got["stats"]["reserved"][0][SPARSE]) == 1
    for name in PLANES + SIGMAS + DIAGNOSTICS:
        assert np.isnan(got[name][~got["valid"]]).all() and np.isfinite(got[name][got["valid"]]).all(), name
    # with a floor the zero sigma is weighable; NaN and infinity stay out
    got = node_strain_weighted_reference(u, v, su, sv, state, s, 1, 1, floor=0.005)
    assert got["weighable"][3, 4] and got["valid"][3, 4] and weighted_words(got) == [0, 0, 0, 2]
    # a row of nodes: every window is collinear, the second pivot fails
    got = node_strain_weighted_reference(u[:1], v[:1], su[:1] * 0 + F32(0.01), sv[:1] * 0 + F32(0.01), None, s, 2, 1, min_nodes=3)
    assert (got["reason"] == DEGENERATE).all() and int(got["stats"]["reserved"][0][DEGENERATE]) == nw
    assert weighted_words(got) == [0, 0, 0, 0]


@pytest.mark.parametrize("m,order", [(1, 1), (2, 1), (2, 2), (3, 2)])
def test_a_planted_outlier_is_rejected_at_three_sigmas(m, order):
    """An exact affine field with sigma 0.01 px everywhere and one node 1 px (100 sigmas) off: at T = 3 with four passes every
    window that holds it and keeps enough rejects it, it is the one suspect, and the gradients are the clean field's.  A rejected
    tap 100 sigmas out keeps the weight 9 / (9 + r2) < 1e-3 of a clean one; what that still pulls is bounded by the tolerance
    below, 1e-3 * 1 px / s at the worst lever of 4 (tests/test_node_strain_robust_cpu.py derives the lever) over s = 8."""
    nw, nh, s = 14, 10, 8
    g = (3 / 1024, -2 / 1024, 1.5 / 1024, 2.5 / 1024)
    u, v = affine_field(nw, nh, s, g)
    sig = np.full((nh, nw), 0.01, F32)
    clean = node_strain_weighted_reference(u, v, sig, sig, None, s, m, order, threshold=3.0, iterations=4)
    assert clean["valid"].all() and weighted_words(clean) == [0, 0, 0, 0]
    u[4, 5] += F32(1.0)
    got = node_strain_weighted_reference(u, v, sig, sig, None, s, m, order, threshold=3.0, iterations=4)
    holds = np.zeros((nh, nw), bool)
    holds[max(0, 4 - m):4 + m + 1, max(0, 5 - m):5 + m + 1] = True
    assert got["valid"].all()
    assert np.array_equal(got["rejected"], holds.astype(F32))
    only = np.zeros((nh, nw), bool)
    only[4, 5] = True
    assert np.array_equal(got["suspect"], only)
    assert weighted_words(got) == [int(holds.sum()), int(holds.sum()), 1, 0]
    assert got["centre"][4, 5] > 50 and (got["residual"] <= 3).all()
    worst = max(float(np.abs(a - b).max()) for a, b in zip(got["gradient"], clean["gradient"]))
    print("m %d order %d: worst gradient difference from the clean field's %.3g" % (m, order, worst))
    assert worst <= 1e-3 * 4 / s
    # T = 0 keeps every tap whatever its residual: nothing rejected, nobody suspect, and the windows are bent
    plain = node_strain_weighted_reference(u, v, sig, sig, None, s, m, order)
    assert weighted_words(plain) == [0, 0, 0, 0] and (plain["rejected"] == 0).all()
    assert max(float(np.abs(a - b).max()) for a, b in zip(plain["gradient"], clean["gradient"])) > 1e-3


def measure_of(p, measure):
    a, b, c, d = p
    if measure == SMALL:
        return np.array([a, d, 0.5 * (b + c)])
    return np.array([a + 0.5 * (a * a + c * c), d + 0.5 * (b * b + d * d), 0.5 * ((b + c) + (a * b + c * d))])


@pytest.mark.parametrize("measure", [SMALL, GREEN])
@pytest.mark.parametrize("order", [1, 2])
def test_sigmas_against_a_finite_difference_jacobian(order, measure):
    """Every sigma plane at every valid node against J * Sigma * J^T, J the central-difference Jacobian of the measure's own
    formulas (they are quadratic: a central difference is exact up to rounding) and Sigma = inv(A^T W A) by numpy.linalg.inv,
    block-diagonal in u and v, at a relative 1e-6.  Large gradients (0.2), so that the Green-Lagrange terms count."""
    nw, nh, s, m = 9, 7, 4, 2
    k = 3 if order == 1 else 6
    u, v = affine_field(nw, nh, s, (0.2, -0.15, 0.1, 0.25))
    rng = np.random.default_rng(5)
    u = (u + 0.01 * rng.standard_normal((nh, nw))).astype(F32)
    su, sv = sigma_case(nw, nh, seed=order)
    state = np.where(rng.random((nh, nw)) < 0.15, 0, 5).astype(F32)
    got = node_strain_weighted_reference(u, v, su, sv, state, s, m, order, measure=measure, floor=0.002)
    assert got["valid"].sum() > 30
    f2 = F64(F32(0.002)) ** 2
    worst = 0.0
    for j, i in zip(*np.nonzero(got["valid"])):
        rows, wu, wv = [], [], []
        for dj in range(-m, m + 1):
            for di in range(-m, m + 1):
                y, x = j + dj, i + di
                if 0 <= y < nh and 0 <= x < nw and got["weighable"][y, x]:
                    rows.append(basis(order, di, dj))
                    wu.append(1.0 / (F64(su[y, x]) ** 2 + f2))
                    wv.append(1.0 / (F64(sv[y, x]) ** 2 + f2))
        A = np.array(rows, F64)
        cov = np.zeros((4, 4))
        cov[:2, :2] = np.linalg.inv(A.T @ (A * np.array(wu)[:, None]))[1:3, 1:3] / s ** 2
        cov[2:, 2:] = np.linalg.inv(A.T @ (A * np.array(wv)[:, None]))[1:3, 1:3] / s ** 2
        assert A.shape[1] == k
        p = np.array([g[j, i] for g in got["gradient"]])
        h = 1e-4
        J = np.array([(measure_of(p + h * e, measure) - measure_of(p - h * e, measure)) / (2 * h) for e in np.eye(4)]).T
        var = J @ cov @ J.T
        want = dict(sigma_ux=cov[0, 0], sigma_uy=cov[1, 1], sigma_vx=cov[2, 2], sigma_vy=cov[3, 3], sigma_divergence=cov[0, 0] + cov[3, 3],
                    sigma_vorticity=cov[1, 1] + cov[2, 2], sigma_exx=var[0, 0], sigma_eyy=var[1, 1], sigma_exy=var[2, 2])
        for name in SIGMAS:
            rel = abs(float(got[name][j, i]) / np.sqrt(want[name]) - 1)
            worst = max(worst, rel)
            assert rel <= 1e-6, (name, j, i, rel)
    print("order %d measure %d: worst relative difference %.3g" % (order, measure, worst))


def test_calibration_on_independent_node_noise():
    """21 x 13 nodes, m = 2, order 1, sigma log-uniform over a decade and independent per node, 200 draws of Gaussian node noise
    with those sigmas on an affine field.  Pooled over the nodes whose window is whole, sqrt(sum of predicted variance / sum of
    the draws' variance) of exx lies in 0.95 .. 1.05 (one sigma of a per-node scatter estimate from 200 draws is 5 %; the pool is
    far tighter), and the weighted fit's pooled scatter is at most 0.7 of the plain fit's."""
    nw, nh, s, m, draws = 21, 13, 8, 2, 200
    g = (0.003, -0.002, 0.0015, 0.0025)
    u0, v0 = affine_field(nw, nh, s, g)
    su, sv = sigma_case(nw, nh, seed=1)
    assert su.max() / su.min() > 8
    rng = np.random.default_rng(20260)
    weighted, plain, predicted = [], [], None
    for _ in range(draws):
        u = (u0 + su * rng.standard_normal((nh, nw))).astype(F32)
        v = (v0 + sv * rng.standard_normal((nh, nw))).astype(F32)
        got = node_strain_weighted_reference(u, v, su, sv, None, s, m, 1)
        assert got["valid"].all()
        weighted.append(got["gradient"][0])
        plain.append(node_strain_reference(u, v, None, None, s, m, 1)["gradient"][0])
        predicted = got["sigma_exx"].astype(F64)  # (the same in every draw: at T = 0 it depends on the sigmas alone)
    inner = (slice(m, nh - m), slice(m, nw - m))
    scatter_w = np.var(np.array(weighted), axis=0, ddof=1)[inner]
    scatter_p = np.var(np.array(plain), axis=0, ddof=1)[inner]
    ratio = float(np.sqrt((predicted[inner] ** 2).sum() / scatter_w.sum()))
    gain = float(np.sqrt(scatter_w.sum() / scatter_p.sum()))
    per_node = predicted[inner] / np.sqrt(scatter_w)
    bias = float(np.abs(np.mean(np.array(weighted), axis=0)[inner] - g[0]).max())
    print("%d nodes: predicted / empirical sigma_exx pooled %.4f, per node %.3f .. %.3f; weighted / plain scatter %.4f; worst mean "
          "error %.3g" % (scatter_w.size, ratio, per_node.min(), per_node.max(), gain, bias))
    assert 0.95 <= ratio <= 1.05
    assert gain <= 0.7


def test_refusals_without_a_device(flow2d):
    """What flow2d_node_strain_weighted_2d refuses before it looks at its context (the pointers are never followed)."""
    lib = flow2d.hip_lib()
    nw, nh, pitch = 40, 30, 256
    span = pitch * nh
    base = 1 << 20
    ptr = lambda k: base + 2 * k * span  # noqa: E731
    need = lib.flow2d_node_strain_weighted_workspace_bytes(nw, nh, 1)
    assert need == 224 * 8 and lib.flow2d_node_strain_weighted_workspace_bytes(nw, nh, 3) == 3 * need
    assert lib.flow2d_node_strain_weighted_workspace_bytes(0, nh, 1) == 0
    d = dict(u=ptr(0), v=ptr(1), state=ptr(2), su=ptr(3), sv=ptr(4), nw=nw, nh=nh, pitch=pitch, s=8, m=2, order=1, min_nodes=4, min_state=1,
             measure=SMALL, floor=0.005, threshold=3.0, iterations=4, planes={"exx": ptr(5)},
             diag={"residual": ptr(6), "rejected": ptr(7), "centre": ptr(8)}, sig={"sigma_exx": ptr(9), "sigma_exy": ptr(10)},
             stats=ptr(11), ws=ptr(12), ws_bytes=need)
    fake = ctypes.create_string_buffer(4096)  # never read: every call below is refused, or refused for its null context

    def call(ctx=ctypes.addressof(fake), **kw):
        a = dict(d, **kw)
        out = flow2d.DeformationPlanes(**a["planes"])
        diag = flow2d.NodeStrainDiagnostics(**a["diag"])
        sig = flow2d.StrainSigmaPlanes(**a["sig"])
        return lib.flow2d_node_strain_weighted_2d(ctx, a["u"], a["v"], a["state"], a["su"], a["sv"], a["nw"], a["nh"], a["pitch"], a["s"],
                                                  a["m"], a["order"], a["min_nodes"], a["min_state"], a["measure"], a["floor"],
                                                  a["threshold"], a["iterations"], ctypes.byref(out), ctypes.byref(diag), ctypes.byref(sig),
                                                  a["stats"], a["ws"], a["ws_bytes"])

    assert call(ctx=None) == 1
    nan, inf = float("nan"), float("inf")
    bad = [dict(u=None), dict(v=None), dict(su=None), dict(sv=None), dict(su=ptr(3) + 4), dict(planes={}, diag={}, sig={}, stats=None),
           dict(nw=0), dict(nh=0), dict(pitch=pitch + 8), dict(pitch=16), dict(s=0), dict(s=65), dict(m=0), dict(m=-1), dict(m=8),
           dict(order=0), dict(order=3), dict(min_nodes=2), dict(min_nodes=26), dict(order=2, min_nodes=5), dict(min_state=2),
           dict(measure=2), dict(floor=-0.005), dict(floor=nan), dict(floor=inf), dict(threshold=-1.0), dict(threshold=nan),
           dict(threshold=inf), dict(iterations=-1), dict(iterations=MAX_ITERATIONS + 1), dict(threshold=0.0, iterations=1),
           dict(state=ptr(2) + 4), dict(stats=ptr(11) + 4), dict(ws=ptr(12) + 8), dict(ws=None), dict(ws_bytes=need - 1),
           dict(diag={"residual": ptr(0)}), dict(sig={"sigma_ux": ptr(3)}), dict(sig={"sigma_vorticity": ptr(4) + span - pitch}),
           dict(planes={"e1": ptr(4)}), dict(diag={"centre": ptr(3)}), dict(sig={"sigma_exx": ptr(5)}),
           dict(sig={"sigma_exx": ptr(9), "sigma_eyy": ptr(9)}), dict(sig={"sigma_uy": ptr(11)}), dict(sig={"sigma_vy": ptr(12)}),
           dict(sig={"sigma_vx": ptr(9) + 2}), dict(planes={"e1": ptr(0)})]
    for kw in bad:
        assert call(**kw) == 1, kw
    assert call(nw=1 << 16, nh=1 << 15, pitch=4 << 16, stats=None, planes={"exx": 1 << 50}, diag={}, sig={}) == 5  # 2^31 nodes


def test_strain_options(flow2d):
    """OpticalFlow2D::StrainOptionsOk with `weighted`: a window to weight, a floor and a threshold that are finite and not
    negative, passes in their limits where there is a threshold, and no robust scale in pixels beside the one in sigmas."""
    ok = flow2d.OpticalFlow.strain_options_ok
    assert ok(2, 1, weighted=True) and ok(7, 2, weighted=True, sigma_floor=0.005, threshold=3.0, iterations=MAX_ITERATIONS)
    assert ok(1, 1, weighted=True, threshold=3.0, iterations=0) and ok(2, 1, weighted=True, iterations=99)  # T = 0: not looked at
    assert ok(2, 1) and ok(2, 1, sigma=0.05)  # the plain and the robust options are what they were
    nan, inf = float("nan"), float("inf")
    for kw in (dict(window=0), dict(sigma=0.05), dict(sigma_floor=-0.005), dict(sigma_floor=nan), dict(sigma_floor=inf),
               dict(threshold=-3.0), dict(threshold=nan), dict(threshold=inf), dict(threshold=3.0, iterations=-1),
               dict(threshold=3.0, iterations=MAX_ITERATIONS + 1), dict(order=3), dict(min_nodes=2), dict(measure=2)):
        assert not ok(**dict(dict(window=2, order=1, weighted=True), **kw)), kw
    # the object keeps the weighting for the weighted calls alone; what it refuses to store
    lib = flow2d.host_lib()
    for bad in ((1, -0.005, 0.0, 0), (1, nan, 0.0, 0), (1, 0.0, -1.0, 0), (1, 0.0, inf, 0), (1, 0.0, 3.0, -1), (1, 0.0, 3.0, MAX_ITERATIONS + 1)):
        assert lib.flow2d_host_set_strain_weighting(None, *bad) == 1, bad
    assert lib.flow2d_host_node_strain_weighted(None, None, None, 1, 8, 8, 8, 2, 1, 0, 1, 0, None, None, None) == 1
    assert lib.flow2d_host_node_strain_weighted_device(None, None, None, 1, 8, 8, 8, 2, 1, 0, 1, 0, None, None, None) == 1


def test_cli_usage_errors(flow2d):
    """--strain-weighted needs --subset-uncertainty and --subset-strain M with M >= 1, excludes --strain-sigma, and its floor,
    threshold and passes are checked: a usage error before any file is read or a device opened."""
    base = [flow2d.CLI_PATH, "--correlation", "7", "--subset-refine", "7"]
    full = ["--subset-uncertainty", "--subset-strain", "2", "--strain-weighted"]
    for extra in (["--strain-weighted"], ["--subset-strain", "2", "--strain-weighted"], ["--subset-uncertainty", "--strain-weighted"],
                  ["--subset-uncertainty", "--subset-strain", "0", "--strain-weighted"], full + ["--strain-sigma", "0.05"],
                  full + ["--strain-sigma-floor", "-0.005"], full + ["--strain-sigma-floor", "nan"], full + ["--strain-sigma-floor"],
                  full + ["--strain-threshold", "-1"], full + ["--strain-threshold", "inf"], full + ["--strain-threshold"],
                  full + ["--strain-iterations", "4"], full + ["--strain-threshold", "3", "--strain-iterations", "17"],
                  ["--subset-uncertainty", "--subset-strain", "2", "--strain-sigma-floor", "0.005"],
                  ["--subset-uncertainty", "--subset-strain", "2", "--strain-threshold", "3"]):
        run = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60,
                             env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert run.returncode == 5 and "--strain-" in run.stdout, (extra, run.returncode, run.stdout[-300:])


def test_a_window_that_keeps_too_few_is_sparse_and_still_counted():
    """The 2 x 2 window of a corner node at m = 1 holds four taps and min_nodes is four: with one of them 250 sigmas out no three
    are enough, whichever the passes settle on.  The node is sparse by what it kept, finished, and its rejected taps are in the
    record; the T = 0 fit delivers it, bent."""
    nw, nh, s = 6, 5, 8
    u, v = affine_field(nw, nh, s, (3 / 1024, -2 / 1024, 1.5 / 1024, 2.5 / 1024))
    sig = np.full((nh, nw), 0.01, F32)
    u[1, 0] += F32(2.5)
    bent = node_strain_weighted_reference(u, v, sig, sig, None, s, 1, 1)
    assert bent["valid"][0, 0] and abs(bent["gradient"][1][0, 0] + 2 / 1024) > 0.05
    got = node_strain_weighted_reference(u, v, sig, sig, None, s, 1, 1, threshold=3.0, iterations=4)
    assert got["reason"][0, 0] == SPARSE and got["finished"][0, 0] and got["n"][0, 0] == 4 and got["kept"][0, 0] <= 3
    assert all(np.isnan(got[name][0, 0]) for name in PLANES + SIGMAS + DIAGNOSTICS)
    words = weighted_words(got)
    lost = got["finished"] & ~got["valid"]
    assert lost[0, 0] and words[0] >= int(lost.sum()) + 1 and words[1] >= words[0] and words[3] == 0
    # the outlier itself has a 2 x 3 window: five clean taps, delivered and suspect
    assert got["valid"][1, 0] and got["suspect"][1, 0] and got["rejected"][1, 0] == 1
