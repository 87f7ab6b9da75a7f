"""flow2d_node_strain_robust_2d restated in numpy from the text of include/flow2d_c_abi.h (np.float64 operations in the stated
order, vectorised over the nodes with Python loops over the passes and over the window's offsets in raster order), with its
diagnostic planes and its record, and what can be checked without a device: that pass 0 alone is flow2d_node_strain_2d, that
planted outliers are rejected and named on exact fields, that a window which would lock onto its outlier comes out sparse, the
claim of profiles/robust_strain on the 176 x 144 rotation row, and the refusals of the entry, the host layer and the CLI."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

from test_deformation_cpu import F32, GREEN, NAN, PLANES, SMALL, STAT_NAMES, STATS_DTYPE, bits
from test_node_strain_cpu import (CENTRE, DEGENERATE, F64, MAX_WINDOW, SPARSE, affine_field, basis, node_case, node_positions,
                                  node_strain_reference, strain_quantities, usable_nodes)

MAX_ITERATIONS = 16  # FLOW2D_NODE_STRAIN_MAX_ITERATIONS
DIAGNOSTICS = ("residual", "rejected", "centre")
TOUCHED, REJECTED, SUSPECT = 3, 4, 5  # reserved[3 .. 5] of the record


def robust_window_fit(u, v, usable, s, m, order, min_nodes, sigma, passes):
    """(a, b, c, d, reason, n, kept, sum of the kept r2, r2 of the centre, finished) of the reweighted window fit for every node."""
    nh, nw = u.shape
    k = 3 if order == 1 else 6
    top = 2 * order
    pad = lambda x, fill: np.pad(x, m, constant_values=fill)  # noqa: E731
    pu, pv, pok = pad(u.astype(F64), 0.0), pad(v.astype(F64), 0.0), pad(usable, False)
    uc, vc = u.astype(F64), v.astype(F64)
    s2 = F64(F32(sigma)) * F64(F32(sigma))
    zeros = lambda *shape: np.zeros(shape + (nh, nw), F64)  # noqa: E731
    cu, cv = zeros(k), zeros(k)
    degenerate = np.zeros((nh, nw), bool)
    n = np.zeros((nh, nw), np.int64)
    kept = np.zeros((nh, nw), np.int64)
    kept_r2, centre_r2 = zeros(), zeros()
    exps = [(a in (1, 4)) + 2 * (a == 3) for a in range(6)], [(a in (2, 4)) + 2 * (a == 5) for a in range(6)]
    with np.errstate(all="ignore"):
        for t in range(passes + 2):
            fit = t <= passes
            S = {(p, q): zeros() for p in range(top + 1) for q in range(top + 1 - p)}
            bu, bv = zeros(k), zeros(k)
            for dj in range(-m, m + 1):
                for di in range(-m, m + 1):
                    sl = (slice(m + dj, m + dj + nh), slice(m + di, m + di + nw))
                    ok = pok[sl]
                    wu, wv = pu[sl] - uc, pv[sl] - vc
                    phi = basis(order, di, dj)
                    w, r2 = np.ones((nh, nw), F64), zeros()
                    if t > 0:
                        fu, fv = zeros(), zeros()
                        for a in range(k):
                            fu = fu + cu[a] * F64(phi[a])
                            fv = fv + cv[a] * F64(phi[a])
                        ru, rv = wu - fu, wv - fv
                        r2 = ru * ru + rv * rv
                        w = s2 / (s2 + r2)
                    if fit:
                        if t == 0:
                            n += ok
                        # a skipped tap adds nothing: + 0.0 leaves a sum that started at +0 as it is, bit for bit
                        for (p, q) in S:
                            S[p, q] += np.where(ok, w * F64(di ** p * dj ** q), 0.0)
                        for a in range(k):
                            wphi = w * F64(phi[a])
                            bu[a] += np.where(ok, wphi * wu, 0.0)
                            bv[a] += np.where(ok, wphi * wv, 0.0)
                    else:
                        keep = ok & (r2 <= s2)
                        kept += keep
                        kept_r2 += np.where(keep, r2, 0.0)
                        if di == 0 and dj == 0:
                            centre_r2 = r2
            if not fit:
                break
            H = np.array([[S[exps[0][a] + exps[0][b], exps[1][a] + exps[1][b]] for b in range(k)] for a in range(k)])
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

            def solve(b):
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

            cu, cv = solve(bu), solve(bv)
        sd = F64(s)
        grad = (cu[1] / sd, cu[2] / sd, cv[1] / sd, cv[2] / sd)
    # (a node that is sparse by its n is never factored; one that turned degenerate in a pass takes no further pass)
    reason = np.where(~usable, CENTRE, np.where(~(n >= min_nodes), SPARSE,
                                                np.where(degenerate, DEGENERATE, np.where(~(kept >= min_nodes), SPARSE, -1))))
    # finished: the passes ran to the end -- the node is valid, or sparse by what it kept
    return grad + (reason, n, kept, kept_r2, centre_r2, usable & (n >= min_nodes) & ~degenerate)


def node_strain_robust_reference(u, v, state=None, s=8, m=2, order=1, min_nodes=None, min_state=1, measure=SMALL, sigma=0.05,
                                 iterations=8):
    """What node_strain_reference gives -- the nine planes, "gradient", "valid", "reason", "stats" with "abs_sum" / "abs_sum_sq"
    -- with the planes of DIAGNOSTICS, "finished", "suspect" (both over the finished nodes, valid or not) and the record's
    reserved[3 .. 5]."""
    u, v = np.ascontiguousarray(u, F32), np.ascontiguousarray(v, F32)
    assert 1 <= s <= 64 and 1 <= m <= MAX_WINDOW and min_state in (0, 1) and order in (1, 2)
    assert np.isfinite(sigma) and sigma > 0 and 0 <= iterations <= MAX_ITERATIONS
    k = 3 if order == 1 else 6
    min_nodes = k + 1 if min_nodes is None else min_nodes
    assert k <= min_nodes <= (2 * m + 1) ** 2
    usable = usable_nodes(u, v, state, None, min_state)
    a, b, c, d, reason, n, kept, kept_r2, centre_r2, finished = robust_window_fit(u, v, usable, s, m, order, min_nodes, sigma, iterations)
    valid = reason == -1
    q = strain_quantities(a, b, c, d, measure)
    out = {name: np.where(valid, q[name], NAN).astype(F32) for name in PLANES}
    s2 = F64(F32(sigma)) * F64(F32(sigma))
    with np.errstate(all="ignore"):
        out["residual"] = np.where(valid, np.sqrt(kept_r2 / kept.astype(F64)).astype(F32), NAN).astype(F32)
        out["rejected"] = np.where(valid, (n - kept).astype(F32), NAN).astype(F32)
        out["centre"] = np.where(valid, np.sqrt(centre_r2).astype(F32), NAN).astype(F32)
        suspect = finished & ~(centre_r2 <= s2)
    stats = np.zeros(1, STATS_DTYPE)
    count = int(valid.sum())
    stats["valid"], stats["invalid"] = count, valid.size - count
    for r in (CENTRE, SPARSE, DEGENERATE):
        stats["reserved"][0][r] = int((reason == r).sum())
    rejected = np.where(finished, n - kept, 0)
    stats["reserved"][0][TOUCHED] = int((rejected > 0).sum())
    stats["reserved"][0][REJECTED] = int(rejected.sum())
    stats["reserved"][0][SUSPECT] = int(suspect.sum())
    out["abs_sum"], out["abs_sum_sq"] = {}, {}
    for name in STAT_NAMES:
        x = out[name][valid].astype(F64)  # raster order
        stats[name]["sum"], stats[name]["sum_sq"] = x.sum(), (x * x).sum()
        if count:
            stats[name]["min"], stats[name]["max"] = x.min(), x.max()
        out["abs_sum"][name], out["abs_sum_sq"][name] = float(np.abs(x).sum()), float((x * x).sum())
    out.update(gradient=(a, b, c, d), valid=valid, reason=reason, stats=stats, finished=finished, suspect=suspect, n=n, kept=kept)
    return out


def robust_words(ref):
    return [int(ref["stats"]["reserved"][0][r]) for r in (TOUCHED, REJECTED, SUSPECT)]


@pytest.mark.parametrize("measure", [SMALL, GREEN])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("nw,nh,m", [(1, 1, 1), (3, 3, 1), (5, 1, 2), (21, 13, 2), (30, 9, 7)])
def test_pass_0_alone_is_the_plain_entry(nw, nh, m, order, measure):
    """K = 0 with a sigma no residual reaches: every weight is 1.0, the sums are the plain entry's and every tap is kept."""
    u, v, state, _ = node_case(nw, nh, seed=m + order)
    for st in (state, None):
        plain = node_strain_reference(u, v, st, None, 8, m, order, measure=measure)
        got = node_strain_robust_reference(u, v, st, 8, m, order, measure=measure, sigma=1e6, iterations=0)
        for name in PLANES:
            assert np.array_equal(bits(got[name]), bits(plain[name])), name
        assert np.array_equal(got["reason"], plain["reason"])
        assert got["stats"].tobytes() == plain["stats"].tobytes() and robust_words(got) == [0, 0, 0]
        valid = got["valid"]
        assert (got["rejected"][valid] == 0).all() and np.isnan(got["rejected"][~valid]).all()
        assert np.isnan(got["residual"][~valid]).all() and np.isnan(got["centre"][~valid]).all()


# Gradients and an offset that are multiples of 2^-10, second-order terms that are multiples of 2^-13: with integer pixel
# coordinates below 256 every node value is exact in fp32, so the clean field's fit is the field's gradient to the last digits
# of a double and the 1e-9 below is a bound on what a rejected tap still pulls.
EXACT_G = (3 / 1024, -2 / 1024, 1.5 / 1024, 2.5 / 1024)
# sigma and the outliers' size.  A rejected tap at distance r from the fit keeps the Cauchy weight s2 / (s2 + r^2) < s2 / r^2 and
# pulls the right-hand side by less than s2 / r pixels.  What that moves the slope by is the tap's differentiation weight over
# the spacing: at most 1 in node units for order 1 (one tap of a 2 x 2 corner window), and for order 2 at the corner of a
# one-sided window the slope is extrapolated -- (-3, 4, -1) / 2 along a line of three, so up to 2 per axis and no more than 4
# with the mixed term.  sigma = 3e-5 and r >= 3 px: 9e-10 / 3 * 4 / 8 = 1.5e-10 < 1e-9.  (A first choice of sigma = 1e-4 counted the
# weight as 1 and left 1.4e-9 at an order-2 corner; the fields are exact, so a small sigma costs nothing.)
PLANT_SIGMA, PLANT_SIZE = 3e-5, 3.0


def exact_field(nw, nh, s, quadratic):
    u, v = affine_field(nw, nh, s, EXACT_G)
    if quadratic:
        x, y = node_positions(nw, nh, s, 7)
        u = (u.astype(F64) + (x * x - x * y) / 8192).astype(F32)
        v = (v.astype(F64) + (y * y) / 8192).astype(F32)
    return u, v


def planted_cases(nw, nh):
    """(name, planted nodes as (j, i), a state plane or None)."""
    hole = np.ones((nh, nw), F32)
    hole[4, 6] = np.nan
    return [("interior", [(4, 5)], None), ("corner", [(0, 0)], None), ("adjacent", [(3, 7), (3, 8)], None),
            ("beside a NaN-state hole", [(4, 7)], hole)]


@pytest.mark.parametrize("m,order", [(1, 1), (2, 1), (3, 1), (2, 2), (3, 2)])
def test_planted_outliers_are_rejected_and_named(m, order):
    nw, nh, s = 14, 10, 8
    min_nodes = (3 if order == 1 else 6) + 1
    for quadratic in ((False, True) if order == 2 else (False,)):
        cu, cv = exact_field(nw, nh, s, quadratic)
        assert np.array_equal(cu.astype(F64), exact_field(nw, nh, s, quadratic)[0].astype(F64))
        for name, planted, state in planted_cases(nw, nh):
            clean = node_strain_robust_reference(cu, cv, state, s, m, order, sigma=PLANT_SIGMA)
            assert robust_words(clean) == [0, 0, 0]
            u, v = cu.copy(), cv.copy()
            for k, (j, i) in enumerate(planted):
                u[j, i] += F32(PLANT_SIZE + k)
                v[j, i] -= F32(0.5 * PLANT_SIZE)
            got = node_strain_robust_reference(u, v, state, s, m, order, sigma=PLANT_SIGMA)
            mark = np.zeros((nh, nw), np.int64)
            for j, i in planted:
                mark[j, i] = 1
            usable = np.ones((nh, nw), bool) if state is None else state >= 1
            pm, pk = np.pad(mark, m), np.pad(usable, m)
            inside = sum(pm[m + dj:m + dj + nh, m + di:m + di + nw] for dj in range(-m, m + 1) for di in range(-m, m + 1))
            n = sum(pk[m + dj:m + dj + nh, m + di:m + di + nw].astype(np.int64) for dj in range(-m, m + 1) for di in range(-m, m + 1))
            enough = usable & (n - inside >= min_nodes)
            what = "%s m %d order %d quadratic %s" % (name, m, order, quadratic)
            assert np.array_equal(got["valid"], enough), what
            assert (got["reason"][usable & ~enough] == SPARSE).all(), what
            worst = max(float(np.abs(a[enough] - b[enough]).max()) for a, b in zip(got["gradient"], clean["gradient"]))
            print("%s: %d valid nodes, worst gradient difference from the clean field's %.3g" % (what, enough.sum(), worst))
            assert worst <= 1e-9, what
            assert np.array_equal(got["rejected"][enough], inside[enough].astype(F32)), what
            # the suspects: every planted node that is delivered, and nothing but planted nodes -- one whose own window keeps too
            # few is sparse, and suspect or not by whether its passes locked onto it
            lost = got["finished"] & ~enough
            assert np.array_equal(got["suspect"] & enough, enough & (mark == 1)) and not (got["suspect"] & (mark == 0)).any(), what
            assert (lost <= (inside > 0)).all(), what
            # the record counts over the finished nodes: the delivered ones as the planes say, and the lost ones
            gone = (got["n"] - got["kept"])[lost]
            assert (gone > 0).all(), what
            assert robust_words(got) == [int((inside[enough] > 0).sum()) + int(lost.sum()), int(inside[enough].sum()) + int(gone.sum()),
                                         int(got["suspect"].sum())], what
            assert (got["centre"][got["suspect"] & enough] > 2).all() and (got["residual"][enough] <= PLANT_SIGMA).all(), what


def test_a_window_that_would_lock_on_comes_out_sparse():
    """The 2 x 2 window of a corner node at m = 1 holds four nodes and min_nodes is four: with one of them an outlier no three
    nodes are enough, whichever three the passes settle on -- three points determine an order-1 fit, which then passes through
    them.  The plain fit delivers the node, bent."""
    nw, nh, s = 6, 5, 8
    u, v = exact_field(nw, nh, s, False)
    u[1, 0] += F32(2.5)
    plain = node_strain_reference(u, v, None, None, s, 1, 1)
    assert plain["valid"][0, 0] and abs(plain["gradient"][1][0, 0] - EXACT_G[1]) > 0.05
    got = node_strain_robust_reference(u, v, None, s, 1, 1, sigma=0.05)
    assert got["reason"][0, 0] == SPARSE and got["n"][0, 0] == 4 and got["kept"][0, 0] <= 3
    assert np.isnan(got["exx"][0, 0]) and np.isnan(got["rejected"][0, 0])
    # the outlier itself has a 2 x 3 window: five clean nodes, delivered and suspect
    assert got["valid"][1, 0] and got["suspect"][1, 0] and got["rejected"][1, 0] == 1


TABLE_FITS = ((1, 1), (2, 1), (3, 1), (2, 2), (3, 2))
TABLE_SIGMA, TABLE_PASSES = 0.05, 8


@pytest.fixture(scope="module")
def rows():
    """{(deformation, width, height): (nodes, true exx, true eyy)} of step 2 of the chained sequences: the nodes of
    tools/node_strain_table.py's rows."""
    sc = importlib.import_module("cuda-flow2d_amd.scenes")
    T = importlib.import_module("test_subset_sequence_cpu")
    out = {}
    for name, w, h in (("rotation", 176, 144), ("rotation", 96, 80), ("stretch", 96, 80)):
        scenes = sc.make_speckle_deformation_sequence(name, 2, None, w, h, seed=0)
        got = T.chained(scenes, 7, 8, 7)[0][-1]
        gu, gv = scenes[-1].gt_u.astype(F64), scenes[-1].gt_v.astype(F64)
        out[name, w, h] = ({n: getattr(got, n) for n in got.NAMES}, (gu[0, -1] - gu[0, 0]) / (w - 1), (gv[-1, 0] - gv[0, 0]) / (h - 1))
    return out


def rms(plane, want):
    e = plane[np.isfinite(plane)].astype(F64) - want
    return float(np.sqrt(np.mean(e * e)))


def both_fits(row, m, order):
    nodes = row[0]
    plain = node_strain_reference(nodes["u"], nodes["v"], nodes["state"], None, 8, m, order)
    robust = node_strain_robust_reference(nodes["u"], nodes["v"], nodes["state"], 8, m, order, sigma=TABLE_SIGMA, iterations=TABLE_PASSES)
    return plain, robust


@pytest.mark.parametrize("m,order", TABLE_FITS)
def test_the_rotation_row_at_176_x_144(rows, m, order):
    """One node of 168 lies 2.47 px off: the plain windows that hold it are bent, the robust ones are not.  Every window that
    holds it rejects it -- 5, 15 and 29 of them at m = 1, 2, 3 -- and it is the one suspect.  At m = 1 its own window (five usable
    nodes, at the edge of the usable region) rejects it and one clean neighbour, keeps three and is sparse: the one node not
    delivered, still finished and so still counted, 6 rejected taps in all."""
    row = rows["rotation", 176, 144]
    plain, robust = both_fits(row, m, order)
    for name, want in (("exx", row[1]), ("eyy", row[2])):
        before, after = rms(plain[name], want), rms(robust[name], want)
        print("m %d order %d %s: RMS %.5f plain, %.5f robust (%.0f x), nodes %d -> %d" %
              (m, order, name, before, after, before / after, plain["valid"].sum(), robust["valid"].sum()))
        assert after <= 0.1 * before and after < 0.0005, name
    assert robust["valid"].sum() >= plain["valid"].sum() - 1
    words = robust_words(robust)
    print("m %d order %d: record words %s" % (m, order, words))
    assert words[2] == 1 and words[1] == {1: 6, 2: 15, 3: 29}[m]


@pytest.mark.parametrize("m,order", TABLE_FITS)
@pytest.mark.parametrize("name", ["rotation", "stretch"])
def test_clean_rows_do_not_change(rows, name, m, order):
    row = rows[name, 96, 80]
    plain, robust = both_fits(row, m, order)
    assert robust_words(robust) == [0, 0, 0] and np.array_equal(robust["valid"], plain["valid"])
    for q, want in (("exx", row[1]), ("eyy", row[2])):
        before, after = rms(plain[q], want), rms(robust[q], want)
        print("%s m %d order %d %s: RMS %.6f plain, %.6f robust" % (name, m, order, q, before, after))
        assert abs(after / before - 1) <= 0.05, q


def test_refusals_without_a_device(flow2d):
    """What flow2d_node_strain_robust_2d refuses before it looks at its context (the pointers are never followed)."""
    lib = flow2d.hip_lib()
    nw, nh, pitch = 40, 30, 256
    span = pitch * nh
    base = 1 << 20
    ptr = lambda k: base + 2 * k * span  # noqa: E731
    need = lib.flow2d_node_strain_robust_workspace_bytes(nw, nh, 1)
    assert need == 224 * 8 and lib.flow2d_node_strain_robust_workspace_bytes(nw, nh, 3) == 3 * need
    assert lib.flow2d_node_strain_robust_workspace_bytes(0, nh, 1) == 0
    d = dict(u=ptr(0), v=ptr(1), state=ptr(2), nw=nw, nh=nh, pitch=pitch, s=8, m=2, order=1, min_nodes=4, min_state=1, measure=SMALL,
             sigma=0.05, iterations=8, planes={"exx": ptr(3)}, diag={"residual": ptr(4), "rejected": ptr(5), "centre": ptr(6)},
             stats=ptr(7), ws=ptr(8), ws_bytes=need)
    fake = ctypes.create_string_buffer(4096)  # never read: every call below is refused, or refused for its null context

    def call(ctx=ctypes.addressof(fake), **kw):
        a = dict(d, **kw)
        out = flow2d.DeformationPlanes(**a["planes"])
        diag = flow2d.NodeStrainDiagnostics(**a["diag"])
        return lib.flow2d_node_strain_robust_2d(ctx, a["u"], a["v"], a["state"], a["nw"], a["nh"], a["pitch"], a["s"], a["m"], a["order"],
                                                a["min_nodes"], a["min_state"], a["measure"], a["sigma"], a["iterations"],
                                                ctypes.byref(out), ctypes.byref(diag), a["stats"], a["ws"], a["ws_bytes"])

    assert call(ctx=None) == 1
    bad = [dict(u=None), dict(v=None), dict(planes={}, diag={}, stats=None), dict(nw=0), dict(nh=0), dict(pitch=pitch + 8), dict(pitch=16),
           dict(s=0), dict(s=65), dict(m=0), dict(m=-1), dict(m=8), dict(order=0), dict(order=3), dict(min_nodes=2), dict(min_nodes=26),
           dict(order=2, min_nodes=5), dict(min_state=2), dict(measure=2), dict(sigma=0.0), dict(sigma=-0.05), dict(sigma=float("nan")),
           dict(sigma=float("inf")), dict(iterations=-1), dict(iterations=MAX_ITERATIONS + 1), dict(state=ptr(2) + 4),
           dict(stats=ptr(7) + 4), dict(ws=ptr(8) + 8), dict(ws=None), dict(ws_bytes=need - 1), dict(diag={"residual": ptr(0)}),
           dict(diag={"rejected": ptr(1) + span - pitch}), dict(diag={"centre": ptr(2)}), dict(diag={"residual": ptr(3)}),
           dict(diag={"residual": ptr(4), "centre": ptr(4)}), dict(diag={"rejected": ptr(7)}), dict(diag={"centre": ptr(8)}),
           dict(diag={"residual": ptr(4) + 2}), dict(planes={"e1": ptr(0)})]
    for kw in bad:
        assert call(**kw) == 1, kw
    assert call(nw=1 << 16, nh=1 << 15, pitch=4 << 16, stats=None, planes={"exx": 1 << 50}, diag={}) == 5  # 2^31 nodes


def test_strain_options(flow2d):
    ok = flow2d.OpticalFlow.strain_options_ok
    assert ok(2, 1) and ok(2, 1, sigma=0.05) and ok(2, 2, sigma=0.05, iterations=0) and ok(7, 1, sigma=1e6, iterations=MAX_ITERATIONS)
    assert ok(0, 1) and ok(0, 1, sigma=0.0, iterations=99)  # off: the iterations are not looked at
    for kw in (dict(window=0, sigma=0.05), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")),
               dict(sigma=0.05, iterations=-1), dict(sigma=0.05, iterations=MAX_ITERATIONS + 1)):
        assert not ok(**dict(dict(window=2, order=1), **kw)), kw


def test_cli_usage_errors(flow2d):
    """--strain-sigma needs --subset-strain M with M >= 1, a positive finite S and K in its limits: a usage error before any
    file is read or a device opened."""
    base = [flow2d.CLI_PATH, "--correlation", "7", "--subset-refine", "7"]
    for extra in (["--strain-sigma", "0.05"], ["--subset-strain", "0", "--strain-sigma", "0.05"],
                  ["--subset-strain", "2", "--strain-sigma", "0"], ["--subset-strain", "2", "--strain-sigma", "-1"],
                  ["--subset-strain", "2", "--strain-sigma", "nan"], ["--subset-strain", "2", "--strain-sigma"],
                  ["--subset-strain", "2", "--strain-iterations", "4"],
                  ["--subset-strain", "2", "--strain-sigma", "0.05", "--strain-iterations", "17"],
                  ["--subset-strain", "2", "--strain-sigma", "0.05", "--strain-iterations", "-1"]):
        run = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60,
                             env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert run.returncode == 5 and "--strain-" in run.stdout, (extra, run.returncode, run.stdout[-300:])
