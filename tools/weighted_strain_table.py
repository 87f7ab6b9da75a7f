#!/usr/bin/env python3
"""What weighting the strain windows by the nodes' own variances buys, and how well the delivered strain sigma predicts the
strain's scatter: noisy draws of two 96 x 80 scenes -- the stretch of the patchy speckle (scenes.make_speckle_patchy: the
contrast, and with it a node's sigma, varies by a decade from one 16-pixel patch to the next) and the stretch of the masked plate
with a hole (scenes.make_speckle_specimen: edge nodes with few usable pixels) --, Gaussian noise of 2 grey values on both
frames, 16 draws from default_rng(1); every draw refined from the truth rounded to whole pixels on the grid (7, s 8) with R = 7,
its uncertainty taken, and the strain fitted at m = 2, order 1 four ways: the plain fit (flow2d_node_strain_2d), the robust fit at
sigma = 0.05 px with K = 8 (flow2d_node_strain_robust_2d), and the weighted fit (flow2d_node_strain_weighted_2d, floor 0.005 px)
at T = 0 and at T = 3 with K = 4.  Per fit: the nodes valid in every draw, the RMS error of exx against the truth (0.06) over
those nodes and the draws, the scatter of exx (the standard deviation across the draws, pooled as an RMS over the nodes) and, for
the weighted fits, the predicted sigma_exx (an RMS over nodes and draws) and its ratio to the scatter.  Neighbouring subsets
overlap (R = 7 at spacing 8 shares one pixel column; the noise of frame 1 is resampled by both), so their errors are correlated
and the ratio need not be 1: it is reported, not asserted.

  python tools/weighted_strain_table.py --numpy    the rows of the numpy restatements, no device: writes
                                                   profiles/weighted_strain/table_numpy.md, the committed rows
  python tools/weighted_strain_table.py            the device's rows into OUT/table.md; they must equal the committed rows digit
                                                   for digit, else exit status 1
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
F32, F64 = np.float32, np.float64
W, H, GRID_R, SPACING, R = 96, 80, 7, 8, 7
NOISE, DRAWS, SEED = 2.0, 16, 1
M, ORDER, FLOOR = 2, 1, 0.005
TRUE_EXX = 0.06
FITS = ("plain", "robust 0.05 px, K 8", "weighted T 0", "weighted T 3, K 4")
HEADER = ("| scene | fit | nodes | RMS error exx | scatter exx | predicted sigma_exx | predicted / scatter | rejected taps |\n|" +
          "---|" * 8 + "\n")
NODE_NAMES = ("u", "v", "ux", "uy", "vx", "vy")


def scenes():
    sc = importlib.import_module("cuda-flow2d_amd.scenes")
    plate, mask = sc.make_speckle_specimen("stretch", W, H, seed=0)
    return (("patchy stretch", sc.make_speckle_patchy("stretch", W, H, seed=0), None), ("plate stretch (masked)", plate, mask))


def numpy_route():
    S = importlib.import_module("test_subset_masked_cpu")
    U = importlib.import_module("test_subset_uncertainty_cpu")
    P = importlib.import_module("test_node_strain_cpu")
    Q = importlib.import_module("test_node_strain_robust_cpu")
    Wt = importlib.import_module("test_node_strain_weighted_cpu")

    def chain(f0, f1, u0, v0, mask):
        got = S.subset_refine_masked_reference(f0, f1, u0, v0, None, mask, S.default_min_pixels(R), GRID_R, SPACING, R, max_shift=4.0)
        sig = U.subset_uncertainty_reference(f0, f1, [getattr(got, n) for n in NODE_NAMES], got.state, GRID_R, SPACING, R, mask=mask)
        u, v, st, su, sv = got.u, got.v, got.state, sig.sigma_u, sig.sigma_v
        fits = [P.node_strain_reference(u, v, st, None, SPACING, M, ORDER), Q.node_strain_robust_reference(u, v, st, SPACING, M, ORDER),
                Wt.node_strain_weighted_reference(u, v, su, sv, st, SPACING, M, ORDER, floor=FLOOR),
                Wt.node_strain_weighted_reference(u, v, su, sv, st, SPACING, M, ORDER, floor=FLOOR, threshold=3.0, iterations=4)]
        return [(f["exx"], f.get("sigma_exx"), int(f["stats"]["reserved"][0][4])) for f in fits]

    return chain, lambda: None


def device_route():
    flow2d = importlib.import_module("cuda-flow2d_amd")
    ctx = flow2d.Context(0)

    def chain(f0, f1, u0, v0, mask):
        nh, nw = u0.shape
        held = []

        def plane(w, h, a=None):
            held.append(ctx.plane(w, h, a))
            return held[-1]

        try:
            p0, p1, pu, pv = plane(W, H, f0), plane(W, H, f1), plane(nw, nh, u0), plane(nw, nh, v0)
            pm = plane(W, H, mask) if mask is not None else None
            outs = [plane(nw, nh) for _ in range(8)]
            keys = dict(out_u=outs[0], out_v=outs[1], out_gradients=outs[2:6], out_score=outs[6], out_state=outs[7], record=None, max_shift=4.0)
            if mask is None:
                ctx.subset_refine(p0, p1, W, H, pu, pv, nw, nh, GRID_R, SPACING, R, **keys)
            else:
                ctx.subset_refine_masked(p0, p1, W, H, pu, pv, None, nw, nh, GRID_R, SPACING, R, pm, **keys)
            sig = [plane(nw, nh) for _ in range(2)] + [None] * 6
            ctx.subset_uncertainty(p0, p1, W, H, outs[:6], outs[7], nw, nh, GRID_R, SPACING, R, mask=pm, out=sig, record=None)
            u, v, st = outs[0], outs[1], outs[7]
            want = ("exx",)
            fits = [ctx.node_strain(u, v, nw, nh, SPACING, M, ORDER, state=st, planes=want),
                    ctx.node_strain_robust(u, v, nw, nh, SPACING, M, ORDER, state=st, planes=want, diagnostics=()),
                    ctx.node_strain_weighted(u, v, sig[0], sig[1], nw, nh, SPACING, M, ORDER, sigma_floor=FLOOR, state=st, planes=want,
                                             sigmas=("sigma_exx",)),
                    ctx.node_strain_weighted(u, v, sig[0], sig[1], nw, nh, SPACING, M, ORDER, sigma_floor=FLOOR, threshold=3.0, iterations=4,
                                             state=st, planes=want, sigmas=("sigma_exx",))]
            return [(got["exx"], got.get("sigma_exx"), int(stats.reserved[4])) for got, stats in fits]
        finally:
            for q in held:
                q.free()
                ctx._planes.remove(q)

    return chain, ctx.close


def rows_of(chain):
    U = importlib.import_module("test_subset_uncertainty_cpu")
    lines = []
    for name, scene, mask in scenes():
        u0, v0 = U.truth_at_nodes(scene, GRID_R, SPACING)
        rng = np.random.default_rng(SEED)
        exx = [[] for _ in FITS]
        predicted = [[] for _ in FITS]
        rejected = [0 for _ in FITS]
        for _ in range(DRAWS):
            f0 = (scene.frame_0.astype(F64) + rng.normal(0.0, NOISE, scene.frame_0.shape)).astype(F32)
            f1 = (scene.frame_1.astype(F64) + rng.normal(0.0, NOISE, scene.frame_1.shape)).astype(F32)
            for k, (e, s, r) in enumerate(chain(f0, f1, u0, v0, mask)):
                exx[k].append(e.astype(F64))
                predicted[k].append(None if s is None else s.astype(F64))
                rejected[k] += r
        for k, fit in enumerate(FITS):
            e = np.stack(exx[k])
            every = np.isfinite(e).all(axis=0)
            error = float(np.sqrt(np.mean((e[:, every] - TRUE_EXX) ** 2)))
            scatter = float(np.sqrt(np.mean(np.var(e[:, every], axis=0, ddof=1))))
            if predicted[k][0] is None:
                tail = "| | |"
            else:
                p = float(np.sqrt(np.mean(np.stack(predicted[k])[:, every] ** 2)))
                tail = "| %.6f | %.3f |" % (p, p / scatter)
            lines.append("| %s | %s | %d | %.6f | %.6f %s %d |\n" % (name, fit, int(every.sum()), error, scatter, tail, rejected[k]))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_strain"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    committed = os.path.join(ROOT, "profiles", "weighted_strain", "table_numpy.md")  # the restatements' rows, kept in the repository
    chain, close = numpy_route() if args.numpy else device_route()
    try:
        got = rows_of(chain)
    finally:
        close()
    path = committed if args.numpy else os.path.join(args.out, "table.md")
    with open(path, "w") as f:
        f.write(HEADER)
        f.writelines(got)
    sys.stdout.write(HEADER + "".join(got))
    if args.numpy:
        return 0
    want = open(committed).readlines()[2:]
    differing = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
    print("%d device rows -> %s; %s" % (len(got), path, "equal to the committed restatement rows" if got == want
                                        else "rows %s DIFFER from %s" % (differing, committed)))
    return 0 if got == want else 1


if __name__ == "__main__":
    sys.exit(main())
