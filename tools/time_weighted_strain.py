#!/usr/bin/env python3
"""Device-event timings of flow2d_node_strain_weighted_2d on the GPU beside flow2d_node_strain_robust_2d at the same K, and at
T = 0 (no robust part: the Gauss-Markov fit alone) beside flow2d_node_strain_2d, on the two node grids of a 4096 x 4096 frame:
(radius 7, spacing 8) -- 511 x 511 nodes -- and the dense grid (radius 7, spacing 1) -- 4082 x 4082 nodes --; m = 2 and m = 7 at
both orders, K = 8 reweighted passes (T = 3 sigmas for the weighted entry, sigma = 0.05 px for the robust one), each with its
planes (nine, the three diagnostic ones, and the nine sigma planes for the weighted entry) and the record; the four entries in
turn on the same grid in the same run, medians of the timed rounds after a warm-up.  The node field is tools/time_node_strain.py's
(affine plus noise, 5 % of the nodes lost) with one node in a thousand moved by 2.5 px; the sigma planes are log-uniform over
0.005 .. 0.05 px, independent per node, the floor 0.005 px.  The weighted entry fits u and v with matrices of their own, so
2 (K + 1) + 1 walks of every window against the robust entry's K + 2 are to be expected.  No time is asserted and there is no
target.  Writes OUT/timings.json and prints one line per case.

  python tools/time_weighted_strain.py [--size 4096] [--rounds 5] [--out profiles/weighted_strain]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
WARMUP = 1
RADIUS = 7
SIGMA, THRESHOLD, FLOOR, PASSES = 0.05, 3.0, 0.005, 8
FORMS = (("m2_order1", 2, 1), ("m2_order2", 2, 2), ("m7_order1", 7, 1), ("m7_order2", 7, 2))
# (case, the case it is compared with)
PAIRS = (("weighted_k8", "robust_k8"), ("weighted_k0", "plain"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_strain"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    field = importlib.import_module("time_node_strain").field
    n = args.size
    results = {"size": n, "rounds": args.rounds, "sigma": SIGMA, "threshold": THRESHOLD, "sigma_floor": FLOOR, "iterations": PASSES,
               "grids": {}}
    with flow2d.Context(0) as ctx:
        results["device"] = ctx.device_name()
        for spacing in (8, 1):
            nw, nh = flow2d.correlation_grid(n, n, RADIUS, spacing)
            u, v, state, _ = field(nw, nh)
            rng = np.random.default_rng(1)
            u[rng.random((nh, nw)) < 0.001] += np.float32(2.5)
            su, sv = ((0.005 * 10.0 ** rng.random((nh, nw))).astype(np.float32) for _ in range(2))
            pu, pv, ps, psu, psv = (ctx.plane(nw, nh, a) for a in (u, v, state, su, sv))
            outs = {name: ctx.plane(nw, nh) for name in flow2d.DEFORMATION_PLANES}
            diag = {name: ctx.plane(nw, nh) for name in flow2d.NODE_STRAIN_DIAGNOSTICS}
            sig = {name: ctx.plane(nw, nh) for name in flow2d.STRAIN_SIGMA_PLANES}
            record, begin, end = ctx.deformation_records(), ctx.event(), ctx.event()

            def plain(m, order):
                ctx.node_strain(pu, pv, nw, nh, spacing, m, order, state=ps, planes=outs, stats=record)

            def robust(m, order):
                ctx.node_strain_robust(pu, pv, nw, nh, spacing, m, order, sigma=SIGMA, iterations=PASSES, state=ps, planes=outs,
                                       diagnostics=diag, stats=record)

            def weighted(m, order, threshold, passes):
                ctx.node_strain_weighted(pu, pv, psu, psv, nw, nh, spacing, m, order, sigma_floor=FLOOR, threshold=threshold,
                                         iterations=passes, state=ps, planes=outs, diagnostics=diag, sigmas=sig, stats=record)

            cases = []
            for name, m, order in FORMS:
                cases.append((name + "_plain", (lambda m=m, order=order: plain(m, order))))
                cases.append((name + "_weighted_k0", (lambda m=m, order=order: weighted(m, order, 0.0, 0))))
                cases.append((name + "_robust_k8", (lambda m=m, order=order: robust(m, order))))
                cases.append((name + "_weighted_k8", (lambda m=m, order=order: weighted(m, order, THRESHOLD, PASSES))))
            times = {name: [] for name, _ in cases}
            counts = {}
            for i in range(WARMUP + args.rounds):
                for name, call in cases:  # in turn, so that a drift of the clocks meets all alike
                    ctx.record(begin)
                    call()
                    ctx.record(end)
                    ms = ctx.elapsed_ms(begin, end)
                    if i >= WARMUP:
                        times[name].append(ms)
                    if i == 0:
                        rec = ctx.read_deformation_stats(record)[0]
                        counts[name] = dict(valid=int(rec.valid), **flow2d.node_strain_weighted_counts(rec))
            grid = {"spacing": spacing, "nw": nw, "nh": nh, "cases": {}}
            for name, _ in cases:
                t = times[name]
                grid["cases"][name] = dict(counts[name], median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)),
                                           ns_per_node=1e6 * float(np.median(t)) / (nw * nh))
                print("%4d x %-4d %-22s median %10.4f ms  (min %.4f, max %.4f, %d rounds)  %.3f ns per node, %s" % (
                    nw, nh, name, np.median(t), np.min(t), np.max(t), args.rounds, grid["cases"][name]["ns_per_node"], counts[name]))
            for name, _, _ in FORMS:
                for case, other in PAIRS:
                    ratio = grid["cases"]["%s_%s" % (name, case)]["median_ms"] / grid["cases"]["%s_%s" % (name, other)]["median_ms"]
                    grid["cases"]["%s_%s" % (name, case)]["times_" + other] = ratio
                    print("%4d x %-4d %-22s %s / %s %.2f" % (nw, nh, name, case, other, ratio))
            results["grids"]["spacing_%d" % spacing] = grid
            for q in [pu, pv, ps, psu, psv, record] + list(outs.values()) + list(diag.values()) + list(sig.values()):
                q.free()
                ctx._planes.remove(q)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
