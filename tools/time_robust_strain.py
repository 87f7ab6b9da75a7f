#!/usr/bin/env python3
"""Device-event timings of flow2d_node_strain_robust_2d on the GPU beside flow2d_node_strain_2d, on the two node grids of a
4096 x 4096 frame: (radius 7, spacing 8) -- 511 x 511 nodes -- and the dense grid (radius 7, spacing 1) -- 4082 x 4082 nodes --;
m = 2 and m = 7 at both orders, K = 8 reweighted passes at sigma = 0.05, each with its planes (nine, and the three diagnostic
ones for the robust entry) and the record; the plain and the robust entry in turn on the same grid in the same run, medians of
the timed rounds after a warm-up.  The node field is tools/time_node_strain.py's (affine plus noise, 5 % of the nodes lost) with
one node in a thousand moved by 2.5 px.  K + 2 walks of every window against one are to be expected.  No time is asserted and
there is no target.  Writes OUT/timings.json and prints one line per case.

  python tools/time_robust_strain.py [--size 4096] [--rounds 5] [--out profiles/robust_strain]
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
SIGMA, PASSES = 0.05, 8
FORMS = (("m2_order1", 2, 1), ("m2_order2", 2, 2), ("m7_order1", 7, 1), ("m7_order2", 7, 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust_strain"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    field = importlib.import_module("time_node_strain").field
    n = args.size
    results = {"size": n, "rounds": args.rounds, "sigma": SIGMA, "iterations": PASSES, "grids": {}}
    with flow2d.Context(0) as ctx:
        results["device"] = ctx.device_name()
        for spacing in (8, 1):
            nw, nh = flow2d.correlation_grid(n, n, RADIUS, spacing)
            u, v, state, _ = field(nw, nh)
            u[np.random.default_rng(1).random((nh, nw)) < 0.001] += np.float32(2.5)
            pu, pv, ps = ctx.plane(nw, nh, u), ctx.plane(nw, nh, v), ctx.plane(nw, nh, state)
            outs = {name: ctx.plane(nw, nh) for name in flow2d.DEFORMATION_PLANES}
            diag = {name: ctx.plane(nw, nh) for name in flow2d.NODE_STRAIN_DIAGNOSTICS}
            record, begin, end = ctx.deformation_records(), ctx.event(), ctx.event()

            def plain(m, order):
                ctx.node_strain(pu, pv, nw, nh, spacing, m, order, state=ps, planes=outs, stats=record)

            def robust(m, order):
                ctx.node_strain_robust(pu, pv, nw, nh, spacing, m, order, sigma=SIGMA, iterations=PASSES, state=ps, planes=outs,
                                       diagnostics=diag, stats=record)

            cases = []
            for name, m, order in FORMS:
                cases.append((name + "_plain", (lambda m=m, order=order: plain(m, order))))
                cases.append((name + "_robust", (lambda m=m, order=order: robust(m, order))))
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
                        counts[name] = dict(valid=int(rec.valid), **flow2d.node_strain_robust_counts(rec))
            grid = {"spacing": spacing, "nw": nw, "nh": nh, "cases": {}}
            for name, _ in cases:
                t = times[name]
                grid["cases"][name] = dict(counts[name], median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)),
                                           ns_per_node=1e6 * float(np.median(t)) / (nw * nh))
                print("%4d x %-4d %-18s median %10.4f ms  (min %.4f, max %.4f, %d rounds)  %.3f ns per node, %s" % (
                    nw, nh, name, np.median(t), np.min(t), np.max(t), args.rounds, grid["cases"][name]["ns_per_node"], counts[name]))
            for name, _, _ in FORMS:
                ratio = grid["cases"][name + "_robust"]["median_ms"] / grid["cases"][name + "_plain"]["median_ms"]
                grid["cases"][name + "_robust"]["times_the_plain_entry"] = ratio
                print("%4d x %-4d %-18s robust / plain %.2f  (K + 2 = %d walks against one)" % (nw, nh, name, ratio, PASSES + 2))
            results["grids"]["spacing_%d" % spacing] = grid
            for q in [pu, pv, ps, record] + list(outs.values()) + list(diag.values()):
                q.free()
                ctx._planes.remove(q)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
