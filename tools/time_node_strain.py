#!/usr/bin/env python3
"""Device-event timings of flow2d_node_strain_2d on the GPU, on the two node grids of a 4096 x 4096 frame: (radius 7, spacing 8) --
511 x 511 nodes -- and the dense grid (radius 7, spacing 1) -- 4082 x 4082 nodes --; the direct form (window 0) and the window
fit with m = 2 and m = 7 at both orders, each with all nine planes and the record, and flow2d_deformation_2d (nine planes, the
record) on a plane with the same number of points beside them, in the same run, in turn; medians of the timed rounds after a
warm-up.  The node field is an affine displacement plus noise with 5 % of the nodes lost (state 0), so that the windows have holes.
No time is asserted and there is no target.  Writes OUT/timings.json and prints one line per case.

  python tools/time_node_strain.py [--size 4096] [--rounds 7] [--out profiles/node_strain]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP = 1
RADIUS = 7
FORMS = (("direct", 0, 1), ("m2_order1", 2, 1), ("m2_order2", 2, 2), ("m7_order1", 7, 1), ("m7_order2", 7, 2))


def field(nw, nh, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:nh, 0:nw].astype(np.float32)
    u = (0.01 * x - 0.004 * y + 0.02 * rng.standard_normal((nh, nw))).astype(np.float32)
    v = (0.003 * x + 0.008 * y + 0.02 * rng.standard_normal((nh, nw))).astype(np.float32)
    state = np.where(rng.random((nh, nw)) < 0.05, 0, 3).astype(np.float32)
    grads = [(0.01 * rng.standard_normal((nh, nw))).astype(np.float32) for _ in range(4)]
    return u, v, state, grads


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node_strain"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    n = args.size
    results = {"size": n, "rounds": args.rounds, "grids": {}}
    with flow2d.Context(0) as ctx:
        results["device"] = ctx.device_name()
        for spacing in (8, 1):
            nw, nh = flow2d.correlation_grid(n, n, RADIUS, spacing)
            u, v, state, grads = field(nw, nh)
            pu, pv, ps = ctx.plane(nw, nh, u), ctx.plane(nw, nh, v), ctx.plane(nw, nh, state)
            pg = [ctx.plane(nw, nh, g) for g in grads]
            outs = {name: ctx.plane(nw, nh) for name in flow2d.DEFORMATION_PLANES}
            record, begin, end = ctx.deformation_records(), ctx.event(), ctx.event()

            def strain(m, order):
                ctx.node_strain(pu, pv, nw, nh, spacing, m, order, state=ps, gradients=pg, planes=outs, stats=record)

            cases = [(name, (lambda m=m, order=order: strain(m, order))) for name, m, order in FORMS]
            cases.append(("deformation_2d", lambda: ctx.deformation(pu, pv, nw, nh, planes=outs, stats=record)))
            times = {name: [] for name, _ in cases}
            valid = {}
            for i in range(WARMUP + args.rounds):
                for name, call in cases:  # in turn, so that a drift of the clocks meets all alike
                    ctx.record(begin)
                    call()
                    ctx.record(end)
                    ms = ctx.elapsed_ms(begin, end)
                    if i >= WARMUP:
                        times[name].append(ms)
                    if i == 0:
                        valid[name] = int(ctx.read_deformation_stats(record)[0].valid)
            grid = {"spacing": spacing, "nw": nw, "nh": nh, "cases": {}}
            for name, _ in cases:
                t = times[name]
                grid["cases"][name] = {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t)),
                                       "valid": valid[name], "ns_per_node": 1e6 * float(np.median(t)) / (nw * nh)}
                print("%4d x %-4d %-14s median %9.4f ms  (min %.4f, max %.4f, %d rounds)  %.3f ns per node, %d valid" % (
                    nw, nh, name, np.median(t), np.min(t), np.max(t), args.rounds, grid["cases"][name]["ns_per_node"], valid[name]))
            results["grids"]["spacing_%d" % spacing] = grid
            for q in [pu, pv, ps, record] + pg + list(outs.values()):
                q.free()
                ctx._planes.remove(q)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
