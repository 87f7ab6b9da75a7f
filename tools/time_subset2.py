#!/usr/bin/env python3
"""Device-event timings of flow2d_subset_refine2_2d beside flow2d_subset_refine_2d at 4096 x 4096 on the GPU: the grid (radius 7,
spacing 8) -- 511 x 511 nodes -- refined with subsets of R = 7 and of R = 15, both orders on the same frames and the same starts
(the validated node field of flow2d_correlate_2d, range 8) in the same run, their calls alternating -- order 1, order 2, order 1,
... -- after one warm-up call each; medians.  The frames are those of tools/time_subset.py: band-limited noise moved by (3.3,
-1.6).  A refinement's time is proportional to the iterations its record counts, so "ns per node and iteration" -- the time over
the iterations begun -- is printed as well.  No time is asserted.  Writes OUT/timings.json and prints one line per case.

  python tools/time_subset2.py [--size 4096] [--repeats 5] [--out profiles/subset2]
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
GRID = (7, 8, 8)  # radius, range, spacing


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset2"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    first_order = importlib.import_module("time_subset")
    n = args.size
    f0, f1 = first_order.frames(n)
    r, d, s = GRID
    with flow2d.Context(0) as ctx:
        p0, p1 = ctx.plane(n, n, f0), ctx.plane(n, n, f1)
        nw, nh = flow2d.correlation_grid(n, n, r, s)
        raw, start, out = ([ctx.plane(nw, nh) for _ in range(k)] for k in (3, 2, 14))
        record, checks, counts = ctx.correlation_records(), ctx.pass_records(), ctx.subset_records()
        begin, end = ctx.event(), ctx.event()
        ctx.correlate(p0, p1, n, n, 0.0, 1.0, r, d, s, -1.0, raw[0], raw[1], raw[2], record)
        ctx.validate_nodes(raw[0], raw[1], nw, nh, 2.0, 0.1, 3, flow2d.VALIDATE_REPLACE, start[0], start[1], None, checks)
        results = {"size": n, "device": ctx.device_name(), "grid": {"radius": r, "range": d, "spacing": s, "nw": nw, "nh": nh},
                   "shift": first_order.SHIFT, "repeats": args.repeats, "cases": {}}
        for R in (7, 15):
            calls = {
                1: lambda: ctx.subset_refine(p0, p1, n, n, start[0], start[1], nw, nh, r, s, R, out_u=out[0], out_v=out[1],
                                             out_gradients=out[2:6], out_score=out[12], out_state=out[13], record=counts),
                2: lambda: ctx.subset_refine2(p0, p1, n, n, start[0], start[1], nw, nh, r, s, R, out_u=out[0], out_v=out[1],
                                              out_gradients=out[2:6], out_curvatures=out[6:12], out_score=out[12], out_state=out[13],
                                              record=counts)}
            times, records, errors = {1: [], 2: []}, {}, {}
            for i in range(1 + args.repeats):
                for order in (1, 2):
                    ctx.record(begin)
                    calls[order]()
                    ctx.record(end)
                    ms = ctx.elapsed_ms(begin, end)
                    if i >= 1:
                        times[order].append(ms)
                    if i == args.repeats:
                        records[order] = ctx.read_subset_record(counts)[0].summary()
                        state, u, v = out[13].download(nw, nh), out[0].download(nw, nh), out[1].download(nw, nh)
                        good = state >= 1
                        errors[order] = float(np.hypot(u[good] - first_order.SHIFT[0], v[good] - first_order.SHIFT[1]).mean()) if good.any() else None
            for order in (1, 2):
                rec = records[order]
                entry = {"median_ms": float(np.median(times[order])), "min_ms": float(np.min(times[order])), "max_ms": float(np.max(times[order])),
                         "record": rec, "ns_per_node_iteration": 1e6 * float(np.median(times[order])) / max(rec["iterations"], 1),
                         "converged_mean_error_px": errors[order]}
                results["cases"]["order%d_R%d" % (order, R)] = entry
                print("order %d, R = %2d: median %9.3f ms (min %.3f, max %.3f, %d calls), %d iterations begun, %.1f ns per node and iteration; "
                      "converged %d of %d, their mean error %s px" % (order, R, entry["median_ms"], entry["min_ms"], entry["max_ms"], args.repeats,
                                                                      rec["iterations"], entry["ns_per_node_iteration"], rec["converged"],
                                                                      rec["nodes"], entry["converged_mean_error_px"]))
            results["cases"]["order2_over_order1_R%d" % R] = (results["cases"]["order2_R%d" % R]["median_ms"] /
                                                              results["cases"]["order1_R%d" % R]["median_ms"])
            print("    R = %d: order 2 takes %.2f x order 1's time" % (R, results["cases"]["order2_over_order1_R%d" % R]))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
