#!/usr/bin/env python3
"""Device-event timings of flow2d_subset_uncertainty_2d beside the refinement that produced its input, at 4096 x 4096 on the GPU:
the grid (radius 7, spacing 8) -- 511 x 511 nodes -- with subsets of R = 7 and of R = 15, both samplers (the Catmull-Rom sample of
frame 1, the cubic B-spline sample of its coefficients), and an all-zero mask against none.  Per case the refinement (from the
validated node field of flow2d_correlate_2d, range 8) and the uncertainty of its result alternate in the same process -- refine,
evaluate, refine, ... -- after one warm-up call each; medians of five.  The frames are those of tools/time_subset.py.  The bytes
of the all-zero mask's run are checked against those without a mask.  No time is asserted.  Writes OUT/timings.json and prints one
line per case.

  python tools/time_subset_uncertainty.py [--size 4096] [--repeats 5] [--out profiles/subset_uncertainty]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset_uncertainty"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    first_order = importlib.import_module("time_subset")
    n = args.size
    f0, f1 = first_order.frames(n)
    r, d, s = GRID
    with flow2d.Context(0) as ctx:
        p0, p1 = ctx.plane(n, n, f0), ctx.plane(n, n, f1)
        coeff = ctx.bspline_prefilter(p1, n, n)
        zero = ctx.plane(n, n, np.zeros((n, n), np.float32))
        nw, nh = flow2d.correlation_grid(n, n, r, s)
        raw, start, field, out = ([ctx.plane(nw, nh) for _ in range(k)] for k in (3, 2, 8, 8))
        record, checks, counts, evaluated = ctx.correlation_records(), ctx.pass_records(), ctx.subset_records(), ctx.uncertainty_records()
        begin, end = ctx.event(), ctx.event()
        ctx.correlate(p0, p1, n, n, 0.0, 1.0, r, d, s, -1.0, raw[0], raw[1], raw[2], record)
        ctx.validate_nodes(raw[0], raw[1], nw, nh, 2.0, 0.1, 3, flow2d.VALIDATE_REPLACE, start[0], start[1], None, checks)
        results = {"size": n, "device": ctx.device_name(), "grid": {"radius": r, "range": d, "spacing": s, "nw": nw, "nh": nh},
                   "shift": first_order.SHIFT, "repeats": args.repeats, "cases": {}}
        into = dict(out_u=field[0], out_v=field[1], out_gradients=field[2:6], out_score=field[6], out_state=field[7], record=counts)
        for R in (7, 15):
            planes = {}
            for sampler in ("catmull-rom", "bspline"):
                for masked in (False, True):
                    second, interpolation = (coeff, 1) if sampler == "bspline" else (p1, 0)
                    mask = zero if masked else None

                    def refine():
                        if sampler == "bspline":
                            ctx.subset_refine_spline(p0, coeff, n, n, start[0], start[1], None, nw, nh, r, s, R, mask, None, max_shift=2.0, **into)
                        elif masked:
                            ctx.subset_refine_masked(p0, p1, n, n, start[0], start[1], None, nw, nh, r, s, R, mask, None, max_shift=2.0, **into)
                        else:
                            ctx.subset_refine(p0, p1, n, n, start[0], start[1], nw, nh, r, s, R, **into)

                    def evaluate():
                        ctx.subset_uncertainty(p0, second, n, n, field[:6], field[7], nw, nh, r, s, R, 1, interpolation, mask, None, out, evaluated)

                    times = {"refine": [], "uncertainty": []}
                    for i in range(1 + args.repeats):
                        for kind, call in (("refine", refine), ("uncertainty", evaluate)):
                            ctx.record(begin)
                            call()
                            ctx.record(end)
                            ms = ctx.elapsed_ms(begin, end)
                            if i >= 1:
                                times[kind].append(ms)
                    refined, rec = ctx.read_subset_record(counts)[0], ctx.read_uncertainty_record(evaluated)[0]
                    name = "R%d_%s_%s" % (R, sampler, "zero_mask" if masked else "no_mask")
                    planes[sampler, masked] = [q.download(nw, nh).tobytes() for q in out]
                    sigma_u = out[0].download(nw, nh)
                    entry = {kind: {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))} for kind, t in times.items()}
                    entry["uncertainty_over_refine"] = entry["uncertainty"]["median_ms"] / entry["refine"]["median_ms"]
                    entry["iterations_per_converged_node"] = refined.iterations / max(refined.converged, 1)
                    entry["refine_record"], entry["uncertainty_record"] = refined.summary(), rec.summary()
                    entry["ns_per_evaluated_node"] = 1e6 * entry["uncertainty"]["median_ms"] / max(rec.evaluated, 1)
                    entry["median_sigma_u_px"] = float(np.nanmedian(sigma_u))
                    results["cases"][name] = entry
                    print("%-28s refine %8.3f ms (min %.3f, max %.3f), uncertainty %8.3f ms (min %.3f, max %.3f): %.3f x; %d of %d evaluated, "
                          "%.2f iterations per converged node, %.1f ns per evaluated node, median sigma_u %.5f px"
                          % (name, entry["refine"]["median_ms"], entry["refine"]["min_ms"], entry["refine"]["max_ms"],
                             entry["uncertainty"]["median_ms"], entry["uncertainty"]["min_ms"], entry["uncertainty"]["max_ms"],
                             entry["uncertainty_over_refine"], rec.evaluated, rec.nodes, entry["iterations_per_converged_node"],
                             entry["ns_per_evaluated_node"], entry["median_sigma_u_px"]))
            for sampler in ("catmull-rom", "bspline"):
                same = planes[sampler, True] == planes[sampler, False]
                results["cases"]["R%d_%s_zero_mask_equals_no_mask" % (R, sampler)] = same
                print("    R = %d, %s: the all-zero mask's bytes %s those without a mask" % (R, sampler, "are" if same else "DIFFER from"))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
