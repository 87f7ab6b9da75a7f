#!/usr/bin/env python3
"""Device-event timings of the cubic B-spline path of the subset refinement at 4096 x 4096 on the GPU, beside what it stands next to.
  The prefilter (flow2d_bspline_prefilter_2d) beside flow2d_gaussian_blur (sigma 1.5, radius 5: the existing separable filter of a
  similar shape) on the same plane, the two alternating; each figure is the time of BURST launches between two events, divided.
  The spline entries (flow2d_subset_refine_spline_2d without a mask, flow2d_subset_refine2_spline_2d) beside the Catmull-Rom entries
  of the same library (flow2d_subset_refine_from_2d, flow2d_subset_refine2_2d) on the same frames and the same starts -- the
  validated node field of flow2d_correlate_2d, range 8, on the grid (radius 7, spacing 8), 511 x 511 nodes -- at R = 7 and R = 15,
  the calls alternating after one warm-up call each; medians of --repeats.  The samplers need different numbers of iterations, so
  they are compared per node and iteration begun.  The frames are those of tools/time_subset.py.  No time is asserted.
Writes OUT/timings.json and prints one line per case.

  python tools/time_subset_spline.py [--size 4096] [--repeats 5] [--out profiles/subset_spline]
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
BURST = 20        # launches between the two events of a filter's figure
KINDS = ("catmull_rom", "bspline")


def summary(times):
    return {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset_spline"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    first_order = importlib.import_module("time_subset")
    n = args.size
    f0, f1 = first_order.frames(n)
    r, d, s = GRID
    with flow2d.Context(0) as ctx:
        p0, p1, coeff, blurred = ctx.plane(n, n, f0), ctx.plane(n, n, f1), ctx.plane(n, n), ctx.plane(n, n)
        nw, nh = flow2d.correlation_grid(n, n, r, s)
        raw, start = ([ctx.plane(nw, nh) for _ in range(k)] for k in (3, 2))
        out = [ctx.plane(nw, nh) for _ in range(14)]
        zeros = [ctx.plane(nw, nh, np.zeros((nh, nw), np.float32)) for _ in range(4)]
        record, checks, counts = ctx.correlation_records(), ctx.pass_records(), ctx.subset_records()
        begin, end = ctx.event(), ctx.event()
        ctx.correlate(p0, p1, n, n, 0.0, 1.0, r, d, s, -1.0, raw[0], raw[1], raw[2], record)
        ctx.validate_nodes(raw[0], raw[1], nw, nh, 2.0, 0.1, 3, flow2d.VALIDATE_REPLACE, start[0], start[1], None, checks)
        results = {"size": n, "device": ctx.device_name(), "grid": {"radius": r, "range": d, "spacing": s, "nw": nw, "nh": nh},
                   "shift": first_order.SHIFT, "repeats": args.repeats, "burst": BURST, "cases": {}}
        # ---- the two filters
        taps, radius = flow2d.gaussian_kernel(1.5)
        filters = {"prefilter": lambda: ctx.bspline_prefilter(p1, n, n, out=coeff), "gaussian_blur": lambda: ctx.gaussian_blur(blurred, p1, n, n, taps, radius)}
        times = {k: [] for k in filters}
        for i in range(1 + args.repeats):
            for kind, call in filters.items():
                ctx.record(begin)
                for _ in range(BURST):
                    call()
                ctx.record(end)
                ms = ctx.elapsed_ms(begin, end) / BURST
                if i >= 1:
                    times[kind].append(ms)
        for kind in filters:
            entry = summary(times[kind])
            entry["gb_per_s"] = 2.0 * 4.0 * n * n / (entry["median_ms"] * 1e6)  # one plane read, one written
            results["cases"][kind] = entry
            print("%-13s: median %8.2f us per launch (min %.2f, max %.2f; %d bursts of %d), %.0f GB/s of plane traffic" % (
                kind, 1e3 * entry["median_ms"], 1e3 * entry["min_ms"], 1e3 * entry["max_ms"], args.repeats, BURST, entry["gb_per_s"]))
        results["cases"]["gaussian_blur"]["radius"] = radius
        results["cases"]["prefilter_over_gaussian_blur"] = results["cases"]["prefilter"]["median_ms"] / results["cases"]["gaussian_blur"]["median_ms"]
        print("    the prefilter takes %.2f x the blur's time" % results["cases"]["prefilter_over_gaussian_blur"])
        # ---- the refinements (coeff holds frame 1's coefficients)
        for order in (1, 2):
            for R in (7, 15):
                def call(kind):
                    sampled = coeff if kind == "bspline" else p1
                    if order == 1:
                        common = dict(out_u=out[0], out_v=out[1], out_gradients=out[2:6], out_score=out[6], out_state=out[7], record=counts)
                        if kind == "bspline":
                            ctx.subset_refine_spline(p0, sampled, n, n, start[0], start[1], zeros, nw, nh, r, s, R, None, None, max_shift=2.0, **common)
                        else:
                            ctx.subset_refine_from(p0, sampled, n, n, start[0], start[1], zeros, nw, nh, r, s, R, max_shift=2.0, **common)
                    else:
                        entry = ctx.subset_refine2_spline if kind == "bspline" else ctx.subset_refine2
                        entry(p0, sampled, n, n, start[0], start[1], nw, nh, r, s, R, out_u=out[0], out_v=out[1], out_gradients=out[2:6],
                              out_curvatures=out[6:12], out_score=out[12], out_state=out[13], record=counts)

                times, records = {k: [] for k in KINDS}, {}
                for i in range(1 + args.repeats):
                    for kind in KINDS:
                        ctx.record(begin)
                        call(kind)
                        ctx.record(end)
                        ms = ctx.elapsed_ms(begin, end)
                        if i >= 1:
                            times[kind].append(ms)
                        if i == args.repeats:
                            rec = ctx.read_subset_record(counts)[0]
                            records[kind] = rec.summary()
                            u, v, state = out[0].download(nw, nh), out[1].download(nw, nh), out[13 if order == 2 else 7].download(nw, nh)
                            good = state >= 1
                            records[kind]["converged_mean_error_px"] = (float(np.hypot(u[good] - first_order.SHIFT[0], v[good] - first_order.SHIFT[1]).mean())
                                                                        if good.any() else None)
                for kind in KINDS:
                    rec = records[kind]
                    entry = dict(summary(times[kind]), record=rec,
                                 ns_per_node_iteration=1e6 * float(np.median(times[kind])) / max(rec["iterations"], 1))
                    results["cases"]["%s_order%d_R%d" % (kind, order, R)] = entry
                    print("%-11s order %d R = %2d: median %9.3f ms (min %.3f, max %.3f, %d calls), %d iterations begun, %.1f ns per node and "
                          "iteration; converged %d of %d, their mean error %s px" % (
                              kind, order, R, entry["median_ms"], entry["min_ms"], entry["max_ms"], args.repeats, rec["iterations"],
                              entry["ns_per_node_iteration"], rec["converged"], rec["nodes"], rec["converged_mean_error_px"]))
                a, b = (results["cases"]["%s_order%d_R%d" % (k, order, R)] for k in KINDS)
                ratio = {"per_node_iteration": b["ns_per_node_iteration"] / a["ns_per_node_iteration"], "whole_launch": b["median_ms"] / a["median_ms"]}
                results["cases"]["bspline_over_catmull_rom_order%d_R%d" % (order, R)] = ratio
                print("    order %d R = %d: the spline entry takes %.3f x the Catmull-Rom entry's time per node and iteration, %.3f x per launch" % (
                    order, R, ratio["per_node_iteration"], ratio["whole_launch"]))
                if order == 1 and R == 7:
                    share = results["cases"]["prefilter"]["median_ms"] / b["median_ms"]
                    results["cases"]["prefilter_share_of_the_R7_refinement"] = share
                    print("    the prefilter is %.2f %% of the R = 7 spline refinement" % (100.0 * share))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
