#!/usr/bin/env python3
"""Device-event timings of flow2d_subset_refine_masked_2d beside flow2d_subset_refine_from_2d at 4096 x 4096 on the GPU: the grid
(radius 7, spacing 8) -- 511 x 511 nodes -- refined with subsets of R = 7 and of R = 15 on the same frames and the same starts (the
validated node field of flow2d_correlate_2d, range 8, with zero start gradients) in the same run, the calls alternating -- plain,
all-zero mask, half mask, plain, ... -- after one warm-up call each; medians.  "zero": a mask that excludes nothing, so the new
kernel does the plain one's work plus five mask loads per pixel and one compaction per node; "half": a mask that excludes the right
half of the frame, whose nodes end as masked before they read a pixel.  The frames are those of tools/time_subset.py.  The bytes
of the all-zero run are checked against the plain one's.  No time is asserted.  Writes OUT/timings.json and prints one line per case.

  python tools/time_subset_mask.py [--size 4096] [--repeats 5] [--out profiles/subset_mask]
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
KINDS = ("plain", "zero", "half")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset_mask"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    first_order = importlib.import_module("time_subset")
    n = args.size
    f0, f1 = first_order.frames(n)
    r, d, s = GRID
    half = np.zeros((n, n), np.float32)
    half[:, n // 2:] = 1
    with flow2d.Context(0) as ctx:
        p0, p1 = ctx.plane(n, n, f0), ctx.plane(n, n, f1)
        masks = {"zero": ctx.plane(n, n, np.zeros((n, n), np.float32)), "half": ctx.plane(n, n, half)}
        nw, nh = flow2d.correlation_grid(n, n, r, s)
        raw, start, out = ([ctx.plane(nw, nh) for _ in range(k)] for k in (3, 2, 8))
        zeros = [ctx.plane(nw, nh, np.zeros((nh, nw), np.float32)) for _ in range(4)]
        record, checks, counts = ctx.correlation_records(), ctx.pass_records(), ctx.subset_records()
        begin, end = ctx.event(), ctx.event()
        ctx.correlate(p0, p1, n, n, 0.0, 1.0, r, d, s, -1.0, raw[0], raw[1], raw[2], record)
        ctx.validate_nodes(raw[0], raw[1], nw, nh, 2.0, 0.1, 3, flow2d.VALIDATE_REPLACE, start[0], start[1], None, checks)
        results = {"size": n, "device": ctx.device_name(), "grid": {"radius": r, "range": d, "spacing": s, "nw": nw, "nh": nh},
                   "shift": first_order.SHIFT, "repeats": args.repeats, "cases": {}}
        for R in (7, 15):
            common = dict(out_u=out[0], out_v=out[1], out_gradients=out[2:6], out_score=out[6], out_state=out[7], record=counts)

            def call(kind):
                if kind == "plain":
                    ctx.subset_refine_from(p0, p1, n, n, start[0], start[1], zeros, nw, nh, r, s, R, max_shift=2.0, **common)
                else:
                    ctx.subset_refine_masked(p0, p1, n, n, start[0], start[1], zeros, nw, nh, r, s, R, masks[kind], None, max_shift=2.0, **common)

            times, records, planes = {k: [] for k in KINDS}, {}, {}
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
                        records[kind] = dict(rec.summary(), masked=rec.masked)
                        planes[kind] = [q.download(nw, nh).tobytes() for q in out]
            same = planes["zero"] == planes["plain"] and {k: v for k, v in records["zero"].items()} == records["plain"]
            results["cases"]["zero_equals_plain_R%d" % R] = same
            for kind in KINDS:
                rec = records[kind]
                entry = {"median_ms": float(np.median(times[kind])), "min_ms": float(np.min(times[kind])), "max_ms": float(np.max(times[kind])),
                         "record": rec, "ns_per_node_iteration": 1e6 * float(np.median(times[kind])) / max(rec["iterations"], 1)}
                results["cases"]["%s_R%d" % (kind, R)] = entry
                print("%-5s R = %2d: median %9.3f ms (min %.3f, max %.3f, %d calls), %d iterations begun, %.1f ns per node and iteration; "
                      "converged %d, masked %d of %d" % (kind, R, entry["median_ms"], entry["min_ms"], entry["max_ms"], args.repeats,
                                                        rec["iterations"], entry["ns_per_node_iteration"], rec["converged"], rec["masked"],
                                                        rec["nodes"]))
            for kind in ("zero", "half"):
                ratio = results["cases"]["%s_R%d" % (kind, R)]["median_ms"] / results["cases"]["plain_R%d" % R]["median_ms"]
                results["cases"]["%s_over_plain_R%d" % (kind, R)] = ratio
                print("    R = %d: the %s mask takes %.3f x the plain entry's time" % (R, kind, ratio))
            print("    R = %d: the all-zero mask's bytes and record %s the plain entry's" % (R, "are" if same else "DIFFER from"))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
