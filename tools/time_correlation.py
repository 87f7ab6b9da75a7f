#!/usr/bin/env python3
"""Device-event timings of flow2d_correlate_2d and flow2d_expand_nodes_2d at 4096 x 4096 on the GPU: a PIV-style grid (radius 7,
range 8, spacing 8), the dense setting (radius 7, range 8, spacing 1) and the expansion of the PIV grid's nodes to the frame.
The frames are uniform noise in u8's range, frame 1 = frame 0 moved by (3, -2) plus noise -- the time does not depend on the
content: every candidate is scored in full.  Median of the timed calls after a warm-up, one call between two events.

The correlation kernel is bound by the vector units and LDS, so beside each time stands the kernel's own count of work: per
candidate (a displacement whose window lies inside frame 1, counted exactly here) N = (2r + 1)^2 pixels, each a byte
multiply-add into S1, S11 and S01 -- 3 N byte multiply-adds, issued four to a v_dot4_u32_u8 -- plus the four neighbours of every
peak scored once more.  The expansion is bound by bytes: two planes written, the node planes read (they stay in cache).
No time is asserted anywhere.  Writes OUT/timings.json and prints one line per case.

  python tools/time_correlation.py [--size 4096] [--out profiles/correlation]
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
CASES = (("piv_r7_d8_s8", 7, 8, 8, 10), ("dense_r7_d8_s1", 7, 8, 1, 3))  # name, radius, range, spacing, timed calls


def candidates(size, r, d, s):
    """The number of (node, displacement) pairs whose displaced window lies inside the frame (the same along both axes)."""
    left = np.arange((size - 2 * r - 1) // s + 1) * s
    per_node = sum(((left + k >= 0) & (left + k + 2 * r + 1 <= size)).astype(np.int64) for k in range(-d, d + 1))
    return int(per_node.sum()) ** 2, len(left)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correlation"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    n = args.size
    rng = np.random.default_rng(0)
    big = rng.uniform(0, 255, (n + 8, n + 8)).astype(np.float32)
    f0 = big[4:4 + n, 4:4 + n]
    f1 = (big[6:6 + n, 1:1 + n] + rng.normal(0, 6, (n, n))).astype(np.float32)
    with flow2d.Context(0) as ctx:
        p0, p1 = ctx.plane(n, n, f0), ctx.plane(n, n, f1)
        nodes = [ctx.plane(n, n) for _ in range(3)]
        dense = [ctx.plane(n, n) for _ in range(2)]
        record = ctx.correlation_records()
        start, stop = ctx.event(), ctx.event()
        results = {"size": n, "device": ctx.device_name(), "cases": {}}

        def timed(call, repeats):
            times = []
            for i in range(WARMUP + repeats):
                ctx.record(start)
                call()
                ctx.record(stop)
                ms = ctx.elapsed_ms(start, stop)
                if i >= WARMUP:
                    times.append(ms)
            return float(np.median(times)), float(np.min(times)), float(np.max(times))

        for name, r, d, s, repeats in CASES:
            ms, lo, hi = timed(lambda: ctx.correlate(p0, p1, n, n, 0.0, 1.0, r, d, s, -1.0, nodes[0], nodes[1], nodes[2], record), repeats)
            rec = ctx.read_correlation_record(record)[0].summary()
            count, per_axis = candidates(n, r, d, s)
            macs = 3 * (2 * r + 1) ** 2 * (count + 4 * (rec["nodes"] - rec["invalid"]))
            results["cases"][name] = {"median_ms": ms, "min_ms": lo, "max_ms": hi, "repeats": repeats, "nodes_per_axis": per_axis,
                                      "candidates": count, "byte_multiply_adds": macs, "tera_byte_macs_per_s": macs / ms * 1e-9,
                                      "record": rec}
            print("%-16s median %9.3f ms  (min %.3f, max %.3f)  %d^2 nodes  %.3e byte multiply-adds  %.2f T/s  %s" %
                  (name, ms, lo, hi, per_axis, macs, macs / ms * 1e-9, json.dumps(rec)))
            if s == 8:  # the expansion of this grid: the node planes are what the call above left
                nw, nh = flow2d.correlation_grid(n, n, r, s)
                ems, elo, ehi = timed(lambda: ctx.expand_nodes(nodes[0], nodes[1], nw, nh, r, s, dense[0], dense[1], n, n), 10)
                moved = 2 * n * n * 4 + 2 * nw * nh * 4
                results["cases"]["expand_r7_s8"] = {"median_ms": ems, "min_ms": elo, "max_ms": ehi, "repeats": 10, "bytes": moved,
                                                    "gb_per_s": moved / ems * 1e-6}
                print("%-16s median %9.3f ms  (min %.3f, max %.3f)  %.1f MB written and read  %.0f GB/s" %
                      ("expand_r7_s8", ems, elo, ehi, moved * 1e-6, moved / ems * 1e-6))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
