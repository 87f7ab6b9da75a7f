#!/usr/bin/env python3
"""Device-event timings of the masked window search and the masked median test on the GPU, medians of five timed calls per case
after a warm-up, the cases of one comparison alternating in one run (round by round, not case by case):
  (a) at 4096 x 4096 on the PIV grid (radius 7, range 8, spacing 8), no predictor: flow2d_correlate_offset_2d, against
      flow2d_correlate_masked_2d with an all-zero mask and with a mask that excludes the right half of the frame;
  (b) on 1022 x 1022 nodes (the grid (4, ., 4) of the same frame): flow2d_validate_nodes_2d against
      flow2d_validate_nodes_masked_2d with the all-zero mask and with the right half excluded.
The frames are uniform noise in u8's range, frame 1 = frame 0 moved by (3, -2) plus noise.  No time is asserted.  Writes
OUT/timings.json and prints one line per case.

  python tools/time_search_mask.py [--size 4096] [--out profiles/search_mask]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, ROUNDS = 2, 5


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_mask"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    n = args.size
    rng = np.random.default_rng(0)
    big = rng.uniform(0, 255, (n + 8, n + 8)).astype(np.float32)
    f0 = big[4:4 + n, 4:4 + n]
    f1 = (big[6:6 + n, 1:1 + n] + rng.normal(0, 6, (n, n))).astype(np.float32)
    half = np.zeros((n, n), np.float32)
    half[:, n // 2:] = 1
    with flow2d.Context(0) as ctx:
        p0, p1 = ctx.plane(n, n, f0), ctx.plane(n, n, f1)
        zero, right = ctx.plane(n, n, np.zeros((n, n), np.float32)), ctx.plane(n, n, half)
        raw, val = ([ctx.plane(n, n) for _ in range(2)] for _ in range(2))
        score = ctx.plane(n, n)
        passes, checks = ctx.pass_records(), ctx.pass_records()
        start, stop = ctx.event(), ctx.event()
        results = {"size": n, "device": ctx.device_name(), "warmup": WARMUP, "rounds": ROUNDS, "cases": {}}

        def alternate(cases):
            """cases: name -> (call, read the record).  Every round runs each case once; the medians are over the timed rounds."""
            times = {name: [] for name in cases}
            for i in range(WARMUP + ROUNDS):
                for name, (call, _) in cases.items():
                    ctx.record(start)
                    call()
                    ctx.record(stop)
                    ms = ctx.elapsed_ms(start, stop)
                    if i >= WARMUP:
                        times[name].append(ms)
            for name, (call, read) in cases.items():
                call()
                entry = {"median_ms": float(np.median(times[name])), "min_ms": float(np.min(times[name])), "max_ms": float(np.max(times[name])),
                         "record": read()}
                results["cases"][name] = entry
                print("%-34s median %9.3f ms  (min %.3f, max %.3f)  %s" % (name, entry["median_ms"], entry["min_ms"], entry["max_ms"],
                                                                          json.dumps(entry["record"])))
            return {name: results["cases"][name]["median_ms"] for name in cases}

        def pass_record():
            rec = ctx.read_correlation_pass_record(passes)[0]
            return dict(rec.summary(), masked=rec.masked)

        def check_record():
            rec = ctx.read_validation_record(checks)[0]
            return dict(rec.summary(), masked=rec.masked)

        # (a)
        r, d, s = 7, 8, 8
        side = (2 * r + 1) ** 2

        def search(mask):
            if mask is None:
                return lambda: ctx.correlate_offset(p0, p1, n, n, 0.0, 1.0, r, d, s, -1.0, None, raw[0], raw[1], score, passes)
            return lambda: ctx.correlate_masked(p0, p1, n, n, 0.0, 1.0, r, d, s, mask, side // 4 + 1, -1.0, None, raw[0], raw[1], score, passes)

        a = alternate({"a_offset_r7_d8_s8": (search(None), pass_record), "a_masked_all_zero_r7_d8_s8": (search(zero), pass_record),
                       "a_masked_right_half_r7_d8_s8": (search(right), pass_record)})
        results["a_all_zero_over_offset"] = a["a_masked_all_zero_r7_d8_s8"] / a["a_offset_r7_d8_s8"]
        results["a_right_half_over_offset"] = a["a_masked_right_half_r7_d8_s8"] / a["a_offset_r7_d8_s8"]
        print("(a) masked, all zero / unmasked = %.3f;  masked, right half / unmasked = %.3f" % (results["a_all_zero_over_offset"],
                                                                                               results["a_right_half_over_offset"]))

        # (b): the nodes of the grid (4, 4), searched once with a small range
        r, s = 4, 4
        nw, nh = flow2d.correlation_grid(n, n, r, s)
        ctx.correlate_offset(p0, p1, n, n, 0.0, 1.0, r, 4, s, -1.0, None, raw[0], raw[1], None, passes)

        def validate(mask):
            if mask is None:
                return lambda: ctx.validate_nodes(raw[0], raw[1], nw, nh, 2.0, 0.1, 3, flow2d.VALIDATE_REPLACE, val[0], val[1], None, checks)
            return lambda: ctx.validate_nodes_masked(raw[0], raw[1], nw, nh, mask, n, n, r, s, 2.0, 0.1, 3, flow2d.VALIDATE_REPLACE, val[0], val[1],
                                                     None, checks)

        name = "%dx%d" % (nw, nh)
        b = alternate({"b_validate_" + name: (validate(None), check_record), "b_validate_masked_all_zero_" + name: (validate(zero), check_record),
                       "b_validate_masked_right_half_" + name: (validate(right), check_record)})
        results["b_all_zero_over_validate"] = b["b_validate_masked_all_zero_" + name] / b["b_validate_" + name]
        print("(b) masked validation, all zero / unmasked = %.3f" % results["b_all_zero_over_validate"])
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
