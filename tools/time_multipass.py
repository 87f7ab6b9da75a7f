#!/usr/bin/env python3
"""Device-event timings of the multi-pass window correlation at 4096 x 4096 on the GPU, medians of the timed calls after a
warm-up, everything of one comparison in the same run:
  (a) flow2d_correlate_offset_2d with a NULL predictor on the PIV grid (radius 7, range 8, spacing 8) against
      flow2d_correlate_2d on the same setting: what staging per node instead of per tile costs;
  (b) the schedule 15:16:32, 7:4:8, 4:2:4 -- offset search, median test (REPLACE) and expansion per pass, queued back to back
      between two events, no host round trip -- against one flow2d_correlate_2d at radius 4, spacing 4 and range 22, the
      smallest that covers the schedule's reach of 16 + 4 + 2 px;
  (c) flow2d_validate_nodes_2d alone on the finest grid of (b).
The frames are uniform noise in u8's range, frame 1 = frame 0 moved by (3, -2) plus noise; the offset kernel's time depends on
the content only through the predictor, which sends the search areas of (b)'s later passes to other places.  No time is
asserted.  Writes OUT/timings.json and prints one line per case.

  python tools/time_multipass.py [--size 4096] [--out profiles/multipass]
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
SCHEDULE = ((15, 16, 32), (7, 4, 8), (4, 2, 4))
SINGLE = (4, sum(p[1] for p in SCHEDULE), 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multipass"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    n = args.size
    rng = np.random.default_rng(0)
    big = rng.uniform(0, 255, (n + 8, n + 8)).astype(np.float32)
    f0 = big[4:4 + n, 4:4 + n]
    f1 = (big[6:6 + n, 1:1 + n] + rng.normal(0, 6, (n, n))).astype(np.float32)
    with flow2d.Context(0) as ctx:
        p0, p1 = ctx.plane(n, n, f0), ctx.plane(n, n, f1)
        raw, val, dense = ([ctx.plane(n, n) for _ in range(2)] for _ in range(3))
        score = ctx.plane(n, n)
        record, passes, checks = ctx.correlation_records(), ctx.pass_records(), ctx.pass_records()
        start, stop = ctx.event(), ctx.event()
        results = {"size": n, "device": ctx.device_name(), "cases": {}}

        def timed(name, call, repeats, **extra):
            times = []
            for i in range(WARMUP + repeats):
                ctx.record(start)
                call()
                ctx.record(stop)
                ms = ctx.elapsed_ms(start, stop)
                if i >= WARMUP:
                    times.append(ms)
            entry = dict({"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times)),
                          "repeats": repeats}, **extra)
            results["cases"][name] = entry
            print("%-28s median %9.3f ms  (min %.3f, max %.3f, %d calls)  %s" % (name, entry["median_ms"], entry["min_ms"], entry["max_ms"],
                                                                                repeats, json.dumps(extra) if extra else ""))
            return entry["median_ms"]

        # (a)
        r, d, s = 7, 8, 8
        tile = timed("a_correlate_r7_d8_s8", lambda: ctx.correlate(p0, p1, n, n, 0.0, 1.0, r, d, s, -1.0, raw[0], raw[1], score, record), 10)
        node = timed("a_offset_null_r7_d8_s8",
                     lambda: ctx.correlate_offset(p0, p1, n, n, 0.0, 1.0, r, d, s, -1.0, None, raw[0], raw[1], score, passes), 10)
        results["a_offset_over_correlate"] = node / tile
        print("(a) per-node staging / per-tile staging = %.3f" % (node / tile))

        # (b)
        def chain():
            pred = None
            for k, (r, d, s) in enumerate(SCHEDULE):
                nw, nh = flow2d.correlation_grid(n, n, r, s)
                ctx.correlate_offset(p0, p1, n, n, 0.0, 1.0, r, d, s, -1.0, pred, raw[0], raw[1], score if k == len(SCHEDULE) - 1 else None, passes)
                ctx.validate_nodes(raw[0], raw[1], nw, nh, 2.0, 0.1, 3, flow2d.VALIDATE_REPLACE, val[0], val[1], None, checks)
                ctx.expand_nodes(val[0], val[1], nw, nh, r, s, dense[0], dense[1], n, n)
                pred = dense

        multi = timed("b_schedule_15:16:32_7:4:8_4:2:4", chain, 5)
        last = ctx.read_correlation_pass_record(passes)[0].summary()
        r, d, s = SINGLE
        one = timed("b_correlate_r4_d22_s4", lambda: ctx.correlate(p0, p1, n, n, 0.0, 1.0, r, d, s, -1.0, raw[0], raw[1], score, record), 3)
        results["b_schedule_over_single"] = multi / one
        results["b_last_pass_record"] = last
        print("(b) schedule / single pass = %.3f   last pass: %s" % (multi / one, json.dumps(last)))
        for k, (r, d, s) in enumerate(SCHEDULE):  # the passes on their own, with the predictor (b) left behind
            timed("b_pass_%d_offset_%d:%d:%d" % (k + 1, r, d, s),
                  lambda: ctx.correlate_offset(p0, p1, n, n, 0.0, 1.0, r, d, s, -1.0, dense, raw[0], raw[1], None, passes), 5)

        # (c)
        r, d, s = SCHEDULE[-1]
        nw, nh = flow2d.correlation_grid(n, n, r, s)
        timed("c_validate_%dx%d" % (nw, nh), lambda: ctx.validate_nodes(raw[0], raw[1], nw, nh, 2.0, 0.1, 3, flow2d.VALIDATE_REPLACE, val[0], val[1],
                                                                    None, checks), 10, nodes=nw * nh,
              record=ctx.read_validation_record(checks)[0].summary())
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
