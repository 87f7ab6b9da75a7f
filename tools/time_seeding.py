#!/usr/bin/env python3
"""Device-event timings of the pyramid started from a prior flow, at 4096 x 4096 with the benchmark's configuration 3 (Gradient,
8 levels at scale 0.5, 10 x 5 sweeps, median 5, sigma 1.5, alpha 35):

  entry_*       flow2d_prior_registration_2d alone, the 4096^2 prior brought to the level the run would start at: 4096^2 (reach 1),
                2048^2 (reach 2) and 1024^2 (reach 4); beside each the bytes it moves -- both prior planes read once, three level
                planes written, frame 0 or the four gathers of frame 1 (counted as one level plane) -- and the rate that makes
  unseeded      OpticalFlow.compute_flow_device of the same build
  prior_reach_* OpticalFlow.compute_flow_from_prior_device at reach 2 (starts at level 1 of 8) and 4 (level 2), without the report
  chain         OpticalFlow.compute_flow_correlation_seeded_device (radius 7, range 8, spacing 8, reach 2): correlation, expansion,
                pyramid and the two records read back; the call synchronises twice inside, and the events span those waits too

The pyramids are recorded once into a HIP graph and replayed (what bench.py times); every figure is the median of the timed calls
after the warm-up, one call between two events.  The frames are uniform noise in u8's range, frame 1 = frame 0 moved by (2, 1) plus
noise, the prior the true motion plus noise of 0.2 px: none of the times depends on the content.  No time is asserted anywhere.
Writes OUT/timings.json and prints one line per case.

  python tools/time_seeding.py [--size 4096] [--out profiles/seeding]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, REPEATS = 2, 7
CONFIG_3 = (8, 0.5, 10, 5, 35.0, 0.001, 0.001, 5, 1.5)  # bench.py: cfg3_4096_gradient


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeding"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    n = args.size
    rng = np.random.default_rng(0)
    big = rng.uniform(0, 255, (n + 8, n + 8)).astype(np.float32)
    f0 = big[4:4 + n, 4:4 + n]
    f1 = (big[3:3 + n, 2:2 + n] + rng.normal(0, 6, (n, n))).astype(np.float32)
    prior = [(c + rng.normal(0, 0.2, (n, n))).astype(np.float32) for c in (2.0, 1.0)]
    with flow2d.Context(0) as ctx:
        p0, p1 = ctx.plane(n, n, f0), ctx.plane(n, n, f1)
        pu, pv = ctx.plane(n, n, prior[0]), ctx.plane(n, n, prior[1])
        out = [ctx.plane(n, n) for _ in range(3)]
        record = ctx.prior_records()
        start, stop = ctx.event(), ctx.event()
        results = {"size": n, "device": ctx.device_name(), "config": list(CONFIG_3), "warmup": WARMUP, "repeats": REPEATS, "cases": {}}

        def timed(call):
            times = []
            for i in range(WARMUP + REPEATS):
                ctx.record(start)
                call()
                ctx.record(stop)
                ms = ctx.elapsed_ms(start, stop)
                if i >= WARMUP:
                    times.append(ms)
            return {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times))}

        def report(name, case):
            results["cases"][name] = case
            extra = "  %.1f MB  %.0f GB/s" % (case["bytes"] * 1e-6, case["gb_per_s"]) if "bytes" in case else ""
            print("%-16s median %9.3f ms  (min %.3f, max %.3f)%s" % (name, case["median_ms"], case["min_ms"], case["max_ms"], extra))

        for reach in (1.0, 2.0, 4.0):
            level = flow2d.prior_start_level(n, n, CONFIG_3[0], CONFIG_3[1], reach)
            w = h = int(np.ceil(n * CONFIG_3[1] ** level))
            hx = float(np.float32(n) / np.float32(w))
            case = timed(lambda: ctx.prior_registration(pu, pv, n, n, out[0], out[1], p0, p1, w, h, hx, hx, out[2], record=record))
            case["level"], case["width"], case["height"] = level, w, h
            case["bytes"] = 2 * n * n * 4 + 4 * w * h * 4
            case["gb_per_s"] = case["bytes"] / case["median_ms"] * 1e-6
            report("entry_reach_%g" % reach, case)

        flow = flow2d.OpticalFlow(n, n, flow2d.GRADIENT, ctx=ctx)
        try:
            p = flow.params(*CONFIG_3)
            flow.use_graph(True)
            report("unseeded", timed(lambda: flow.compute_flow_device(p0.ptr, p1.ptr, out[0].ptr, out[1].ptr, p)))
            for reach in (2.0, 4.0):
                case = timed(lambda: flow.compute_flow_from_prior_device(p0.ptr, p1.ptr, pu.ptr, pv.ptr, out[0].ptr, out[1].ptr, p,
                                                                         reach=reach, report=False))
                case["start_level"] = flow2d.prior_start_level(n, n, CONFIG_3[0], CONFIG_3[1], reach)
                case["of_unseeded"] = case["median_ms"] / results["cases"]["unseeded"]["median_ms"]
                report("prior_reach_%g" % reach, case)
            last = {}

            def chain():
                last["report"], last["record"] = flow.compute_flow_correlation_seeded_device(p0.ptr, p1.ptr, out[0].ptr, out[1].ptr, p,
                                                                                             0.0, 1.0, 7, 8, 8, reach=2.0)
            case = timed(chain)
            case["report"], case["record"] = last["report"].summary(), last["record"].summary()
            case["of_unseeded"] = case["median_ms"] / results["cases"]["unseeded"]["median_ms"]
            report("chain", case)
        finally:
            flow.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
