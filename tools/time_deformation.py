#!/usr/bin/env python3
"""Device-event timings of flow2d_deformation_2d at 4096 x 4096 on the GPU: all nine planes with the record, the divergence
alone, and the record alone, each with and without a mask.  Median of REPEATS timed calls after a warm-up, one call between two
events; the rate is the algorithmic bytes of the call -- 8 per pixel read (12 with a mask), 4 per plane written -- over that
time.  Writes OUT/timings.json and prints one line per case.  No time is asserted anywhere.

  python tools/time_deformation.py [--size 4096] [--out profiles/deformation]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS, WARMUP = 20, 3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deformation"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    n = args.size
    rng = np.random.default_rng(0)
    with flow2d.Context(0) as ctx:
        pu = ctx.plane(n, n, rng.standard_normal((n, n)).astype(np.float32))
        pv = ctx.plane(n, n, rng.standard_normal((n, n)).astype(np.float32))
        pm = ctx.plane(n, n, (rng.random((n, n)) < 0.3).astype(np.float32))
        outs = {name: ctx.plane(n, n) for name in flow2d.DEFORMATION_PLANES}
        record = ctx.deformation_records()
        start, stop = ctx.event(), ctx.event()
        results = {"size": n, "device": ctx.device_name(), "repeats": REPEATS, "measure": "green_lagrange",
                   "workspace_bytes": flow2d.hip_lib().flow2d_deformation_workspace_bytes(n, n, 1), "cases": {}}
        cases = (("all_planes_and_stats", outs, record), ("divergence_only", {"divergence": outs["divergence"]}, None),
                 ("stats_only", {}, record))
        for name, planes, stats in cases:
            for mask in (None, pm):
                times = []
                for i in range(WARMUP + REPEATS):
                    ctx.record(start)
                    ctx.deformation(pu, pv, n, n, flow2d.STRAIN_GREEN_LAGRANGE, mask=mask, planes=planes, stats=stats)
                    ctx.record(stop)
                    ms = ctx.elapsed_ms(start, stop)
                    if i >= WARMUP:
                        times.append(ms)
                bytes_per_pixel = 8 + (4 if mask else 0) + 4 * len(planes)
                us = float(np.median(times)) * 1e3
                key = name + ("_masked" if mask else "")
                results["cases"][key] = {"median_us": us, "min_us": float(np.min(times)) * 1e3, "max_us": float(np.max(times)) * 1e3,
                                         "bytes_per_pixel": bytes_per_pixel, "tb_per_s": bytes_per_pixel * n * n / us * 1e-6,
                                         "launches": 2 if stats else 1}
                print("%-28s median %8.1f us  (min %.1f, max %.1f)  %2d B/pixel  %.2f TB/s" %
                      (key, us, np.min(times) * 1e3, np.max(times) * 1e3, bytes_per_pixel, results["cases"][key]["tb_per_s"]))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
