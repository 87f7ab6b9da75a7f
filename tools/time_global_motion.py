#!/usr/bin/env python3
"""Device-event timings of the global-motion entries at 4096 x 4096 on the GPU: flow2d_global_motion_2d for each model with K = 0
and K = 5 reweighted passes (with and without a mask), flow2d_global_flow_2d and flow2d_warp_global_2d.  Median of REPEATS
timed calls after a warm-up, one call between two events.  Writes OUT/timings.json and prints one line per variant.

  python tools/time_global_motion.py [--size 4096] [--out profiles/global_motion]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_motion"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    n = args.size
    rng = np.random.default_rng(0)
    with flow2d.Context(0) as ctx:
        u = ctx.plane(n, n, (1.5 + rng.normal(0, 0.5, (n, n))).astype(np.float32))
        v = ctx.plane(n, n, (-0.75 + rng.normal(0, 0.5, (n, n))).astype(np.float32))
        mask = ctx.plane(n, n, (rng.random((n, n)) < 0.1).astype(np.float32))
        frame = ctx.plane(n, n, rng.uniform(1, 255, (n, n)).astype(np.float32))
        outs = [ctx.plane(n, n) for _ in range(5)]
        motion = ctx.motion_records()
        variants = {}
        for model, name in enumerate(("translation", "similarity", "affine")):
            for k in (0, 5):
                variants["fit_%s_K%d" % (name, k)] = lambda model=model, k=k: ctx.global_motion(u, v, n, n, model, 0.5, k, motion=motion)
        variants["fit_affine_K5_mask"] = lambda: ctx.global_motion(u, v, n, n, 2, 0.5, 5, mask, motion=motion)
        variants["global_flow_all_outputs"] = lambda: ctx.global_flow(motion, n, n, u, v, mask, 0.5, *outs)
        variants["global_flow_residual"] = lambda: ctx.global_flow(motion, n, n, u, v, residual_u=outs[2], residual_v=outs[3])
        variants["warp_global"] = lambda: ctx.warp_global(motion, frame, n, n, outs[0])
        variants["warp_global_valid"] = lambda: ctx.warp_global(motion, frame, n, n, outs[0], outs[1])
        start, stop = ctx.event(), ctx.event()
        results = {"size": n, "device": ctx.device_name(), "repeats": REPEATS, "ms": {}}
        ctx.global_motion(u, v, n, n, 2, 0.5, 5, motion=motion)  # a record for the per-pixel entries
        for name, call in variants.items():
            times = []
            for i in range(WARMUP + REPEATS):
                ctx.record(start)
                call()
                ctx.record(stop)
                ms = ctx.elapsed_ms(start, stop)
                if i >= WARMUP:
                    times.append(ms)
            results["ms"][name] = {"median": float(np.median(times)), "min": float(np.min(times)), "max": float(np.max(times))}
            print("%-28s median %.4f ms  (min %.4f, max %.4f)" % (name, np.median(times), np.min(times), np.max(times)))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
