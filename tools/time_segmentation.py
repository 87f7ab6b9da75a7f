#!/usr/bin/env python3
"""Device-event timings of flow2d_segment_motion_2d at 4096 x 4096 on the GPU for three inputs: the residuals of two_layer (one
square on an empty frame), a full-foreground frame (one region: the worst case for the atomics) and site noise at p = 0.59
(near the percolation threshold: large ragged clusters).  Median of REPEATS timed calls after a warm-up, one call between two
events.  Writes OUT/timings.json and prints one line per input.

  python tools/time_segmentation.py [--size 4096] [--out profiles/segmentation]
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
MAX_REGIONS = 4096


def inputs(n):
    scenes = importlib.import_module("cuda-flow2d_amd.scenes")
    sc = scenes.make_scene("two_layer", n, n, 0)
    yield "two_layer", sc.gt_u, sc.gt_v
    yield "full_foreground", np.full((n, n), 2.0, np.float32), np.full((n, n), -1.0, np.float32)
    rng = np.random.default_rng(0)
    yield "noise_p0.59", np.where(rng.random((n, n)) < 0.59, 2.0, 0.0).astype(np.float32), np.zeros((n, n), np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segmentation"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    n = args.size
    with flow2d.Context(0) as ctx:
        ru, rv, labels = ctx.plane(n, n), ctx.plane(n, n), ctx.plane(n, n)
        regions, summary = ctx.region_records(MAX_REGIONS), ctx.segment_summaries()
        start, stop = ctx.event(), ctx.event()
        workspace = flow2d.hip_lib().flow2d_segment_motion_workspace_bytes(n, n, 1)
        results = {"size": n, "device": ctx.device_name(), "repeats": REPEATS, "max_regions": MAX_REGIONS, "workspace_bytes": workspace,
                   # read: the two residual planes by the tile pass, the border pairs and the label pass; written: the labels
                   "plane_bytes_per_pixel": 8 + 8 + 4, "workspace_bytes_per_pixel": workspace / float(n * n), "ms": {}}
        for name, u, v in inputs(n):
            ru.upload(u)
            rv.upload(v)
            times = []
            for i in range(WARMUP + REPEATS):
                ctx.record(start)
                ctx.segment_motion(ru, rv, n, n, 0.5, max_regions=MAX_REGIONS, labels=labels, regions=regions, summary=summary)
                ctx.record(stop)
                ms = ctx.elapsed_ms(start, stop)
                if i >= WARMUP:
                    times.append(ms)
            s = ctx.read_segment_summary(summary)[0]
            results["ms"][name] = {"median": float(np.median(times)), "min": float(np.min(times)), "max": float(np.max(times)),
                                   "regions": s.region_count, "foreground": s.foreground}
            print("%-16s median %.4f ms  (min %.4f, max %.4f)  %d regions, %d foreground pixels" %
                  (name, np.median(times), np.min(times), np.max(times), s.region_count, s.foreground))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
