#!/usr/bin/env python3
"""Device-event timings of flow2d_refine_flow_2d at 4096 x 4096 on the GPU for r = 3, 5, 7 with guide, mask and record, on two
flows: `scene` -- two_layer's true flow with the occlusions smeared and 0.05 px of noise, what a computed flow looks like: the
bisection closes after about as many steps as neighbouring vectors differ in bits -- and `random` -- independent N(0, 3) vectors,
the selection's worst case.  Median of REPEATS timed calls after a warm-up, one call between two events.

The kernel is bound by the vector units and LDS, not by bytes, so its rate is given in lane-operations per second: per wave 64
lanes x (the vector instructions of the weight phase + steps x those of one bisection pass), with the instruction counts taken
from the compiled kernel (VALU + LDS instructions of the unrolled loops) and the steps counted here, in numpy,
from the same input: a wave runs as many steps as its widest key range has bits.  No time is asserted anywhere.
Writes OUT/timings.json and prints one line per case.

  python tools/time_refinement.py [--size 4096] [--out profiles/refinement]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS, WARMUP = 10, 2
SIGMA_GUIDE = 25.0
# vector + LDS instructions per sample of the compiled kernel with guide and mask: the weight phase, and one
# bisection pass over both components
WEIGHT_OPS_PER_SAMPLE, STEP_OPS_PER_SAMPLE = 33, 7


def keys(a):
    b = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return np.where(b >> 31, ~b, b | np.uint32(0x80000000)).astype(np.uint64)


def window_extreme(a, r, take, neutral):
    """take (np.minimum / np.maximum) over the (2r + 1)^2 window, the frame's outside holding `neutral`."""
    for axis in (0, 1):
        p = np.pad(a, [(r, r) if k == axis else (0, 0) for k in (0, 1)], constant_values=neutral)
        out = np.full_like(a, neutral)
        for d in range(2 * r + 1):
            out = take(out, np.take(p, np.arange(d, d + a.shape[axis]), axis=axis))
        a = out
    return a


def mean_wave_steps(u, v, mask, r):
    """The mean number of bisection steps of a wave (64 consecutive pixels of a row): the bits of the widest key range among its
    lanes and both components, over the samples that count (usable vectors with a mask value below 1)."""
    with np.errstate(invalid="ignore"):
        counts = (np.abs(u) <= 1e9) & (np.abs(v) <= 1e9) & (mask < 1)
    steps = np.zeros(u.shape, np.int64)
    top = np.uint64(0xFFFFFFFF)
    for a in (u, v):
        k = keys(a)
        lo = window_extreme(np.where(counts, k, top), r, np.minimum, top)
        hi = window_extreme(np.where(counts, k, np.uint64(0)), r, np.maximum, np.uint64(0))
        span = np.where(hi > lo, hi - lo, 0).astype(np.float64)
        steps = np.maximum(steps, np.ceil(np.log2(span + 1)).astype(np.int64))
    h, w = steps.shape
    w64 = w // 64 * 64
    return float(steps[:, :w64].reshape(h, -1, 64).max(axis=2).mean())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refinement"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    scenes = importlib.import_module("cuda-flow2d_amd.scenes")
    n = args.size
    rng = np.random.default_rng(0)
    sc = scenes.make_scene("two_layer", n, n, seed=0)
    occ = sc.occlusion > 0
    su, sv = sc.gt_u.copy(), sc.gt_v.copy()
    su[occ], sv[occ] = 4.5, -2.25
    su += (0.05 * rng.standard_normal((n, n))).astype(np.float32)
    sv += (0.05 * rng.standard_normal((n, n))).astype(np.float32)
    flows = {"scene": (su, sv, sc.occlusion.astype(np.float32)),
             "random": ((3 * rng.standard_normal((n, n))).astype(np.float32), (3 * rng.standard_normal((n, n))).astype(np.float32),
                        (rng.random((n, n)) < 0.1).astype(np.float32))}
    with flow2d.Context(0) as ctx:
        guide = ctx.plane(n, n, sc.frame_0)
        ou, ov, record = ctx.plane(n, n), ctx.plane(n, n), ctx.refine_records()
        start, stop = ctx.event(), ctx.event()
        results = {"size": n, "device": ctx.device_name(), "repeats": REPEATS, "sigma_guide": SIGMA_GUIDE, "cases": {}}
        for name, (u, v, mask) in flows.items():
            pu, pv, pm = ctx.plane(n, n, u), ctx.plane(n, n, v), ctx.plane(n, n, mask)
            for r in (3, 5, 7):
                times = []
                for i in range(WARMUP + REPEATS):
                    ctx.record(start)
                    ctx.refine_flow(pu, pv, n, n, r, guide, pm, SIGMA_GUIDE, 0.0, ou, ov, record)
                    ctx.record(stop)
                    ms = ctx.elapsed_ms(start, stop)
                    if i >= WARMUP:
                        times.append(ms)
                rec = ctx.read_refine_record(record)[0].summary()
                steps = mean_wave_steps(u, v, mask, r)
                samples = (2 * r + 1) ** 2
                lane_ops = n * n * samples * (WEIGHT_OPS_PER_SAMPLE + steps * STEP_OPS_PER_SAMPLE)
                ms = float(np.median(times))
                key = "%s_r%d" % (name, r)
                results["cases"][key] = {"median_ms": ms, "min_ms": float(np.min(times)), "max_ms": float(np.max(times)),
                                         "mean_wave_steps": steps, "lane_ops": lane_ops, "tera_lane_ops_per_s": lane_ops / ms * 1e-9,
                                         "record": rec}
                print("%-12s median %8.3f ms  (min %.3f, max %.3f)  %5.1f steps per wave  %.2f T lane-ops/s  %s" %
                      (key, ms, np.min(times), np.max(times), steps, lane_ops / ms * 1e-9, json.dumps(rec)))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
