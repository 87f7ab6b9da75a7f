#!/usr/bin/env python3
"""Device times of temporal denoising at 4096 x 4096 (one process, one device; the variants alternate, medians of >= 20 launches):

  fused      one flow2d_denoise_2d launch with N = 2 and N = 4 neighbours, without and with occlusion masks
  N warps    N launches of flow2d_registration_2d: what warping the neighbours onto the centre took before that entry
  compose    one flow2d_compose_flow_2d launch with masks
  sequence   OpticalFlow.denoise_sequence_device (radius 1, masks) per frame, beside one ComputeFlowBidirectionalDevice pair

    python tools/time_denoising.py [--size 4096] [--launches 25] [--frames 4] [--sequence-runs 5] [--out profiles/denoising]
                                 [--no-sequence]

Writes OUT/time_denoising_<size>.json, which tools/denoising_table.py puts into OUT/README.md."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

flow2d = importlib.import_module("cuda-flow2d_amd")

PARAMS = (50, 0.9, 40, 5, 35.0, 0.001, 0.001, 5, 1.5)
F32 = np.float32
PEAK = 8.0e12


def timed(ctx, call, events=[]):
    """Device milliseconds of call(); one start / stop pair of events, created on first use and kept."""
    if not events:
        events.extend((ctx.event(), ctx.event()))
    start, stop = events
    ctx.record(start)
    call()
    ctx.record(stop)
    return ctx.elapsed_ms(start, stop)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=25)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoising"))
    ap.add_argument("--sequence-runs", type=int, default=5, help="repetitions of the whole-sequence timing (median)")
    ap.add_argument("--no-sequence", action="store_true")
    args = ap.parse_args()
    n = args.size
    rng = np.random.default_rng(0)
    ctx = flow2d.Context(0)
    result = {"size": n, "launches": args.launches, "device": ctx.device_name(), "kernels": []}
    try:
        # frames of noise; flows of a translation of a few pixels plus sub-pixel noise: the access pattern of a real flow
        centre = ctx.plane(n, n, rng.uniform(0, 255, (n, n)).astype(F32))
        frames = [ctx.plane(n, n, rng.uniform(0, 255, (n, n)).astype(F32)) for _ in range(4)]
        us = [ctx.plane(n, n, (rng.uniform(-6, 6) + rng.normal(0, 0.5, (n, n))).astype(F32)) for _ in range(4)]
        vs = [ctx.plane(n, n, (rng.uniform(-6, 6) + rng.normal(0, 0.5, (n, n))).astype(F32)) for _ in range(4)]
        occs = [ctx.plane(n, n, (rng.random((n, n)) < 0.1).astype(F32)) for _ in range(4)]
        out, warped, out_v, out_m = (ctx.plane(n, n) for _ in range(4))
        variants = {}
        for k in (2, 4):
            variants["fused_%d" % k] = lambda k=k: ctx.denoise(centre, frames[:k], us[:k], vs[:k], n, n, out)
            variants["masks_%d" % k] = lambda k=k: ctx.denoise(centre, frames[:k], us[:k], vs[:k], n, n, out, occs[:k])
            variants["warps_%d" % k] = lambda k=k: [ctx.registration(centre, frames[j], us[j], vs[j], n, n, 1.0, 1.0, warped)
                                                    for j in range(k)]
        variants["compose"] = lambda: ctx.compose_flow(us[0], vs[0], us[1], vs[1], n, n, out, out_v, occs[0], occs[1], out_m)
        times = {name: [] for name in variants}
        for name, call in variants.items():  # warm-up
            call()
        ctx.synchronize()
        for _ in range(args.launches):
            for name, call in variants.items():
                times[name].append(timed(ctx, call))
        med = {name: statistics.median(t) for name, t in times.items()}
        for k in (2, 4):
            px = float(n) * n
            result["kernels"].append({
                "n": k, "fused_ms": med["fused_%d" % k], "fused_masks_ms": med["masks_%d" % k], "warps_ms": med["warps_%d" % k],
                "fraction_no_masks": px * (8 + 12 * k) / (med["fused_%d" % k] * 1e-3) / PEAK,
                "fraction_masks": px * (8 + 16 * k) / (med["masks_%d" % k] * 1e-3) / PEAK,
                "fused_min_ms": min(times["fused_%d" % k]), "warps_min_ms": min(times["warps_%d" % k])})
        result["compose_ms"] = med["compose"]
        if not args.no_sequence:
            flow = flow2d.OpticalFlow(n, n, flow2d.GREY, ctx=ctx)
            try:
                p = flow.params(*PARAMS)
                # a textured sequence moving by (1.5, -0.75) px per frame, with noise
                ys, xs = np.mgrid[0:n, 0:n].astype(F32)
                seq = []
                for k in range(args.frames):
                    img = 128 + 60 * np.sin((xs - 1.5 * k) / 9.0) * np.cos((ys + 0.75 * k) / 7.0)
                    seq.append(ctx.plane(n, n, (img + rng.normal(0, 4, (n, n))).astype(F32)))
                outs = [ctx.plane(n, n) for _ in range(args.frames)]
                pair = [ctx.plane(n, n) for _ in range(6)]
                run_seq = lambda: flow.denoise_sequence_device([q.ptr for q in seq], [o.ptr for o in outs], p, 1, 0.0, True)  # noqa: E731
                run_pair = lambda: flow.compute_flow_bidirectional_device(  # noqa: E731
                    [seq[0].ptr, seq[1].ptr], [pair[0].ptr], [pair[1].ptr], [pair[2].ptr], [pair[3].ptr], p, [pair[4].ptr],
                    [pair[5].ptr])
                run_seq()
                run_pair()
                ctx.synchronize()
                t_seq, t_pair = [], []
                for _ in range(args.sequence_runs):
                    t_seq.append(timed(ctx, run_seq))
                    t_pair.append(timed(ctx, run_pair))
                result["sequence"] = {"frames": args.frames, "runs": args.sequence_runs,
                                      "per_frame_ms": statistics.median(t_seq) / args.frames,
                                      "pair_ms": statistics.median(t_pair)}
            finally:
                flow.close()
    finally:
        ctx.close()
    print(json.dumps(result, indent=1))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "time_denoising_%d.json" % n), "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
