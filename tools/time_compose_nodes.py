#!/usr/bin/env python3
"""Device-event timings of flow2d_compose_nodes_2d on the GPU, medians of the timed rounds after a warm-up, on the two node grids
of a 4096 x 4096 frame -- 511 x 511 (radius 7, spacing 8) and the dense 4082 x 4082 (radius 7, spacing 1) -- beside, on the same
planes in the same run and in turn:

  compose      flow2d_compose_nodes_2d with a score and a record: 15 planes read at the node (the increment's at the four corners
               of a cell, mostly from the cache), 8 written
  compose_no_record   the same without the record: what the record's atomics, which all land on one 64-byte line, cost
  predict      one pass of flow2d_predict_nodes_2d with a record: 7 planes read, 7 written
  strain       flow2d_node_strain_2d with window 0, the nine planes, no record: 7 read, 9 written

The base is a rotation of 3 degrees about the grid's centre with 5 % of its nodes lost, the increment a smooth made-up field with
5 % lost.  Beside each time the bytes the kernel has to move at the least -- 4 bytes per node and plane read or written once -- and
what that makes per second.  Then whole calls of OpticalFlow.correlate_subset_sequence_device on five frames of SIZE x SIZE (band-
limited noise moved by (3.3, -1.6) per step): a new reference every 3 steps against the fixed reference, wall-clock (the call
synchronises once).  No time is asserted and there is no target.  Writes OUT/timings.json and prints one line per case.

  python tools/time_compose_nodes.py [--size 4096] [--rounds 7] [--out profiles/subset_reference]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
WARMUP = 1
R = 7


def fields(nw, nh, r, s, seed=0):
    """(base, increment, score): seven, seven and one [nh, nw] float32 arrays."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(nh, dtype=np.float64) * s, np.arange(nw, dtype=np.float64) * s, indexing="ij")
    cx, cy = xs.mean(), ys.mean()
    a = np.radians(3.0)
    g = (np.cos(a) - 1, -np.sin(a), np.sin(a), np.cos(a) - 1)
    base = [g[0] * (xs - cx) + g[1] * (ys - cy), g[2] * (xs - cx) + g[3] * (ys - cy)] + [np.full((nh, nw), q) for q in g]
    base.append(np.where(rng.random((nh, nw)) < 0.05, -3.0, 4.0))
    wave = np.sin(xs / 97.0) * np.cos(ys / 131.0)
    inc = [1.5 * wave, -0.8 * wave, 0.01 * wave, -0.005 * wave, 0.004 * wave, 0.012 * wave, np.where(rng.random((nh, nw)) < 0.05, -3.0, 5.0)]
    score = 0.9 + 0.1 * wave
    return [q.astype(np.float32) for q in base], [q.astype(np.float32) for q in inc], score.astype(np.float32)


def time_kernels(flow2d, ctx, size, r, s, rounds):
    nw, nh = flow2d.correlation_grid(size, size, r, s)
    base, inc, score = fields(nw, nh, r, s)
    pa, pb, psc = [ctx.plane(nw, nh, q) for q in base], [ctx.plane(nw, nh, q) for q in inc], ctx.plane(nw, nh, score)
    out = [ctx.plane(nw, nh) for _ in range(9)]
    crec, prec = ctx.compose_records(), ctx.predict_records()
    names = flow2d.DEFORMATION_PLANES
    begin, end = ctx.event(), ctx.event()
    cases = (("compose", lambda: ctx.compose_nodes(pa, pb, nw, nh, r, s, 1, psc, out[:6], out[6], out[7], crec), 15 + 8),
             ("compose_no_record", lambda: ctx.compose_nodes(pa, pb, nw, nh, r, s, 1, psc, out[:6], out[6], out[7], None), 15 + 8),
             ("predict", lambda: ctx.predict_nodes(pb[:6], pb[6], nw, nh, s, 1, 1, out[:6], out[6], prec), 7 + 7),
             ("strain", lambda: ctx.node_strain(pb[0], pb[1], nw, nh, s, window=0, state=pb[6], gradients=pb[2:6],
                                                planes=dict(zip(names, out)), stats=None), 7 + 9))
    times = {name: [] for name, _, _ in cases}
    for i in range(WARMUP + rounds):
        for name, call, _ in cases:  # in turn, so that a drift of the clocks meets all three alike
            ctx.record(begin)
            call()
            ctx.record(end)
            ms = ctx.elapsed_ms(begin, end)
            if i >= WARMUP:
                times[name].append(ms)
    result = {"nw": nw, "nh": nh, "radius": r, "spacing": s, "compose_record": ctx.read_compose_record(crec)[0].summary(), "cases": {}}
    for name, _, planes in cases:
        t = times[name]
        least = 4 * nw * nh * planes
        entry = {"median_us": 1e3 * float(np.median(t)), "min_us": 1e3 * float(np.min(t)), "max_us": 1e3 * float(np.max(t)), "planes_moved": planes,
                 "least_bytes": least, "GB_per_s": least / (1e6 * float(np.median(t)))}
        result["cases"][name] = entry
        print("%4d x %-4d %-8s median %9.1f us  (min %.1f, max %.1f, %d rounds)  %.1f MB at the least: %.0f GB/s" % (
            nw, nh, name, entry["median_us"], entry["min_us"], entry["max_us"], rounds, least / 1e6, entry["GB_per_s"]))
    for q in pa + pb + [psc] + out + [crec, prec]:
        q.free()
        ctx._planes.remove(q)
    return result


def time_sequences(flow2d, ctx, size, rounds):
    frames = importlib.import_module("time_subset_sequence").frames(size, 5)
    dev = [ctx.plane(size, size, f) for f in frames]
    names = flow2d.OpticalFlow.SUBSET_PLANES
    out = [{n: ctx.plane(size, size).ptr for n in names} for _ in range(4)]
    flow = flow2d.OpticalFlow(size, size, flow2d.GREY, ctx=ctx)
    result = {"size": size, "frames": 5, "passes": [[7, 8, 8]], "subset_radius": R, "cases": {}}
    try:
        times = {0: [], 3: []}
        for i in range(WARMUP + rounds):
            for every in (0, 3):
                t0 = time.perf_counter()
                _, steps = flow.correlate_subset_sequence_device([q.ptr for q in dev], 0.0, 1.0, [(7, 8, 8)], R, out, reference_every=every)
                ms = 1e3 * (time.perf_counter() - t0)
                if i >= WARMUP:
                    times[every].append(ms)
                result["cases"]["reference_every_%d" % every] = {"subset_records": [q.subset.summary() for q in steps],
                                                                  "compose_records": [q.summary() for q in flow.compose_records]}
        for every, t in times.items():
            entry = result["cases"]["reference_every_%d" % every]
            entry.update(median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)))
            print("four steps, reference_every %d: median %9.3f ms  (min %.3f, max %.3f, %d rounds)" % (every, entry["median_ms"], entry["min_ms"],
                                                                                                       entry["max_ms"], rounds))
    finally:
        flow.close()
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset_reference"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    with flow2d.Context(0) as ctx:
        results = {"device": ctx.device_name(), "rounds": args.rounds,
                   "grids": [time_kernels(flow2d, ctx, args.size, 7, s, args.rounds) for s in (8, 1)]}
        results["sequence"] = time_sequences(flow2d, ctx, args.size, args.rounds)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
