#!/usr/bin/env python3
"""Times flow2d_track_points_2d and flow2d_seed_points_2d at 4096^2 on the MI355X with device events, at spacing 1 (16.7 M
tracks) and spacing 4 (1.05 M).  Prints one JSON line per kernel and spacing: microseconds per call and the algorithmic bytes
over that time, also as a fraction of 8 TB/s.

Bytes counted (unique, per slot or cell):
  track  35 B/slot: 16 B of table (x, y read; x, y written), 1 B of reason, and the flow gather -- two coherent flow pairs,
         the forward pair at the track and the backward pair at its new position: 16 B when neighbouring lanes share their
         neighbourhoods, as they do for a dense table (the boundary taps hit the same lines) -- plus the count, amortised
  seed   8 B per live track (x, y read by the marking pass), the frame (4 B per pixel at spacing 1, where the 5x5 windows
         of neighbouring cells overlap; 16 B per cell at spacing 4), 3 B of coverage flag per cell (cleared, marked,
         decided) and 8 B per seed written
The track table is a dense grid of tracks at the seed pixels carried by a smooth flow of a few pixels, every slot alive.
Seeding runs with every cell covered but those a 5 % hole leaves open (the usual case after the first frame).
Run it under `rocprofv3 --kernel-trace --stats` for the kernels' own times (profiles/tracking/).

    python tools/time_tracking.py [--size 4096] [--calls 20]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
flow2d = importlib.import_module("cuda-flow2d_amd")

PEAK_BYTES_PER_S = 8e12
F32 = np.float32


def timed(ctx, call, calls, reset=None):
    """Microseconds per call: back to back, or each call alone after reset() when given."""
    for _ in range(3):
        if reset:
            reset()
        call()
    ctx.synchronize()
    start, stop = ctx.event(), ctx.event()
    if reset is None:
        ctx.record(start)
        for _ in range(calls):
            call()
        ctx.record(stop)
        return ctx.elapsed_ms(start, stop) * 1e3 / calls
    total = 0.0
    for _ in range(calls):
        reset()
        ctx.record(start)
        call()
        ctx.record(stop)
        total += ctx.elapsed_ms(start, stop) * 1e3
    return total / calls


def line(kernel, us, bytes_, **kw):
    return json.dumps(dict({"kernel": kernel}, **kw, us_per_call=round(us, 2), algorithmic_bytes=int(bytes_),
                           tb_per_s=round(bytes_ / us / 1e6, 3),
                           fraction_of_8tbs=round(bytes_ / (us * 1e-6) / PEAK_BYTES_PER_S, 3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if flow2d.device_count() < 1:
        sys.exit("no HIP device: timing needs the MI355X")
    n = args.size
    rng = np.random.default_rng(0)
    ys, xs = np.mgrid[0:n, 0:n].astype(F32)
    u = (3.0 + 2.0 * np.sin(xs / 97.0)).astype(F32)
    v = (-1.5 + 1.0 * np.cos(ys / 131.0)).astype(F32)
    frame = rng.uniform(0, 255, (n, n)).astype(F32)
    del xs, ys
    with flow2d.Context(0) as ctx:
        pu, pv, bu, bv, pf = (ctx.plane(n, n, a) for a in (u, v, -u, -v, frame))
        for s in (1, 4):
            gy, gx = np.mgrid[s // 2:n:s, s // 2:n:s].astype(F32)
            cap = gx.size
            tx, ty = ctx.plane(cap, 1, gx.reshape(1, -1)), ctx.plane(cap, 1, gy.reshape(1, -1))
            ox, oy = ctx.plane(cap, 1), ctx.plane(cap, 1)
            reason = ctx.plane(cap // 4, 1)
            count = ctx.counter(cap)

            def track():
                ctx.track_points(pu, pv, bu, bv, n, n, tx, ty, count, cap, ox, oy, reason)

            us = timed(ctx, track, args.calls)
            print(line("track_points", us, 35 * cap, size=n, spacing=s, slots=cap, calls=args.calls), flush=True)
            keep = rng.random(cap) >= 0.05  # a 5 % hole: about 5 % of the cells get a seed
            live = int(keep.sum())
            hx = np.full(2 * cap, np.nan, F32)
            hy = np.full(2 * cap, np.nan, F32)
            hx[:live], hy[:live] = gx.ravel()[keep], gy.ravel()[keep]
            sx, sy = ctx.plane(2 * cap, 1, hx.reshape(1, -1)), ctx.plane(2 * cap, 1, hy.reshape(1, -1))
            seed_count = ctx.counter(live)
            start_count = np.frombuffer(np.array([live, 0], np.uint64).tobytes(), F32).reshape(1, 4)

            def reset():
                seed_count.upload(start_count)

            def seed():
                ctx.seed_points(pf, n, n, s, sx, sy, seed_count, 2 * cap, 0.0)

            us = timed(ctx, seed, args.calls, reset)
            seeds = ctx.read_count(seed_count) - live
            frame_bytes = 4 * n * n if s == 1 else 16 * cap
            print(line("seed_points", us, 8 * live + frame_bytes + 3 * cap + 8 * seeds, size=n, spacing=s, cells=cap,
                       live_tracks=live, seeds=seeds, calls=args.calls), flush=True)
            for p in (tx, ty, ox, oy, reason, count, sx, sy, seed_count):
                p.free()
                ctx._planes.remove(p)


if __name__ == "__main__":
    main()
