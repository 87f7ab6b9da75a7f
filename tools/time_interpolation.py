#!/usr/bin/env python3
"""Times flow2d_interpolate_2d at 4096^2 on the MI355X with device events: K = 1, 2, 4 fixed-point iterations, with both
occlusion masks and without.  Prints one JSON line per form: microseconds per call and the algorithmic bytes over that time
(unique bytes: 8 planes read and 1 written, 36 B/px with masks, 28 without), also as a fraction of 8 TB/s.
Run it under `rocprofv3 --kernel-trace --stats` for the kernel's own times (profiles/interpolation/).

    python tools/time_interpolation.py [--size 4096] [--calls 50]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
flow2d = importlib.import_module("cuda-flow2d_amd")

PEAK_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    if flow2d.device_count() < 1:
        sys.exit("no HIP device: timing needs the MI355X")
    n = args.size
    rng = np.random.default_rng(0)
    frames = [rng.uniform(0, 255, (n, n)).astype(np.float32) for _ in range(2)]
    # a smooth flow of a few pixels and its approximate inverse, as the bidirectional path delivers them
    ys, xs = np.mgrid[0:n, 0:n].astype(np.float32)
    u = (3.0 + 2.0 * np.sin(xs / 97.0)).astype(np.float32)
    v = (-1.5 + 1.0 * np.cos(ys / 131.0)).astype(np.float32)
    masks = [(rng.random((n, n)) < 0.05).astype(np.float32) for _ in range(2)]
    with flow2d.Context(0) as ctx:
        f0, f1, pu, pv, bu, bv, o0, o1 = (ctx.plane(n, n, a) for a in frames + [u, v, -u, -v] + masks)
        out = ctx.plane(n, n)
        start, stop = ctx.event(), ctx.event()
        for masked in (True, False):
            for k in (1, 2, 4):
                def call():
                    ctx.interpolate(f0, f1, pu, pv, bu, bv, n, n, 0.5, out, o0 if masked else None, o1 if masked else None,
                                    k, 0.5)
                for _ in range(5):
                    call()
                ctx.synchronize()
                ctx.record(start)
                for _ in range(args.calls):
                    call()
                ctx.record(stop)
                us = ctx.elapsed_ms(start, stop) * 1e3 / args.calls
                bytes_ = (36 if masked else 28) * n * n
                print(json.dumps({"form": "masks" if masked else "no_masks", "iterations": k, "size": n, "calls": args.calls,
                                  "us_per_call": round(us, 2), "algorithmic_bytes": bytes_, "tb_per_s": round(bytes_ / us / 1e6, 3),
                                  "fraction_of_8tbs": round(bytes_ / (us * 1e-6) / PEAK_BYTES_PER_S, 3)}))


if __name__ == "__main__":
    main()
