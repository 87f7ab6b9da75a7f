#!/usr/bin/env python3
"""Device-event timings of flow2d_subset_refine_2d at 4096 x 4096 on the GPU, medians of the timed calls after a warm-up, beside
flow2d_correlate_2d on the same grid in the same run: the grid (radius 7, spacing 8) -- 511 x 511 nodes -- refined with subsets of
R = 7 and of R = 15, each from the validated node field of flow2d_correlate_2d (range 8) on the pair.
The frames are band-limited noise in u8's range (white noise low-passed with a Gaussian of sigma 1.5 px), frame 1 = frame 0 moved
by (3.3, -1.6) by a phase shift: the subsets have something to converge on, and the record says how many iterations ran -- the
refinement's time is proportional to them, so "us per node and iteration" is printed as well.  No time is asserted.  Writes
OUT/timings.json and prints one line per case.

  python tools/time_subset.py [--size 4096] [--out profiles/subset]
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
GRID = (7, 8, 8)  # radius, range, spacing
SHIFT = (3.3, -1.6)


def frames(n, seed=0):
    rng = np.random.default_rng(seed)
    spectrum = np.fft.rfft2(rng.standard_normal((n, n)))
    ky, kx = np.fft.fftfreq(n)[:, None], np.fft.rfftfreq(n)[None, :]
    spectrum *= np.exp(-2.0 * (np.pi * 1.5) ** 2 * (kx * kx + ky * ky))
    moved = spectrum * np.exp(-2j * np.pi * (kx * SHIFT[0] + ky * SHIFT[1]))
    f0, f1 = np.fft.irfft2(spectrum, (n, n)), np.fft.irfft2(moved, (n, n))
    lo, hi = f0.min(), f0.max()
    to_u8 = lambda a: ((a - lo) * (255.0 / (hi - lo))).astype(np.float32)  # noqa: E731
    return to_u8(f0), to_u8(f1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    n = args.size
    f0, f1 = frames(n)
    r, d, s = GRID
    with flow2d.Context(0) as ctx:
        p0, p1 = ctx.plane(n, n, f0), ctx.plane(n, n, f1)
        nw, nh = flow2d.correlation_grid(n, n, r, s)
        raw, start, out = ([ctx.plane(nw, nh) for _ in range(k)] for k in (3, 2, 8))
        record, checks, counts = ctx.correlation_records(), ctx.pass_records(), ctx.subset_records()
        begin, end = ctx.event(), ctx.event()
        results = {"size": n, "device": ctx.device_name(), "grid": {"radius": r, "range": d, "spacing": s, "nw": nw, "nh": nh},
                   "shift": SHIFT, "cases": {}}

        def timed(name, call, repeats, after=None):
            times = []
            for i in range(WARMUP + repeats):
                ctx.record(begin)
                call()
                ctx.record(end)
                ms = ctx.elapsed_ms(begin, end)
                if i >= WARMUP:
                    times.append(ms)
            extra = after() if after else {}
            entry = dict({"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times)),
                          "repeats": repeats}, **extra)
            results["cases"][name] = entry
            print("%-28s median %9.3f ms  (min %.3f, max %.3f, %d calls)  %s" % (name, entry["median_ms"], entry["min_ms"], entry["max_ms"],
                                                                                repeats, json.dumps(extra) if extra else ""))
            return entry

        search = timed("correlate_r%d_d%d_s%d" % GRID, lambda: ctx.correlate(p0, p1, n, n, 0.0, 1.0, r, d, s, -1.0, raw[0], raw[1], raw[2], record),
                       10, lambda: {"record": ctx.read_correlation_record(record)[0].summary()})
        ctx.validate_nodes(raw[0], raw[1], nw, nh, 2.0, 0.1, 3, flow2d.VALIDATE_REPLACE, start[0], start[1], None, checks)
        for R in (7, 15):
            def after():
                rec = ctx.read_subset_record(counts)[0].summary()
                return {"record": rec}

            entry = timed("subset_refine_R%d" % R,
                          lambda: ctx.subset_refine(p0, p1, n, n, start[0], start[1], nw, nh, r, s, R, out_u=out[0], out_v=out[1],
                                                    out_gradients=out[2:6], out_score=out[6], out_state=out[7], record=counts), 5, after)
            rec = entry["record"]
            entry["us_per_node_iteration"] = 1e3 * entry["median_ms"] / max(rec["iterations"], 1)
            entry["over_correlate"] = entry["median_ms"] / search["median_ms"]
            state = out[7].download(nw, nh)
            u, v = out[0].download(nw, nh), out[1].download(nw, nh)
            good = state >= 1
            entry["converged_mean_error_px"] = float(np.hypot(u[good] - SHIFT[0], v[good] - SHIFT[1]).mean()) if good.any() else None
            print("    R = %d: %.3f us per node and iteration, %.2f x the search; converged nodes' mean error %s px" % (
                R, entry["us_per_node_iteration"], entry["over_correlate"], entry["converged_mean_error_px"]))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
