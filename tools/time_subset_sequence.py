#!/usr/bin/env python3
"""Device-event timings of one step of a DIC sequence at 4096 x 4096 on the GPU, grid (radius 7, spacing 8) -- 511 x 511 nodes --,
subsets of R = 7, three things in the same run, in turn, medians of the timed rounds after a warm-up:

  chained      a later step as OpticalFlow2D::CorrelateSubsetSequence runs it: two passes of flow2d_predict_nodes_2d on the previous
               step's planes, then flow2d_subset_refine_from_2d of (frame 0, frame 2) with max_shift 4
  pair_chain   the body of OpticalFlow2D::CorrelateSubsetDevice on the same frames: the search (flow2d_correlate_offset_2d, range 8),
               flow2d_validate_nodes_2d by replacement, flow2d_subset_refine_2d with max_shift 2
  prediction   the two prediction passes alone

The frames are band-limited noise in u8's range (white noise low-passed with a Gaussian of sigma 1.5 px); frame k is frame 0 moved by
k x (3.3, -1.6) by a phase shift, so the previous step's result -- the pair chain on (frame 0, frame 1), computed once before the
timing -- is 3.6 px from the step's answer.  No time is asserted and there is no target: the figures are stated against the pair
chain for what they are, with the records, which say how many iterations ran.  Writes OUT/timings.json and prints one line per case.

  python tools/time_subset_sequence.py [--size 4096] [--rounds 7] [--out profiles/subset_sequence]
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
R = 7
SHIFT = (3.3, -1.6)


def frames(n, count, seed=0):
    rng = np.random.default_rng(seed)
    spectrum = np.fft.rfft2(rng.standard_normal((n, n)))
    ky, kx = np.fft.fftfreq(n)[:, None], np.fft.rfftfreq(n)[None, :]
    spectrum *= np.exp(-2.0 * (np.pi * 1.5) ** 2 * (kx * kx + ky * ky))
    out = [np.fft.irfft2(spectrum * np.exp(-2j * np.pi * k * (kx * SHIFT[0] + ky * SHIFT[1])), (n, n)) for k in range(count)]
    lo, hi = out[0].min(), out[0].max()
    return [((a - lo) * (255.0 / (hi - lo))).astype(np.float32) for a in out]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset_sequence"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    n = args.size
    f0, f1, f2 = frames(n, 3)
    r, d, s = GRID
    with flow2d.Context(0) as ctx:
        p0, p1, p2 = (ctx.plane(n, n, f) for f in (f0, f1, f2))
        nw, nh = flow2d.correlation_grid(n, n, r, s)
        new = lambda k: [ctx.plane(nw, nh) for _ in range(k)]  # noqa: E731
        raw, start, previous, ping, pong, chained, alone = new(2), new(2), new(8), new(7), new(7), new(8), new(8)
        passes, checks, counts, alone_counts = ctx.pass_records(), ctx.pass_records(), ctx.subset_records(), ctx.subset_records()
        predicted = [ctx.predict_records() for _ in range(2)]
        begin, end = ctx.event(), ctx.event()

        def pair_chain(frame, out, record):
            ctx.correlate_offset(p0, frame, n, n, 0.0, 1.0, r, d, s, -1.0, None, raw[0], raw[1], None, passes)
            ctx.validate_nodes(raw[0], raw[1], nw, nh, 2.0, 0.1, 3, flow2d.VALIDATE_REPLACE, start[0], start[1], None, checks)
            ctx.subset_refine(p0, frame, n, n, start[0], start[1], nw, nh, r, s, R, out_u=out[0], out_v=out[1], out_gradients=out[2:6],
                              out_score=out[6], out_state=out[7], record=record)

        def prediction():
            ctx.predict_nodes(previous[:6], previous[7], nw, nh, s, 1, 1, ping[:6], ping[6], predicted[0])
            ctx.predict_nodes(ping[:6], ping[6], nw, nh, s, 1, 1, pong[:6], pong[6], predicted[1])

        def chained_step():
            prediction()
            ctx.subset_refine_from(p0, p2, n, n, pong[0], pong[1], pong[2:6], nw, nh, r, s, R, max_shift=4.0, out_u=chained[0], out_v=chained[1],
                                   out_gradients=chained[2:6], out_score=chained[6], out_state=chained[7], record=counts)

        pair_chain(p1, previous, alone_counts)  # step 1, once
        ctx.synchronize()
        first = ctx.read_subset_record(alone_counts)[0].summary()
        cases = (("chained", chained_step), ("pair_chain", lambda: pair_chain(p2, alone, alone_counts)), ("prediction", prediction))
        times = {name: [] for name, _ in cases}
        for i in range(WARMUP + args.rounds):
            for name, call in cases:  # in turn, so that a drift of the clocks meets all three alike
                ctx.record(begin)
                call()
                ctx.record(end)
                ms = ctx.elapsed_ms(begin, end)
                if i >= WARMUP:
                    times[name].append(ms)
        records = {"chained": ctx.read_subset_record(counts)[0].summary(), "pair_chain": ctx.read_subset_record(alone_counts)[0].summary(),
                   "prediction": [ctx.read_predict_record(q)[0].summary() for q in predicted]}
        results = {"size": n, "device": ctx.device_name(), "grid": {"radius": r, "range": d, "spacing": s, "nw": nw, "nh": nh}, "subset_radius": R,
                   "shift_per_step": SHIFT, "rounds": args.rounds, "step_1_record": first, "cases": {}}
        truth = (2 * SHIFT[0], 2 * SHIFT[1])
        for name, planes in (("chained", chained), ("pair_chain", alone)):
            state, u, v = planes[7].download(nw, nh), planes[0].download(nw, nh), planes[1].download(nw, nh)
            good = state >= 1
            records[name + "_converged_mean_error_px"] = float(np.hypot(u[good] - truth[0], v[good] - truth[1]).mean()) if good.any() else None
        for name, _ in cases:
            t = times[name]
            entry = {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t)), "record": records[name]}
            if name != "prediction":
                entry["converged_mean_error_px"] = records[name + "_converged_mean_error_px"]
                entry["us_per_node_iteration"] = 1e3 * entry["median_ms"] / max(records[name]["iterations"], 1)
            results["cases"][name] = entry
            print("%-12s median %9.3f ms  (min %.3f, max %.3f, %d rounds)  %s" % (name, entry["median_ms"], entry["min_ms"], entry["max_ms"],
                                                                                 args.rounds, json.dumps(entry["record"])))
        c = results["cases"]
        results["chained_over_pair_chain"] = c["chained"]["median_ms"] / c["pair_chain"]["median_ms"]
        results["prediction_share_of_chained"] = c["prediction"]["median_ms"] / c["chained"]["median_ms"]
        print("a chained step takes %.2f x the pair chain; the prediction is %.1f %% of it" % (
            results["chained_over_pair_chain"], 100 * results["prediction_share_of_chained"]))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
