#!/usr/bin/env python3
"""Device-event timings of the warm start, at 4096 x 4096 with the benchmark's configuration 3 (Gradient, 8 levels at scale 0.5,
10 x 5 sweeps, median 5, sigma 1.5, alpha 35), and the same pair at scale 0.9 on a frame that fits (--size-09, 50 levels asked for):

  propagate_*   flow2d_propagate_flow_2d alone (Context.propagate_flow with the caller's planes, record and workspace): without and
                with the two frames (the photometric term), at 0 and 4 fill passes; beside each the bytes it moves at the least --
                8 per pixel of flow read (16 + the gathers, counted as one plane, with frames), the 8-byte key written by the atomic
                and read by the resolve, 8 of winners gathered, 8 stored, 16 per fill pass -- and the rate that makes
  plain_pair    the second pair of OpticalFlow.compute_flow_sequence_device over three frames: sequence minus its first pair,
                timed as the difference of the medians of a three-frame and a two-frame call
  warm_pair     the same for OpticalFlow.compute_flow_sequence_warm_device (reach 2, four fill passes, photometric scale 1, no
                adaptation, no reports): propagation included

Sequences run eagerly (they are not recorded into graphs); every figure is the median of the timed calls after the warm-up, one
call between two events.  The frames are uniform noise in u8's range, each the one before moved by (2, 1) plus noise, the flow to
propagate the true motion plus noise of 0.2 px.  No time is asserted anywhere.  Writes OUT/timings.json and prints one line per case.

  python tools/time_warmstart.py [--size 4096] [--size-09 1024] [--out profiles/warmstart]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, REPEATS = 2, 7
CONFIG_3 = (8, 0.5, 10, 5, 35.0, 0.001, 0.001, 5, 1.5)  # bench.py: cfg3_4096_gradient
CONFIG_09 = (50, 0.9, 10, 5, 35.0, 0.001, 0.001, 5, 1.5)


def frames_for(n, count, rng):
    big = rng.uniform(0, 255, (n + 8 * count, n + 8 * count)).astype(np.float32)
    return [(big[4 * count - k:4 * count - k + n, 4 * count - 2 * k:4 * count - 2 * k + n] + (rng.normal(0, 6, (n, n)) if k else 0)).astype(np.float32)
            for k in range(count)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--size-09", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warmstart"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    rng = np.random.default_rng(0)
    with flow2d.Context(0) as ctx:
        start, stop = ctx.event(), ctx.event()
        results = {"device": ctx.device_name(), "warmup": WARMUP, "repeats": REPEATS, "cases": {}}

        def timed(call):
            times = []
            for i in range(WARMUP + REPEATS):
                ctx.record(start)
                call()
                ctx.record(stop)
                ms = ctx.elapsed_ms(start, stop)
                if i >= WARMUP:
                    times.append(ms)
            return {"median_ms": float(np.median(times)), "min_ms": float(np.min(times)), "max_ms": float(np.max(times))}

        def report(name, case):
            results["cases"][name] = case
            extra = "  %.1f MB  %.0f GB/s" % (case["bytes"] * 1e-6, case["gb_per_s"]) if "bytes" in case else ""
            print("%-26s median %9.3f ms  (min %.3f, max %.3f)%s" % (name, case["median_ms"], case["min_ms"], case["max_ms"], extra), flush=True)

        n = args.size
        frames = frames_for(n, 3, rng)
        planes = [ctx.plane(n, n, f) for f in frames]
        pu, pv = (ctx.plane(n, n, (c + rng.normal(0, 0.2, (n, n))).astype(np.float32)) for c in (2.0, 1.0))
        out = [ctx.plane(n, n) for _ in range(4)]
        record, work = ctx.propagate_records(), ctx.propagate_workspace(n, n)
        for with_frames in (False, True):
            for fill in (0, 4):
                kw = dict(frame_from=planes[0], frame_to=planes[1]) if with_frames else {}
                case = timed(lambda: ctx.propagate_flow(pu, pv, n, n, fill_passes=fill, out_u=out[0], out_v=out[1], record=record, workspace=work,
                                                        **kw))
                case["bytes"] = n * n * ((24 if with_frames else 8) + 8 + 8 + 8 + 8 + 16 * fill)
                case["gb_per_s"] = case["bytes"] / case["median_ms"] * 1e-6
                case["record"] = ctx.read_propagate_record(record)[0].summary()
                report("propagate_%s_fill_%d" % ("frames" if with_frames else "plain", fill), case)

        def pairs(name, size, config, dev_frames, flows):
            flow = flow2d.OpticalFlow(size, size, flow2d.GRADIENT, ctx=ctx)
            try:
                p = flow.params(*config)
                f, us, vs = [q.ptr for q in dev_frames], [flows[0].ptr, flows[2].ptr], [flows[1].ptr, flows[3].ptr]
                medians = {}
                for kind, call in (("plain", lambda k: flow.compute_flow_sequence_device(f[:k], us[:k - 1], vs[:k - 1], p)),
                                   ("warm", lambda k: flow.compute_flow_sequence_warm_device(f[:k], us[:k - 1], vs[:k - 1], p, reach=2.0))):
                    two, three = timed(lambda: call(2)), timed(lambda: call(3))
                    case = {"median_ms": three["median_ms"] - two["median_ms"], "min_ms": three["min_ms"] - two["max_ms"],
                            "max_ms": three["max_ms"] - two["min_ms"], "three_frames": three, "two_frames": two, "size": size, "config": list(config)}
                    if kind == "warm":
                        case["start_level"] = flow2d.prior_start_level(size, size, config[0], config[1], 2.0)
                        case["levels"] = min(config[0], flow2d.max_warp_level(size, size, config[1]))
                        case["of_plain"] = case["median_ms"] / medians["plain"]
                    medians[kind] = case["median_ms"]
                    report("%s_pair_%s" % (kind, name), case)
            finally:
                flow.close()

        pairs("4096_scale_0.5", n, CONFIG_3, planes, out)
        for q in planes + out + [pu, pv, work]:
            q.free()
            ctx._planes.remove(q)
        m = args.size_09
        small = [ctx.plane(m, m, f) for f in frames_for(m, 3, rng)]
        pairs("%d_scale_0.9" % m, m, CONFIG_09, small, [ctx.plane(m, m) for _ in range(4)])
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "timings.json"), "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
