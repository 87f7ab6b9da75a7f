#!/usr/bin/env python3
"""How well window correlation (flow2d_correlate_2d) places its nodes: the endpoint error of the interior nodes -- those whose
whole search lies inside the frame, r + d <= centre <= size - 1 - r - d -- against the analytic ground truth, per scene and
setting.  Scenes: the three speckle motions of scenes.make_speckle_scene (seeds 0 .. 2) and, for contrast, the sinusoid
`translation` and `affine` of scenes.SCENES, whose long periods leave a 15 x 15 window little to hold on to.

  python tools/correlation_table.py            every row; needs the GPU: the kernel's rows, and beside each the EPE of the
                                               variational flow (the CLI's default parameters) sampled at the same nodes
  python tools/correlation_table.py --numpy    the rows of the numpy restatement (tests/test_correlate_cpu.py) alone, no device
Writes OUT/table.md, or OUT/table_numpy.md with --numpy.
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

scenes = importlib.import_module("cuda-flow2d_amd.scenes")
PARAMS = (50, 0.9, 40, 5, 35.0, 0.001, 0.001, 5, 1.5)  # the CLI's defaults
SPACING = 8
RADII = (4, 7, 10)


def cases(width, height, seeds):
    """(scene, seed, range) per case: range 6 for the small motions, 12 for the large translation."""
    out = []
    for motion in scenes.SPECKLE_MOTIONS:
        for seed in seeds:
            out.append((scenes.make_speckle_scene(motion, width, height, seed), seed, 12 if motion == "large_translation" else 6))
    for name in ("translation", "affine"):
        out.append((scenes.make_scene(name, width, height, seeds[0]), seeds[0], 6))
    return out


def row(sc, seed, engine, r, d, u, v, rec, flow=None):
    T = importlib.import_module("test_correlate_cpu")
    err = T.interior_epe(u, v, sc, r, d, SPACING)
    out = {"scene": sc.name, "seed": seed, "engine": engine, "r": r, "d": d, "nodes": err.size, "mean": float(np.nanmean(err)),
           "max": float(np.nanmax(err)), "lost": int(np.isnan(err).sum()), "record": rec, "flow": None}
    if flow is not None:
        nh, nw = u.shape
        cy, cx = r + np.arange(nh) * SPACING, r + np.arange(nw) * SPACING
        out["flow"] = float(T.interior_epe(flow[0][np.ix_(cy, cx)], flow[1][np.ix_(cy, cx)], sc, r, d, SPACING).mean())
    return out


def numpy_rows(all_cases):
    T = importlib.import_module("test_correlate_cpu")
    rows = []
    for sc, seed, d in all_cases:
        lo, scale = T.frame_range(sc.frame_0, sc.frame_1)
        for r in RADII:
            u, v, _, rec, _ = T.correlate_reference(sc.frame_0, sc.frame_1, lo, scale, r, d, SPACING)
            rows.append(row(sc, seed, "numpy", r, d, u, v, {k: int(rec[k][0]) for k in rec.dtype.names}))
    return rows


def gpu_rows(all_cases, width, height):
    flow2d = importlib.import_module("cuda-flow2d_amd")
    rows = []
    with flow2d.Context(0) as ctx:
        flow = flow2d.OpticalFlow(width, height, flow2d.GREY, ctx=ctx)
        try:
            p = flow.params(*PARAMS)
            for sc, seed, d in all_cases:
                fu, fv, _ = flow.compute_flow(sc.frame_0, sc.frame_1, p)
                for r in RADII:
                    u, v, _, rec, _ = flow.correlate(sc.frame_0, sc.frame_1, r, d, SPACING)
                    rows.append(row(sc, seed, "gpu", r, d, u, v, rec.summary(), (fu, fv)))
        finally:
            flow.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--width", type=int, default=96)
    ap.add_argument("--height", type=int, default=80)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correlation"))
    args = ap.parse_args()
    all_cases = cases(args.width, args.height, list(range(args.seeds)))
    rows = numpy_rows(all_cases)
    if not args.numpy:
        rows += gpu_rows(all_cases, args.width, args.height)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "table_numpy.md" if args.numpy else "table.md")
    with open(path, "w") as f:
        f.write("| scene | seed | engine | r | d | s | interior nodes | mean EPE | max EPE | lost | invalid | unrefined | variational flow, same nodes |\n")
        f.write("|" + "---|" * 13 + "\n")
        for q in rows:
            f.write("| %s | %d | %s | %d | %d | %d | %d | %.4f | %.4f | %d | %d | %d | %s |\n" %
                    (q["scene"], q["seed"], q["engine"], q["r"], q["d"], SPACING, q["nodes"], q["mean"], q["max"], q["lost"],
                     q["record"]["invalid"], q["record"]["unrefined"], "-" if q["flow"] is None else "%.4f" % q["flow"]))
    print("%d rows -> %s" % (len(rows), path))


if __name__ == "__main__":
    main()
