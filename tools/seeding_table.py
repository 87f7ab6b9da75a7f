#!/usr/bin/env python3
"""What starting the variational pyramid from the window correlation's field gives on the speckle scenes: the mean endpoint error
over the pixels at least r + d from the border of the unseeded flow, of the expanded node field (NaN taken as 0) and of the flow
from that field as prior at reach 1, 2 and 4 -- per motion of scenes.make_speckle_scene, seed 0 .. 2 and data term (Grey,
Gradient), with the CLI's default parameters, radius 7, spacing 8, range 6 (12 for the large translation).

The numpy/oracle rows -- the restatement of tests/test_prior_cpu.py over the oracle's stages -- are always computed; the GPU rows
(OpticalFlow.compute_flow and compute_flow_correlation_seeded) where a device is present, or never with --numpy.
Writes OUT/table.md, or OUT/table_numpy.md when there are no GPU rows.

  python tools/seeding_table.py [--numpy] [--seeds 3] [--out profiles/seeding]
"""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

scenes = importlib.import_module("cuda-flow2d_amd.scenes")
PARAMS = (50, 0.9, 40, 5, 35.0, 0.001, 0.001, 5, 1.5)  # the CLI's defaults
RADIUS, SPACING = 7, 8
REACHES = (1.0, 2.0, 4.0)
TERMS = (("Grey", 0), ("Gradient", 1))


def search(motion):
    return 12 if motion == "large_translation" else 6


def oracle_rows(width, height, seeds):
    T = importlib.import_module("test_prior_cpu")
    from oracle import oracle as O
    O.build()
    rows = []
    for motion in scenes.SPECKLE_MOTIONS:
        for seed in seeds:
            sc = scenes.make_speckle_scene(motion, width, height, seed)
            d = search(motion)
            pu, pv, _ = T.correlation_prior(sc.frame_0, sc.frame_1, RADIUS, d, SPACING)
            su, sv, count = T.sanitise(pu, pv)
            for term, constancy in TERMS:
                plain = O.compute_flow(sc.frame_0, sc.frame_1, *PARAMS, constancy)[:2]
                row = {"scene": sc.name, "seed": seed, "term": term, "engine": "oracle", "not_finite": count,
                       "unseeded": T.interior_epe(*plain, sc, RADIUS + d), "nodes": T.interior_epe(su, sv, sc, RADIUS + d), "prior": {}}
                for reach in REACHES:
                    start = T.start_level(width, height, PARAMS[0], PARAMS[1], reach)
                    u, v, _ = T.compute_flow_from_prior(O, sc.frame_0, sc.frame_1, pu, pv, *PARAMS, constancy, start)
                    row["prior"][reach] = (start, T.interior_epe(u, v, sc, RADIUS + d))
                rows.append(row)
    return rows


def gpu_rows(width, height, seeds):
    T = importlib.import_module("test_prior_cpu")
    flow2d = importlib.import_module("cuda-flow2d_amd")
    rows = []
    with flow2d.Context(0) as ctx:
        for term, constancy in TERMS:
            flow = flow2d.OpticalFlow(width, height, constancy, ctx=ctx)
            try:
                p = flow.params(*PARAMS)
                for motion in scenes.SPECKLE_MOTIONS:
                    for seed in seeds:
                        sc = scenes.make_speckle_scene(motion, width, height, seed)
                        d = search(motion)
                        plain = flow.compute_flow(sc.frame_0, sc.frame_1, p)[:2]
                        row = {"scene": sc.name, "seed": seed, "term": term, "engine": "gpu", "unseeded": T.interior_epe(*plain, sc, RADIUS + d),
                               "prior": {}}
                        for reach in REACHES:
                            out = flow.compute_flow_correlation_seeded(sc.frame_0, sc.frame_1, p, RADIUS, d, SPACING, reach=reach)
                            row["prior"][reach] = (out["report"].start_level, T.interior_epe(out["u"], out["v"], sc, RADIUS + d))
                        su, sv, count = T.sanitise(*out["prior"])
                        row["nodes"], row["not_finite"] = T.interior_epe(su, sv, sc, RADIUS + d), count
                        rows.append(row)
            finally:
                flow.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true", help="the numpy/oracle rows alone")
    ap.add_argument("--width", type=int, default=96)
    ap.add_argument("--height", type=int, default=80)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeding"))
    args = ap.parse_args()
    seeds = list(range(args.seeds))
    rows = oracle_rows(args.width, args.height, seeds)
    with_gpu = not args.numpy and importlib.import_module("cuda-flow2d_amd").device_count() > 0
    if with_gpu:
        rows += gpu_rows(args.width, args.height, seeds)
    rows.sort(key=lambda q: (q["scene"], q["seed"], q["term"], q["engine"]))
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "table.md" if with_gpu else "table_numpy.md")
    with open(path, "w") as f:
        f.write("| scene | seed | data term | engine | unseeded | expanded nodes | prior pixels not finite |" +
                "".join(" from prior, reach %g (start level) |" % r for r in REACHES) + "\n")
        f.write("|" + "---|" * (7 + len(REACHES)) + "\n")
        for q in rows:
            f.write("| %s | %d | %s | %s | %.3f | %.3f | %d |" % (q["scene"], q["seed"], q["term"], q["engine"], q["unseeded"], q["nodes"],
                                                                 q["not_finite"]) +
                    "".join(" %.3f (%d) |" % (q["prior"][r][1], q["prior"][r][0]) for r in REACHES) + "\n")
    print("%d rows -> %s" % (len(rows), path))


if __name__ == "__main__":
    main()
