#!/usr/bin/env python3
"""Accuracy of the motion segmentation on the analytic two_layer scene and sequence (scenes.make_scene / make_sequence).

Per pair: the regions of the residual flow against the true square -- the pixels whose ground-truth flow is not zero --: the
number of regions, and for the largest one its intersection over union with the square, the distance of its centroid from the
square's and the error of its mean residual motion against the square's true motion, in pixels.

  python tools/segmentation_table.py            every row; needs the GPU (flow, global motion, residual and labelling run on it)
  python tools/segmentation_table.py --numpy    the true-flow rows alone: the true flow as the residual (the background stands
                                                still) through the numpy restatement (tests/test_segmentation_cpu.py), no device
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
THRESHOLD, MIN_AREA, SIGMA, ITERATIONS = 0.5, 16, 0.5, 5
PARAMS = (50, 0.9, 40, 5, 35.0, 0.001, 0.001, 5, 1.5)  # the CLI's defaults


def score(labels, areas, centroids, motions, gt_u, gt_v, pair, source, engine):
    """One row: the largest region against the true square."""
    square = (gt_u != 0) | (gt_v != 0)
    ys, xs = np.nonzero(square)
    row = {"pair": pair, "source": source, "engine": engine, "regions": len(areas), "square": int(square.sum())}
    if not len(areas):
        return dict(row, area=0, iou=0.0, centroid_error=float("nan"), motion_error=float("nan"))
    k = int(np.argmax(areas))
    mine = labels == k + 1
    true_motion = (float(gt_u[square].astype(np.float64).mean()), float(gt_v[square].astype(np.float64).mean()))
    return dict(row, area=int(areas[k]), iou=float((mine & square).sum() / (mine | square).sum()),
                centroid_error=float(np.hypot(centroids[k][0] - xs.mean(), centroids[k][1] - ys.mean())),
                motion_error=float(np.hypot(motions[k][0] - true_motion[0], motions[k][1] - true_motion[1])))


def numpy_row(gt_u, gt_v, pair):
    ref = importlib.import_module("test_segmentation_cpu").segment_motion_reference(gt_u, gt_v, THRESHOLD, min_area=MIN_AREA)
    r = ref["all_regions"]
    area = r["area"].astype(np.float64)
    return score(ref["labels"], r["area"], list(zip(r["sum_x"] / area, r["sum_y"] / area)),
                 list(zip(r["sum_u_q16"] / 65536.0 / area, r["sum_v_q16"] / 65536.0 / area)), gt_u, gt_v, pair, "true", "numpy")


def pairs_of(size, seed, frames):
    sc = scenes.make_scene("two_layer", size, size, seed)
    yield "scene", sc.frame_0, sc.frame_1, sc.gt_u, sc.gt_v
    seq = scenes.make_sequence("two_layer", frames, size, size, seed)
    for k in range(frames - 1):
        yield "sequence %d-%d" % (k, k + 1), seq.frames[k], seq.frames[k + 1], seq.gt_u[k], seq.gt_v[k]


def gpu_rows(size, seed, frames):
    flow2d = importlib.import_module("cuda-flow2d_amd")
    rows = []
    with flow2d.Context(0) as ctx:
        flow = flow2d.OpticalFlow(size, size, flow2d.GREY, ctx=ctx)
        try:
            p = flow.params(*PARAMS)
            for pair, f0, f1, gt_u, gt_v in pairs_of(size, seed, frames):
                for masks in (False, True):
                    _, _, regions, labels = flow.segment_motion(f0, f1, p, flow2d.MOTION_AFFINE, SIGMA, ITERATIONS, THRESHOLD,
                                                                min_area=MIN_AREA, masks=masks)
                    rows.append(score(labels, [r.area for r in regions], [r.centroid for r in regions],
                                      [r.mean_motion for r in regions], gt_u, gt_v, pair, "grey, masks" if masks else "grey", "gpu"))
        finally:
            flow.close()
    return rows


def format_row(r):
    return "| %-13s | %-11s | %-5s | %3d | %6d | %6d | %.4f | %7.3f | %7.3f |" % (
        r["pair"], r["source"], r["engine"], r["regions"], r["area"], r["square"], r["iou"], r["centroid_error"], r["motion_error"])


HEADER = ("| pair | flows | engine | regions | area of the largest | true square | IoU | centroid error (px) | mean-motion error (px) |\n"
          "|---|---|---|---|---|---|---|---|---|\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true", help="the true-flow rows alone, from the numpy restatement")
    ap.add_argument("--size", type=int, default=256, help="square frames of this side (default 256)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segmentation"), help="where the table goes")
    args = ap.parse_args()
    rows = [numpy_row(gt_u, gt_v, pair) for pair, _, _, gt_u, gt_v in pairs_of(args.size, args.seed, args.frames)]
    if not args.numpy:
        rows += gpu_rows(args.size, args.seed, args.frames)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "table_numpy.md" if args.numpy else "table.md"), "w") as f:
        f.write("Motion segmentation of two_layer, %d x %d, seed %d, threshold %g px, min_area %d, affine global motion, sigma %g px, "
                "%d reweighted passes (tools/segmentation_table.py%s)\n\n"
                % (args.size, args.size, args.seed, THRESHOLD, MIN_AREA, SIGMA, ITERATIONS, " --numpy" if args.numpy else ""))
        f.write(HEADER)
        for r in rows:
            f.write(format_row(r) + "\n")
    for r in rows:
        print(format_row(r))


if __name__ == "__main__":
    main()
