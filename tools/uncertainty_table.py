#!/usr/bin/env python3
"""How well the node uncertainty (flow2d_subset_uncertainty_2d) predicts the scatter of the refinement's own output: the four
rows of tests/test_subset_uncertainty_cpu.py::calibration_row -- a 96 x 80 speckle scene, Gaussian noise of sigma grey values on
both frames, 24 draws from default_rng(1), the 63 interior nodes of the grid (7, s 8), every draw refined from the truth rounded to
whole pixels.  "ratio" is the predicted sigma, an RMS over nodes and draws, over the standard deviation of the refinement's output
across the draws, pooled as an RMS over the nodes; the last column is the mean of the noise plane over sqrt(2) sigma.

  python tools/uncertainty_table.py --numpy    the rows of the numpy restatement, no device: writes
                                               profiles/subset_uncertainty/table_numpy.md, the committed rows (and calibration.json)
  python tools/uncertainty_table.py            the device's rows (Context.subset_refine, Context.subset_uncertainty) into OUT/table.md;
                                               they must equal the committed rows digit for digit, else exit status 1
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HEADER = ("| scene | noise sigma | R | ratio u | ratio v | ratio ux | ratio uy | ratio vx | ratio vy | predicted sigma_u (px) | observed (px) | "
          "noise / (sqrt(2) sigma) |\n|" + "---|" * 12 + "\n")


def line(row):
    q = row["ratio"]
    return "| %s | %g | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.5f | %.5f | %.3f |\n" % (
        row["scene"], row["noise_sigma"], row["R"], q["u"], q["v"], q["ux"], q["uy"], q["vx"], q["vy"], row["predicted"]["u"], row["observed"]["u"],
        row["noise_over_root_two_sigma"])


def device_calls(T, scene_name, R):
    """(refine, evaluate, close): the device's counterparts of the two restatements for calibration_row."""
    flow2d = importlib.import_module("cuda-flow2d_amd")
    S = importlib.import_module("test_subset_cpu")
    ctx = flow2d.Context(0)
    r, s = 7, 8
    scene = S.make_case_scene(scene_name)
    h, w = scene.frame_0.shape
    u0, v0 = T.truth_at_nodes(scene, r, s)
    nh, nw = u0.shape
    u0 = np.where(S.interior_mask(nw, nh, w, h, r, T.MARGIN, s), u0, np.float32(np.nan))
    kept = {}

    def refine(f0, f1):
        for q in kept.pop("planes", []):
            q.free()
            ctx._planes.remove(q)
        p0, p1, pu, pv = ctx.plane(w, h, f0), ctx.plane(w, h, f1), ctx.plane(nw, nh, u0), ctx.plane(nw, nh, v0)
        outs = [ctx.plane(nw, nh) for _ in range(8)]
        ctx.subset_refine(p0, p1, w, h, pu, pv, nw, nh, r, s, R, out_u=outs[0], out_v=outs[1], out_gradients=outs[2:6], out_score=outs[6],
                          out_state=outs[7], record=None)
        kept["planes"] = [p0, p1, pu, pv] + outs
        got = S.Refined()
        for name, q in zip(S.Refined.NAMES, outs):
            setattr(got, name, q.download(nw, nh))
        return got

    def evaluate(f0, f1, got):
        p = kept["planes"]
        planes, _ = ctx.subset_uncertainty(p[0], p[1], w, h, p[4:10], p[11], nw, nh, r, s, R, record=None)
        out = T.Uncertainty()
        for name, plane in zip(T.PLANES, planes):
            setattr(out, name, plane)
        return out

    return refine, evaluate, ctx.close


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset_uncertainty"))
    args = ap.parse_args()
    T = importlib.import_module("test_subset_uncertainty_cpu")
    os.makedirs(args.out, exist_ok=True)
    committed = os.path.join(ROOT, "profiles", "subset_uncertainty", "table_numpy.md")  # the restatement's rows, kept in the repository
    if args.numpy:
        rows = T.calibration_rows()
        with open(T.CALIBRATION_PATH, "w") as f:
            json.dump(dict(source="numpy restatement (tests/test_subset_uncertainty_cpu.py)", rows=rows), f, indent=1, sort_keys=True)
            f.write("\n")
        with open(committed, "w") as f:
            f.write(HEADER)
            f.writelines(line(row) for row in rows)
        sys.stdout.write(HEADER + "".join(line(row) for row in rows))
        return 0
    got = []
    for name, sigma, R in T.CALIBRATION_ROWS:
        refine, evaluate, close = device_calls(T, name, R)
        try:
            got.append(line(T.calibration_row(name, sigma, R, refine, evaluate)))
        finally:
            close()
    with open(os.path.join(args.out, "table.md"), "w") as f:
        f.write(HEADER)
        f.writelines(got)
    sys.stdout.write(HEADER + "".join(got))
    want = open(committed).readlines()[2:]
    differing = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
    print("%d device rows -> %s; %s" % (len(got), os.path.join(args.out, "table.md"),
                                        "equal to the committed restatement rows" if got == want else "rows %s DIFFER from %s" % (differing, committed)))
    return 0 if got == want else 1


if __name__ == "__main__":
    sys.exit(main())
