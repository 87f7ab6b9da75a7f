#!/usr/bin/env python3
"""What the second-order subset refinement (flow2d_subset_refine2_2d) gains over the first-order one where subsets bend: per scene
and subset radius the mean and largest endpoint error of order 1 (the restatement of flow2d_subset_refine_2d) and of order 2 on the
same starts and the same scored nodes, the iterations of the converged nodes, the ratio of the two mean errors and the mean of the
six recovered curvatures.  Scenes: the two bending scenes of scenes.py (kappa = 0.004 per pixel, translation (1.6, -0.7)) at R = 7
and R = 11, and the affine "stretch" scene at R = 7, all 96 x 80 on the grid r = 7, s = 8, started from the restatement of
flow2d_correlate_2d at d = 6 with zero gradients and curvatures; scored: the nodes whose subset, grown by d, lies inside the frame.

  python tools/subset2_table.py --numpy    the rows of the numpy restatement (tests/test_subset2_cpu.py), no device:
                                           writes profiles/subset2/table_numpy.md, the committed rows
  python tools/subset2_table.py            the device's rows (Context.subset_refine2) into OUT/table.md; they must equal the
                                           committed rows digit for digit, else exit status 1
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HEADER = ("| scene | R | nodes | order 1, mean / max EPE (px) | order 2, mean / max EPE (px) | order 1 / order 2 | converged, order 1, 2 | "
          "iterations, order 1 -> 2 | mean uxx, uxy, uyy, vxx, vxy, vyy |\n|" + "---|" * 9 + "\n")
CASES = [("bend", 7), ("bend", 11), ("bulge", 7), ("bulge", 11), ("stretch", 7)]


def line(q):
    return "| %s | %d | %d | %.4f / %.4f | %.4f / %.4f | %.2f | %d, %d | %.2f -> %.2f | %s |\n" % (
        q["scene"], q["R"], q["nodes"], q["order1_mean_epe"], q["order1_max_epe"], q["order2_mean_epe"], q["order2_max_epe"],
        q["order1_mean_epe"] / q["order2_mean_epe"], q["order1_converged"], q["order2_converged"], q["order1_iterations"],
        q["order2_iterations"], ", ".join("%.5f" % q["mean_curvature"][c] for c in ("uxx", "uxy", "uyy", "vxx", "vxy", "vyy")))


def device_refine(T):
    """(refine, close): the device's counterpart of subset_refine2_reference, as a test_subset2_cpu.Refined2."""
    flow2d = importlib.import_module("cuda-flow2d_amd")
    ctx = flow2d.Context(0)

    def refine(f0, f1, u0, v0, r, s, R):
        h, w = f0.shape
        nh, nw = u0.shape
        u, v, gradients, curvatures, score, state, rec = ctx.subset_refine2(ctx.plane(w, h, f0), ctx.plane(w, h, f1), w, h, ctx.plane(nw, nh, u0),
                                                                            ctx.plane(nw, nh, v0), nw, nh, r, s, R)
        out = T.Refined2()
        for name, plane in zip(("u", "v") + T.GRADIENTS + T.CURVATURES + ("score", "state"), (u, v) + gradients + curvatures + (score, state)):
            setattr(out, name, plane)
        out.record = np.frombuffer(bytes(rec), T.SUBSET_DTYPE)
        return out

    return refine, ctx.close


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset2"))
    args = ap.parse_args()
    T = importlib.import_module("test_subset2_cpu")
    os.makedirs(args.out, exist_ok=True)
    committed = os.path.join(ROOT, "profiles", "subset2", "table_numpy.md")  # the restatement's rows, kept in the repository
    if args.numpy:
        rows = [T.scene_figures(name, R) for name, R in CASES]
        with open(committed, "w") as f:
            f.write(HEADER)
            f.writelines(line(q) for q in rows)
        print("%d rows -> %s" % (len(rows), committed))
        return 0
    refine, close = device_refine(T)
    try:
        got = [line(T.scene_figures(name, R, refine)) for name, R in CASES]
    finally:
        close()
    with open(os.path.join(args.out, "table.md"), "w") as f:
        f.write(HEADER)
        f.writelines(got)
    want = open(committed).readlines()[2:]
    differing = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
    print("%d device rows -> %s; %s" % (len(got), os.path.join(args.out, "table.md"),
                                        "equal to the committed restatement rows" if got == want else "rows %s DIFFER from %s" % (differing, committed)))
    return 0 if got == want else 1


if __name__ == "__main__":
    sys.exit(main())
