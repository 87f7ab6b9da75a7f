#!/usr/bin/env python3
"""What the subset refinement (flow2d_subset_refine_2d) gains over the parabola of flow2d_correlate_2d: per scene the mean endpoint
error of the parabola and of the subsets on the same interior nodes, the largest one, the error of the four displacement gradients
against np.gradient of the ground truth (per node the root of the four squared errors; the largest single component), the
iterations of the converged interior nodes and the record.  Scenes: the three speckle motions and the three speckle deformations
of scenes.py at 96 x 80, grid r = 7, s = 8, subset R = 7, started from the restatement of flow2d_correlate_2d.

  python tools/subset_table.py --numpy    the rows of the numpy restatement (tests/test_subset_cpu.py), no device:
                                          writes profiles/subset/table_numpy.md, the committed rows
  python tools/subset_table.py            the device's rows (Context.subset_refine) into OUT/table.md; they must equal the
                                          committed rows digit for digit, else exit status 1
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
HEADER = ("| scene (range d) | interior nodes | parabola, mean EPE | subset, mean / max EPE | gradient error, mean / max | "
          "iterations, mean / max | record |\n|" + "---|" * 7 + "\n")


def line(q):
    return "| speckle %s (%d) | %d | %.4f | %.4f / %.4f | %.4f / %.4f | %.2f / %d | %s |\n" % (
        q["scene"], q["range"], q["interior"], q["parabola_mean_epe"], q["subset_mean_epe"], q["subset_max_epe"], q["gradient_mean_error"],
        q["gradient_max_error"], q["iterations_mean"], q["iterations_max"], json.dumps(q["record"]))


def device_refine(T):
    """(refine, close): the device's counterpart of subset_refine_reference, as a test_subset_cpu.Refined."""
    flow2d = importlib.import_module("cuda-flow2d_amd")
    ctx = flow2d.Context(0)

    def refine(f0, f1, u0, v0, r, s, R):
        h, w = f0.shape
        nh, nw = u0.shape
        u, v, gradients, score, state, rec = ctx.subset_refine(ctx.plane(w, h, f0), ctx.plane(w, h, f1), w, h, ctx.plane(nw, nh, u0),
                                                               ctx.plane(nw, nh, v0), nw, nh, r, s, R)
        out = T.Refined()
        for name, plane in zip(T.Refined.NAMES, (u, v) + gradients + (score, state)):
            setattr(out, name, plane)
        out.record = np.frombuffer(bytes(rec), T.SUBSET_DTYPE)
        return out

    return refine, ctx.close


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset"))
    args = ap.parse_args()
    T = importlib.import_module("test_subset_cpu")
    os.makedirs(args.out, exist_ok=True)
    committed = os.path.join(ROOT, "profiles", "subset", "table_numpy.md")  # the restatement's rows, kept in the repository
    if args.numpy:
        rows = [T.scene_figures(name, d, None) for name, d in T.SCENE_CASES]
        with open(committed, "w") as f:
            f.write(HEADER)
            f.writelines(line(q) for q in rows)
        print("%d scenes -> %s" % (len(rows), committed))
        return 0
    refine, close = device_refine(T)
    try:
        got = [line(T.scene_figures(name, d, refine)) for name, d in T.SCENE_CASES]
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
