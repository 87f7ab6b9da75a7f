#!/usr/bin/env python3
"""What a mask gains the subset refinement at a specimen's edge: per deformation of scenes.make_speckle_specimen (a plate with a
hole in front of a static background, 96 x 80, seed 0) the edge nodes -- on the specimen, with a subset that is not all usable --
under the refinement as it is (flow2d_subset_refine_from_2d), under the mask by the header's rule (flow2d_subset_refine_masked_2d,
min_pixels 57) and, from the restatement only, under a mask that drops the excluded pixels alone (no stencil rule): converged
nodes, the mean and the worst endpoint error over the edge nodes, and the RMS error of ux of a second run whose starts are the
truth rounded to whole pixels.  The grid is r = 7, s = 8; the chain is the search (d = 6), the validation with replacement and the
refinement (R = 7, K = 20, epsilon 1e-3, max_shift 2, max_gradient 0.5), the search and the validation restated in numpy.

  python tools/subset_mask_table.py --numpy    the rows of the numpy restatement (tests/test_subset_masked_cpu.py), no device:
                                               writes profiles/subset_mask/table_numpy.md, the committed rows
  python tools/subset_mask_table.py            the device's rows (Context.subset_refine_masked) into OUT/table.md; they must equal
                                               the committed rows digit for digit, else exit status 1
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HEADER = ("| deformation | refinement | edge nodes | converged | mean endpoint error (px) | worst (px) | ux off, RMS, starts from the truth |\n|" +
          "---|" * 7 + "\n")
LABELS = (("plain", "as it is"), ("masked", "masked, usable rule, min_pixels 57"), ("own_pixel_only", "masked, own pixel only"))


def ux_rms(T, name, refine):
    """The RMS error of ux over the converged edge nodes when every node starts from the truth rounded to whole pixels: (plain,
    masked, own pixel only -- None from a device)."""
    c = T.SPECIMEN
    scene, mask, u0, _ = T.specimen_case(name)
    nh, nw = u0.shape
    cy, cx = c["r"] + np.arange(nh) * c["s"], c["r"] + np.arange(nw) * c["s"]
    su, sv = (np.rint(q[np.ix_(cy, cx)]).astype(np.float32) for q in (scene.gt_u, scene.gt_v))
    truth = np.gradient(scene.gt_u.astype(np.float64), axis=1)[np.ix_(cy, cx)]
    nv = T.usable_counts(mask, nw, nh, c["r"], c["s"], c["R"])
    edge = (mask[np.ix_(cy, cx)] < 0.5) & (nv < (2 * c["R"] + 1) ** 2)

    def run(which, stencil=True):
        if refine is not None:
            return refine(scene, which, su, sv)
        return T.subset_refine_masked_reference(scene.frame_0, scene.frame_1, su, sv, None, which, c["min_pixels"], c["r"], c["s"], c["R"],
                                                max_shift=c["max_shift"], stencil=stencil)

    out = []
    for got in (run(None), run(mask), run(mask, False) if refine is None else None):
        live = edge & (got.state >= 1) if got is not None else None
        out.append(float(np.sqrt(((got.ux[live].astype(np.float64) - truth[live]) ** 2).mean())) if got is not None and live.any() else None)
    return out


def lines(T, name, refine=None):
    rows, _ = T.specimen_rows(name, refine)
    rms = dict(zip(("plain", "masked", "own_pixel_only"), ux_rms(T, name, refine)))
    out = []
    for key, label in LABELS:
        if key in rows:
            q = rows[key]
            out.append("| %s | %s | %d | %d | %.4f | %.4f | %s |\n" % (name, label, q["edge"], q["converged"], q["mean_error"], q["worst_error"],
                                                                       "%.4f" % rms[key] if rms[key] is not None else ""))
    return out


def device_refine(T):
    """(refine, close): the device's counterpart of the restatement, as a test_subset_cpu.Refined."""
    flow2d = importlib.import_module("cuda-flow2d_amd")
    ctx = flow2d.Context(0)
    c = T.SPECIMEN

    def refine(scene, mask, u0, v0):
        h, w = scene.frame_0.shape
        nh, nw = u0.shape
        held = [ctx.plane(w, h, scene.frame_0), ctx.plane(w, h, scene.frame_1), ctx.plane(nw, nh, u0), ctx.plane(nw, nh, v0)]
        if mask is not None:
            held.append(ctx.plane(w, h, mask))
        try:
            u, v, gradients, score, state, rec = ctx.subset_refine_masked(held[0], held[1], w, h, held[2], held[3], None, nw, nh, c["r"], c["s"],
                                                                          c["R"], held[4] if mask is not None else None, c["min_pixels"],
                                                                          max_shift=c["max_shift"])
        finally:
            for q in held:
                q.free()
                ctx._planes.remove(q)
        out = T.Refined()
        for key, plane in zip(T.Refined.NAMES, (u, v) + gradients + (score, state)):
            setattr(out, key, plane)
        out.record = np.frombuffer(bytes(rec), T.SUBSET_DTYPE)
        return out

    return refine, ctx.close


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset_mask"))
    args = ap.parse_args()
    T = importlib.import_module("test_subset_masked_cpu")
    names = importlib.import_module("cuda-flow2d_amd.scenes").SPECKLE_DEFORMATIONS
    os.makedirs(args.out, exist_ok=True)
    committed = os.path.join(ROOT, "profiles", "subset_mask", "table_numpy.md")  # the restatement's rows, kept in the repository
    if args.numpy:
        rows = [q for name in names for q in lines(T, name)]
        with open(committed, "w") as f:
            f.write(HEADER)
            f.writelines(rows)
        print("%d rows -> %s" % (len(rows), committed))
        return 0
    refine, close = device_refine(T)
    try:
        got = [q for name in names for q in lines(T, name, refine)]
    finally:
        close()
    with open(os.path.join(args.out, "table.md"), "w") as f:
        f.write(HEADER)
        f.writelines(got)
    want = [q for q in open(committed).readlines()[2:] if "own pixel only" not in q]  # (the device has the header's rule only)
    differing = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
    print("%d device rows -> %s; %s" % (len(got), os.path.join(args.out, "table.md"),
                                        "equal to the committed restatement rows" if got == want else "rows %s DIFFER from %s" % (differing, committed)))
    return 0 if got == want else 1


if __name__ == "__main__":
    sys.exit(main())
