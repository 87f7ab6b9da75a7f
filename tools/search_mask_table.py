#!/usr/bin/env python3
"""What a region of interest gains the window search and the median test at a specimen's edge: scenes.make_speckle_specimen's plate
with a hole, 96 x 80, seed 0, grid r = 7, d = 10, s = 8, lo and scale from the frames' extremes, min_pixels 57.
Table 1, on the plate moved by (6.4, -3.3) in front of a static background of the specimen's own contrast: the on-specimen nodes
more than 1.5 px from the truth (a NaN among them) -- edge nodes (an excluded pixel in the window) and interior ones -- after the
search as it is (flow2d_correlate_offset_2d), after flow2d_validate_nodes_2d with replacement behind it, after the masked search
(flow2d_correlate_masked_2d), and after flow2d_validate_nodes_masked_2d behind that.
Table 2, on the moved plate and on the committed easy scene (moved by (1.6, -0.7), dim background): the whole chain -- search,
validation with replacement, the masked refinement (flow2d_subset_refine_masked_2d, R = 7, min_pixels 57, max_shift 2) -- without
and with the masked search in front (OpticalFlow2D::SubsetOptions::mask_search): converged nodes, mean and worst endpoint error
over them, for the edge and for the interior nodes.

  python tools/search_mask_table.py --numpy    the rows of the numpy restatement (tests/test_correlate_masked_cpu.py), no device:
                                               writes profiles/search_mask/table_numpy.md, the committed rows
  python tools/search_mask_table.py            the device's rows (Context.correlate_masked, validate_nodes_masked,
                                               subset_refine_masked) into OUT/table.md; they must equal the committed rows digit
                                               for digit, else exit status 1
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
NAMES = ("stretch", "rotation")
HEADER_1 = "| scene | step | edge nodes | edge nodes off by more than 1.5 px | interior nodes | interior nodes off |\n|" + "---|" * 6 + "\n"
HEADER_2 = ("| scene | search | nodes | kind | converged | mean endpoint error (px) | worst (px) |\n|" + "---|" * 7 + "\n")
STEPS = (("search", "search as it is"), ("search+validate", "... then the median test, REPLACE"), ("masked", "masked search"),
         ("masked+validate", "... then the masked median test"))


def lines(T, device=None):
    device = device or {}
    out = [HEADER_1]
    for name in NAMES:
        rows, edges, interior = T.claim_counts(name, **{k: device[k] for k in ("correlate", "validate", "correlate_masked", "validate_masked")
                                                       if k in device})
        for key, label in STEPS:
            out.append("| %s, moved | %s | %d | %d | %d | %d |\n" % (name, label, edges, rows[key][0], interior, rows[key][1]))
    out.append("\n")
    out.append(HEADER_2)
    for scene, args in (("moved", T.CLAIM_SCENE), ("easy", T.EASY_SCENE)):
        for name in NAMES:
            for mask_search in (False, True):
                q = T.chain_figures(name, args, mask_search, device.get("chain_correlate"), device.get("chain_validate"), device.get("refine"))
                for kind in ("edge", "interior"):
                    out.append("| %s, %s | %s | %d | %s | %d | %.4f | %.4f |\n" % (name, scene, "masked" if mask_search else "as it is", q[kind]["nodes"],
                                                                                 kind, q[kind]["converged"], q[kind]["mean"], q[kind]["worst"]))
    return out


def device_calls(T):
    """The device's counterparts of the restatements, and close()."""
    flow2d = importlib.import_module("cuda-flow2d_amd")
    S = importlib.import_module("test_subset_cpu")
    ctx = flow2d.Context(0)

    def planes(arrays):
        return [ctx.plane(a.shape[1], a.shape[0], np.ascontiguousarray(a, np.float32)) if a is not None else None for a in arrays]

    def drop(held):
        for q in held:
            if q is not None:
                q.free()
                ctx._planes.remove(q)

    def correlate_masked(f0, f1, lo, scale, r, d, s, mask, min_pixels):
        held = planes([f0, f1, mask])
        try:
            u, v, score, rec = ctx.correlate_masked(held[0], held[1], f0.shape[1], f0.shape[0], lo, scale, r, d, s, held[2], min_pixels)
        finally:
            drop(held)
        return u, v, score, rec

    def validate_masked(u, v, mask, r, s):
        nh, nw = u.shape
        held = planes([u, v, mask])
        try:
            h, w = mask.shape if mask is not None else (0, 0)
            return ctx.validate_nodes_masked(held[0], held[1], nw, nh, held[2], w, h, r, s)
        finally:
            drop(held)

    def refine(scene, mask, u0, v0):
        h, w = scene.frame_0.shape
        nh, nw = u0.shape
        r, d, s = T.CLAIM_GRID
        held = planes([scene.frame_0, scene.frame_1, u0, v0, mask])
        try:
            u, v, gradients, score, state, rec = ctx.subset_refine_masked(held[0], held[1], w, h, held[2], held[3], None, nw, nh, r, s,
                                                                          T.CHAIN_SUBSET["R"], held[4], T.CHAIN_SUBSET["min_pixels"],
                                                                          max_shift=T.CHAIN_SUBSET["max_shift"])
        finally:
            drop(held)
        out = S.Refined()
        out.u, out.v, out.state = u, v, state
        return out

    calls = dict(correlate=lambda f0, f1, lo, scale, r, d, s: correlate_masked(f0, f1, lo, scale, r, d, s, None, 0),
                 validate=lambda u, v: validate_masked(u, v, None, 0, 0), correlate_masked=correlate_masked, validate_masked=validate_masked,
                 chain_correlate=correlate_masked, chain_validate=validate_masked, refine=refine)
    return calls, ctx.close


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_mask"))
    args = ap.parse_args()
    T = importlib.import_module("test_correlate_masked_cpu")
    os.makedirs(args.out, exist_ok=True)
    committed = os.path.join(ROOT, "profiles", "search_mask", "table_numpy.md")  # the restatement's rows, kept in the repository
    if args.numpy:
        rows = lines(T)
        with open(committed, "w") as f:
            f.writelines(rows)
        print("%d lines -> %s" % (len(rows), committed))
        return 0
    calls, close = device_calls(T)
    try:
        got = lines(T, calls)
    finally:
        close()
    with open(os.path.join(args.out, "table.md"), "w") as f:
        f.writelines(got)
    got, want = "".join(got).splitlines(True), open(committed).readlines()
    differing = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
    same = got == want
    print("%d device lines -> %s; %s" % (len(got), os.path.join(args.out, "table.md"),
                                         "equal to the committed restatement rows" if same else "lines %s DIFFER from %s" % (differing, committed)))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
