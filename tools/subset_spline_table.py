#!/usr/bin/env python3
"""What the cubic B-spline sample of frame 1 gains the subset refinement over the Catmull-Rom one, on the same starts: three tables.
  1. The six scenes of tests/test_subset_cpu.py (96 x 80, grid r = 7, s = 8, R = 7, starts from the window search): mean and
     largest interior endpoint error, mean gradient error, mean iterations, Catmull-Rom and B-spline.
  2. The bending scenes at order 2 (tests/test_subset2_cpu.py): mean endpoint error over the scored nodes.
  3. The specimen scenes under their mask (tests/test_subset_masked_cpu.py, min_pixels 57): the edge nodes and the interior nodes.
The coefficients are those of flow2d_bspline_prefilter_2d, stored as fp32.

  python tools/subset_spline_table.py --numpy   the rows of the numpy restatement (tests/test_subset_spline_cpu.py), no device:
                                                writes profiles/subset_spline/table_numpy.md, the committed rows
  python tools/subset_spline_table.py           the device's rows (Context.bspline_prefilter, subset_refine_spline,
                                                subset_refine2_spline and their Catmull-Rom counterparts) into OUT/table.md; they
                                                must equal the committed rows digit for digit, else exit status 1
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HEAD1 = ("| scene | Catmull-Rom, mean / max EPE (px) | B-spline, mean / max EPE (px) | gradient error, mean | iterations, mean | converged |\n|" +
         "---|" * 6 + "\n")
HEAD2 = "| scene, order 2 | Catmull-Rom mean EPE (px) | B-spline mean EPE (px) | converged |\n|" + "---|" * 4 + "\n"
HEAD3 = ("| specimen | nodes | Catmull-Rom mean error (px) | B-spline mean error (px) |\n|" + "---|" * 4 + "\n")
SPECIMENS = ("stretch", "rotation", "shear")


class Device:
    """The device's counterparts of the restatement's refinements, as the restatement's result classes."""

    def __init__(self):
        self.flow2d = importlib.import_module("cuda-flow2d_amd")
        self.ctx = self.flow2d.Context(0)
        self.S1, self.S2 = importlib.import_module("test_subset_cpu"), importlib.import_module("test_subset2_cpu")

    def close(self):
        self.ctx.close()

    def _planes(self, f0, f1, u0, v0, spline, mask=None):
        h, w = f0.shape
        nh, nw = u0.shape
        held = [self.ctx.plane(w, h, f0), self.ctx.plane(w, h, f1), self.ctx.plane(nw, nh, u0), self.ctx.plane(nw, nh, v0)]
        if mask is not None:
            held.append(self.ctx.plane(w, h, mask))
        if spline:
            held.append(self.ctx.bspline_prefilter(held[1], w, h))
        return held, (held[-1] if spline else held[1]), (w, h, nw, nh)

    def _release(self, held):
        for q in held:
            q.free()
            self.ctx._planes.remove(q)

    def refine(self, f0, f1, u0, v0, r, s, R, spline, mask=None, min_pixels=None, max_shift=2.0):
        held, sampled, (w, h, nw, nh) = self._planes(f0, f1, u0, v0, spline, mask)
        try:
            call = self.ctx.subset_refine_spline if spline else self.ctx.subset_refine_masked
            u, v, gradients, score, state, rec = call(held[0], sampled, w, h, held[2], held[3], None, nw, nh, r, s, R,
                                                      held[4] if mask is not None else None, min_pixels, max_shift=max_shift)
        finally:
            self._release(held)
        out = self.S1.Refined()
        for key, plane in zip(self.S1.Refined.NAMES, (u, v) + gradients + (score, state)):
            setattr(out, key, plane)
        out.record = np.frombuffer(bytes(rec), self.S1.SUBSET_DTYPE)
        return out

    def refine2(self, f0, f1, u0, v0, r, s, R, spline):
        held, sampled, (w, h, nw, nh) = self._planes(f0, f1, u0, v0, spline)
        try:
            call = self.ctx.subset_refine2_spline if spline else self.ctx.subset_refine2
            u, v, gradients, curvatures, score, state, rec = call(held[0], sampled, w, h, held[2], held[3], nw, nh, r, s, R)
        finally:
            self._release(held)
        out = self.S2.Refined2()
        names = ("u", "v") + self.S2.GRADIENTS + self.S2.CURVATURES + ("score", "state")  # the entry's order
        for key, plane in zip(names, (u, v) + gradients + curvatures + (score, state)):
            setattr(out, key, plane)
        out.record = np.frombuffer(bytes(rec), self.S1.SUBSET_DTYPE)
        return out


def tables(device=None):
    T = importlib.import_module("test_subset_spline_cpu")
    S1, S2, SM = (importlib.import_module(m) for m in ("test_subset_cpu", "test_subset2_cpu", "test_subset_masked_cpu"))
    out = [HEAD1]
    for name, d in S1.SCENE_CASES:
        if device is None:
            a, b = S1.scene_rows(name, d), T.spline_scene_rows(name, d)
        else:
            a, b = (S1.scene_figures(name, d, lambda f0, f1, u0, v0, r, s, R, spline=spline: device.refine(f0, f1, u0, v0, r, s, R, spline))
                    for spline in (False, True))
        out.append("| %s | %.4f / %.4f | %.4f / %.4f | %.4f -> %.4f | %.2f -> %.2f | %d, %d of %d |\n" % (
            name, a["subset_mean_epe"], a["subset_max_epe"], b["subset_mean_epe"], b["subset_max_epe"], a["gradient_mean_error"],
            b["gradient_mean_error"], a["iterations_mean"], b["iterations_mean"], a["interior_converged"], b["interior_converged"], b["interior"]))
    out += ["\n", HEAD2]
    for name, R in T.SPLINE_BENDING_CASES:
        if device is None:
            a, b = S2.scene_rows(name, R), T.spline_scene_rows2(name, R)
        else:
            a, b = (S2.scene_figures(name, R, lambda f0, f1, u0, v0, r, s, R_, spline=spline: device.refine2(f0, f1, u0, v0, r, s, R_, spline))
                    for spline in (False, True))
        out.append("| %s, R %d | %.4f | %.4f | %d, %d of %d |\n" % (name, R, a["order2_mean_epe"], b["order2_mean_epe"], a["order2_converged"],
                                                                   b["order2_converged"], b["nodes"]))
    out += ["\n", HEAD3]
    c = SM.SPECIMEN
    for name in SPECIMENS:
        refine = None
        if device is not None:
            def refine(scene, mask, u0, v0, spline):
                return device.refine(scene.frame_0, scene.frame_1, u0, v0, c["r"], c["s"], c["R"], spline, mask, c["min_pixels"], c["max_shift"])
        rows = T.spline_specimen_rows(name, refine)
        a, b = rows["catmull_rom"], rows["bspline"]
        out.append("| %s, edge | %d | %.4f | %.4f |\n" % (name, b["edge"], a["edge_mean_error"], b["edge_mean_error"]))
        out.append("| %s, interior | %d | %.4f | %.4f |\n" % (name, b["interior"], a["interior_mean_error"], b["interior_mean_error"]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset_spline"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    committed = os.path.join(ROOT, "profiles", "subset_spline", "table_numpy.md")  # the restatement's rows, kept in the repository
    if args.numpy:
        rows = tables()
        with open(committed, "w") as f:
            f.writelines(rows)
        print("%d lines -> %s" % (len(rows), committed))
        return 0
    device = Device()
    try:
        got = tables(device)
    finally:
        device.close()
    with open(os.path.join(args.out, "table.md"), "w") as f:
        f.writelines(got)
    got, want = "".join(got).splitlines(), open(committed).read().splitlines()
    differing = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
    same = got == want
    print("%d device lines -> %s; %s" % (len(got), os.path.join(args.out, "table.md"),
                                         "equal to the committed restatement rows" if same else "lines %s DIFFER from %s" % (differing, committed)))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
