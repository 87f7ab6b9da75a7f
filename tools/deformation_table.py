#!/usr/bin/env python3
"""Accuracy of the deformation analysis on the analytic scenes (scenes.make_scene): rotation, zoom, affine and two_layer.

The scenes move by W(x) = A (x - c) + c + t, so the true values follow from A: divergence = tr(A) - 2, vorticity = A10 - A01,
dilatation = det(A) - 1; the Green-Lagrange strain of `rotation` is exactly zero and its small strain cos 3 deg - 1 on the
diagonal.  Per scene, source of the flow and quantity: the mean and RMS error over the valid pixels.  For two_layer, whose
background stands still and whose square moves rigidly, every true value is 0 away from the square's edge; the rows with and
without the occlusion mask show the ring of spurious strain the differences across that edge leave, and what the mask removes.

  python tools/deformation_table.py            every row; needs the GPU (flows, smoothing and analysis run on it)
  python tools/deformation_table.py --numpy    the ground-truth rows alone, through the numpy restatement
                                               (tests/test_deformation_cpu.py), no device
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
SMOOTHING = 2.0
PHI = np.radians(3.0)
MATRICES = {"rotation": [[np.cos(PHI), -np.sin(PHI)], [np.sin(PHI), np.cos(PHI)]], "zoom": [[1.03, 0.0], [0.0, 1.03]],
            "affine": [[1.02, 0.03], [-0.02, 0.985]], "two_layer": [[1.0, 0.0], [0.0, 1.0]]}
QUANTITIES = ("divergence", "vorticity", "dilatation", "exx", "eyy", "exy", "max_shear")


def truth(name, measure):
    """The true value of every quantity of the table for the scene's matrix."""
    a = np.asarray(MATRICES[name], np.float64)
    g = a - np.eye(2)
    e = 0.5 * (g + g.T) if measure == 0 else 0.5 * (a.T @ a - np.eye(2))
    shear = float(np.hypot(0.5 * (e[0, 0] - e[1, 1]), e[0, 1]))
    return {"divergence": g[0, 0] + g[1, 1], "vorticity": g[1, 0] - g[0, 1], "dilatation": float(np.linalg.det(a)) - 1.0,
            "exx": e[0, 0], "eyy": e[1, 1], "exy": e[0, 1], "max_shear": shear}


def rows_of(name, source, engine, measure, planes):
    want = truth(name, measure)
    out = []
    for q in QUANTITIES:
        x = planes[q].astype(np.float64)
        err = x[np.isfinite(x)] - want[q]
        out.append({"scene": name, "source": source, "engine": engine, "measure": ("small", "green")[measure], "quantity": q,
                    "true": want[q], "valid": int(err.size), "mean_error": float(err.mean()) if err.size else float("nan"),
                    "rms_error": float(np.sqrt((err * err).mean())) if err.size else float("nan")})
    return out


def numpy_rows(size, seed):
    ref = importlib.import_module("test_deformation_cpu").deformation_reference
    rows = []
    for name in MATRICES:
        sc = scenes.make_scene(name, size, size, seed)
        for measure in (0, 1):
            rows += rows_of(name, "true", "numpy", measure, ref(sc.gt_u, sc.gt_v, None, measure))
            if name == "two_layer" and sc.occlusion is not None:
                rows += rows_of(name, "true, occlusion mask", "numpy", measure, ref(sc.gt_u, sc.gt_v, np.asarray(sc.occlusion, np.float32), measure))
    return rows


def gpu_rows(size, seed):
    flow2d = importlib.import_module("cuda-flow2d_amd")
    rows = []
    with flow2d.Context(0) as ctx:
        flow = flow2d.OpticalFlow(size, size, flow2d.GREY, ctx=ctx)
        try:
            p = flow.params(*PARAMS)
            for name in MATRICES:
                sc = scenes.make_scene(name, size, size, seed)
                for measure in (0, 1):
                    got, _ = ctx.deformation(ctx.plane(size, size, sc.gt_u), ctx.plane(size, size, sc.gt_v), size, size, measure,
                                             stats=False)
                    rows += rows_of(name, "true", "gpu", measure, got)
                    for sigma in (0.0, SMOOTHING):
                        for masks in ((False, True) if name == "two_layer" else (False,)):
                            got, _ = flow.analyse_deformation(sc.frame_0, sc.frame_1, p, measure, sigma, masks)
                            source = "computed%s%s" % (", sigma %g" % sigma if sigma else "", ", occlusion mask" if masks else "")
                            rows += rows_of(name, source, "gpu", measure, got)
        finally:
            flow.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deformation"))
    args = ap.parse_args()
    rows = numpy_rows(args.size, args.seed)
    if not args.numpy:
        rows += gpu_rows(args.size, args.seed)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "table_numpy.md" if args.numpy else "table.md")
    with open(path, "w") as f:
        f.write("| scene | flow | engine | measure | quantity | true | valid | mean error | RMS error |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | %s | %s | %s | %s | %.6g | %d | %.3g | %.3g |\n" %
                    (r["scene"], r["source"], r["engine"], r["measure"], r["quantity"], r["true"], r["valid"], r["mean_error"],
                     r["rms_error"]))
    print("%d rows -> %s" % (len(rows), path))


if __name__ == "__main__":
    main()
