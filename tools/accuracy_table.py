#!/usr/bin/env python3
"""Accuracy of the flow against analytic ground truth: the scenes of cuda-flow2d_amd/scenes.py crossed with the data terms
Grey, Gradient, GradientUntiled, LogDerivatives and Grey with red-black SOR (omega 1.9).

Default: the product on the GPU -- OpticalFlow.compute_flow (compute_flow_bidirectional where the scene has an occlusion map)
and evaluate_flow (flow2d_flow_error_2d) -- one row per scene and mode with EPE / AE / R1 / Fl over all pixels, and over noc /
occ where the scene has an occlusion map; there also the precision and recall of flow2d_consistency_2d's mask against the
exact map.  --oracle runs the same table through oracle.compute_flow on the CPU (bit-identical to the product for Grey,
Gradient and GradientUntiled; LogDerivatives within 2e-6 per sweep, libm logf) with the metrics and the mask restated in numpy,
so thresholds can be set and the table rehearsed without a GPU.

    python tools/accuracy_table.py [--oracle] [--size 256] [--seed 0] [--json FILE]

Parameters: the CLI's defaults (50 levels at 0.9, 40 x 5 sweeps, alpha 35, median 5, sigma 1.5)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

flow2d = importlib.import_module("cuda-flow2d_amd")
scenes = importlib.import_module("cuda-flow2d_amd.scenes")

PARAMS = (50, 0.9, 40, 5, 35.0, 0.001, 0.001, 5, 1.5)  # levels, scale, outer, inner, alpha, e_smooth, e_data, median, sigma
MODES = (("grey", flow2d.GREY, 0.0), ("gradient", flow2d.GRADIENT, 0.0), ("gradient_untiled", flow2d.GRADIENT_UNTILED, 0.0),
         ("log_derivatives", flow2d.LOG_DERIVATIVES, 0.0), ("grey_sor1.9", flow2d.GREY, 1.9))
F32 = np.float32


def numpy_metrics(u, v, gt_u, gt_v, occlusion=None):
    """EPE / AE (degrees) / R1 / Fl per class, restated in numpy (the scenes' ground truth is finite everywhere)."""
    u, v, gu, gv = (np.asarray(a, F32) for a in (u, v, gt_u, gt_v))
    du, dv = u - gu, v - gv
    epe = np.sqrt(du * du + dv * dv).astype(np.float64)
    a = np.stack([u, v, np.ones_like(u)], -1).astype(np.float64)
    b = np.stack([gu, gv, np.ones_like(gu)], -1).astype(np.float64)
    ae = np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1)))
    gmag = np.sqrt(gu * gu + gv * gv).astype(np.float64)
    finite = np.isfinite(u) & np.isfinite(v)
    occ = np.zeros(u.shape, bool) if occlusion is None else np.asarray(occlusion) != 0
    out = {}
    for name, sel in (("all", finite), ("noc", finite & ~occ), ("occ", finite & occ)):
        n = int(sel.sum())
        e = epe[sel]
        out[name] = {"count": n, "epe": e.mean() if n else None, "ae": ae[sel].mean() if n else None,
                     "r1": (e > 1).mean() if n else None, "fl": ((e > 3) & (e > 0.05 * gmag[sel])).mean() if n else None}
    return out


def consistency_mask(u0, v0, u1, v1, alpha1=0.01, alpha2=0.5):
    """flow2d_consistency_2d's definition (include/flow2d_c_abi.h) in numpy fp32: 1 where forward and backward disagree."""
    h, w = u0.shape
    ys, xs = np.mgrid[0:h, 0:w]
    xf, yf = xs.astype(F32) + u0, ys.astype(F32) + v0
    with np.errstate(invalid="ignore", over="ignore"):
        inside = (xf >= 0) & (xf <= F32(w - 1)) & (yf >= 0) & (yf <= F32(h - 1))
        xf, yf = np.where(inside, xf, F32(0)), np.where(inside, yf, F32(0))
        xi, yi = np.floor(xf).astype(np.int64), np.floor(yf).astype(np.int64)
        dx, dy = xf - xi.astype(F32), yf - yi.astype(F32)
        x1, y1 = np.minimum(w - 1, xi + 1), np.minimum(h - 1, yi + 1)
        one = F32(1)

        def sample(p):
            return (one - dx) * (one - dy) * p[yi, xi] + dx * (one - dy) * p[yi, x1] + (one - dx) * dy * p[y1, xi] + dx * dy * p[y1, x1]

        bu, bv = sample(u1), sample(v1)
        eu, ev = u0 + bu, v0 + bv
        ok = inside & (eu * eu + ev * ev <= F32(alpha1) * ((u0 * u0 + v0 * v0) + (bu * bu + bv * bv)) + F32(alpha2))
    return np.where(ok, F32(0), F32(1))


def gpu_metrics(u, v, s):
    m = flow2d.flow_error_metrics(flow2d.evaluate_flow(u, v, s.gt_u, s.gt_v, occlusion=s.occlusion))
    return {k: {q: m[k][q] for q in ("count", "epe", "ae", "r1", "fl")} for k in flow2d.FLOW_ERROR_CLASSES}


def run_case(s, constancy, omega, use_oracle):
    h, w = s.shape
    mask = None
    if use_oracle:
        from oracle import oracle as O
        u, v, _ = O.compute_flow(s.frame_0, s.frame_1, *PARAMS, constancy, sor_omega=omega)
        if s.occlusion is not None:
            bu, bv, _ = O.compute_flow(s.frame_1, s.frame_0, *PARAMS, constancy, sor_omega=omega)
            mask = consistency_mask(u, v, bu, bv)
        return numpy_metrics(u, v, s.gt_u, s.gt_v, s.occlusion), mask
    flow = flow2d.OpticalFlow(w, h, constancy)
    try:
        p = flow.params(*PARAMS, sor_omega=omega)
        if s.occlusion is not None:
            u, v, _, _, mask, _, _ = flow.compute_flow_bidirectional(s.frame_0, s.frame_1, p)
        else:
            u, v, _ = flow.compute_flow(s.frame_0, s.frame_1, p)
    finally:
        flow.close()
    return gpu_metrics(u, v, s), mask


def fmt(x, spec):
    return "-" if x is None else format(x, spec)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--oracle", action="store_true", help="the CPU oracle and numpy metrics instead of the GPU")
    ap.add_argument("--size", type=int, default=256, help="square frames of this side (default 256)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", help="also write one JSON object per row to this file")
    args = ap.parse_args()
    if not args.oracle and flow2d.device_count() < 1:
        sys.exit("no HIP device: the GPU table needs the MI355X (--oracle runs it on the CPU)")
    rows = []
    print("# %s, %dx%d, seed %d; CLI defaults: %d levels x %.1f, %d x %d sweeps, alpha %.0f, median %d, sigma %.1f" %
          ("CPU oracle" if args.oracle else "GPU", args.size, args.size, args.seed, PARAMS[0], PARAMS[1], PARAMS[2],
           PARAMS[3], PARAMS[4], PARAMS[7], PARAMS[8]))
    print("%-12s %-17s %-4s %8s %8s %8s %8s %8s   %s" % ("scene", "mode", "cls", "pixels", "EPE", "AE(deg)", "R1", "Fl",
                                                        "mask precision / recall"))
    for name in scenes.SCENES:
        s = scenes.make_scene(name, args.size, args.size, args.seed)
        for mode, constancy, omega in MODES:
            m, mask = run_case(s, constancy, omega, args.oracle)
            pr = None
            if mask is not None:
                occ = s.occlusion != 0
                hit = float((occ & (mask != 0)).sum())
                pr = (hit / max(1.0, float((mask != 0).sum())), hit / max(1.0, float(occ.sum())))
            classes = ("all", "noc", "occ") if s.occlusion is not None else ("all",)
            for cls in classes:
                c = m[cls]
                tail = "%.3f / %.3f" % pr if (pr and cls == "all") else ""
                print("%-12s %-17s %-4s %8d %8s %8s %8s %8s   %s" % (name, mode, cls, c["count"], fmt(c["epe"], ".4f"),
                                                                   fmt(c["ae"], ".3f"), fmt(c["r1"], ".4f"), fmt(c["fl"], ".4f"),
                                                                   tail))
            rows.append({"scene": name, "mode": mode, "size": args.size, "seed": args.seed,
                         "source": "oracle" if args.oracle else "gpu", "metrics": m,
                         "mask_precision": pr[0] if pr else None, "mask_recall": pr[1] if pr else None})
    if args.json:
        with open(args.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
