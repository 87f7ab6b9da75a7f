#!/usr/bin/env python3
"""Accuracy of frame interpolation (flow2d_interpolate_2d) against the exact intermediate frames of the analytic scenes of
cuda-flow2d_amd/scenes.py: every scene x t in {0.25, 0.5, 0.75} x {true flows and masks, computed flows and masks, computed flows
without masks, plain blend} x K in {1, 2, 4} fixed-point iterations (max_residual 0.5).  Per row the RMS error in grey levels
(Middlebury's interpolation error, IE) and the count of pixels off by more than 5 grey levels, both leaving out an 8-pixel
border.

Default: the product on the GPU -- OpticalFlow.compute_flow_bidirectional for the computed flows and masks, Context.interpolate
for every row.  --numpy runs the same table on the CPU: oracle.compute_flow in both directions, the consistency mask and the
interpolation restated in numpy (tests/test_interpolation_cpu.py; bit-identical to the kernel).

    python tools/interpolation_table.py [--numpy] [--size 256] [--seed 0] [--json FILE]

Flow parameters: the CLI's defaults (50 levels at 0.9, 40 x 5 sweeps, alpha 35, median 5, sigma 1.5)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

flow2d = importlib.import_module("cuda-flow2d_amd")
scenes = importlib.import_module("cuda-flow2d_amd.scenes")

PARAMS = (50, 0.9, 40, 5, 35.0, 0.001, 0.001, 5, 1.5)
TIMES = (0.25, 0.5, 0.75)
ITERATIONS = (1, 2, 4)
MODES = ("true", "computed", "computed_no_masks", "blend")
BORDER = 8
MAX_RESIDUAL = 0.5
F32 = np.float32


def flows_of(s, use_numpy):
    """(u, v, back_u, back_v, occlusion_0, occlusion_1) computed from the scene's frames."""
    if use_numpy:
        from oracle import oracle as O
        from accuracy_table import consistency_mask
        u, v, _ = O.compute_flow(s.frame_0, s.frame_1, *PARAMS, flow2d.GREY)
        bu, bv, _ = O.compute_flow(s.frame_1, s.frame_0, *PARAMS, flow2d.GREY)
        return u, v, bu, bv, consistency_mask(u, v, bu, bv), consistency_mask(bu, bv, u, v)
    h, w = s.shape
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY)
    try:
        return flow.compute_flow_bidirectional(s.frame_0, s.frame_1, flow.params(*PARAMS))[:6]
    finally:
        flow.close()


class Interpolator:
    def __init__(self, use_numpy, w, h):
        self.use_numpy = use_numpy
        if not use_numpy:
            self.ctx = flow2d.Context(0)
            self.planes = [self.ctx.plane(w, h) for _ in range(9)]

    def __call__(self, frames, flows, masks, t, k):
        if self.use_numpy:
            from test_interpolation_cpu import interpolation_reference
            return interpolation_reference(*frames, *flows, t, masks[0], masks[1], k, MAX_RESIDUAL)
        p = self.planes
        for plane, a in zip(p, list(frames) + list(flows)):
            plane.upload(a)
        occ = [None, None]
        if masks[0] is not None:
            occ = [p[6].upload(masks[0]), p[7].upload(masks[1])]
        h, w = frames[0].shape
        self.ctx.interpolate(*p[:6], w, h, t, p[8], occ[0], occ[1], k, MAX_RESIDUAL)
        self.ctx.synchronize()
        return p[8].download()

    def close(self):
        if not self.use_numpy:
            self.ctx.close()


def score(out, truth):
    e = (out.astype(np.float64) - truth.astype(np.float64))[BORDER:-BORDER, BORDER:-BORDER]
    return float(np.sqrt((e * e).mean())), int((np.abs(e) > 5).sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true", help="the CPU oracle and the numpy restatement instead of the GPU")
    ap.add_argument("--size", type=int, default=256, help="square frames of this side (default 256)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", help="also write one JSON object per row to this file")
    args = ap.parse_args()
    if not args.numpy and flow2d.device_count() < 1:
        sys.exit("no HIP device: the GPU table needs the MI355X (--numpy runs it on the CPU)")
    n = args.size
    print("# %s, %dx%d, seed %d, max_residual %.1f, border %d px; flows: CLI defaults" %
          ("numpy restatement + CPU oracle" if args.numpy else "GPU", n, n, args.seed, MAX_RESIDUAL, BORDER))
    print("%-12s %5s %-18s %2s %9s %8s" % ("scene", "t", "mode", "K", "RMS", ">5 grey"))
    rows = []
    interp = Interpolator(args.numpy, n, n)
    try:
        for name in scenes.SCENES:
            s = scenes.make_scene(name, n, n, args.seed)
            zero = np.zeros(s.shape, F32)
            true_masks = (zero if s.occlusion is None else s.occlusion, zero if s.occlusion_1 is None else s.occlusion_1)
            computed = flows_of(s, args.numpy)
            cases = {"true": ((s.gt_u, s.gt_v, s.gt_back_u, s.gt_back_v), true_masks),
                     "computed": (computed[:4], computed[4:]),
                     "computed_no_masks": (computed[:4], (None, None))}
            for t in TIMES:
                truth = s.frame_at_time(t)
                for mode in MODES:
                    for k in ITERATIONS if mode != "blend" else (None,):
                        if mode == "blend":
                            out = (F32(1) - F32(t)) * s.frame_0 + F32(t) * s.frame_1
                        else:
                            out = interp((s.frame_0, s.frame_1), cases[mode][0], cases[mode][1], t, k)
                        e, bad = score(out, truth)
                        print("%-12s %5.2f %-18s %2s %9.4f %8d" % (name, t, mode, "-" if k is None else k, e, bad))
                        rows.append({"scene": name, "t": t, "mode": mode, "iterations": k, "size": n, "seed": args.seed,
                                     "source": "numpy" if args.numpy else "gpu", "rms": e, "above_5": bad})
    finally:
        interp.close()
    if args.json:
        with open(args.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
