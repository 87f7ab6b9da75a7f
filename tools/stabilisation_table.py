#!/usr/bin/env python3
"""Accuracy of the global motion and of the stabilised frames on the analytic sequences (scenes.make_sequence).

Per scene and model, for every frame k >= 1 of a sequence stabilised against frame 0: the error of the composed parameters
M(0 -> k) against the scene's exact W^k (two_layer: against its static background, the identity) and the RMSE of frame k brought
back onto frame 0's grid against frame 0, over the pixels the warp covers -- with the true flows (source "true") and with the
flows the solver computes (Grey, and Grey with red-black SOR 1.9; sources "grey", "grey_sor").  The row of source "exact" is
the yardstick: the same warp along the exact W^k, whose RMSE is the bilinear sample's alone.

  python tools/stabilisation_table.py            every row; needs the GPU (the fit, the composition and the warp run on it)
  python tools/stabilisation_table.py --numpy    the true-flow rows alone, from the numpy restatements (tests/), no device
The true-flow rows of both engines are the same printed numbers (tests/test_gpu_global_motion.py).  Writes OUT/README.md.
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
MODEL_NAMES = ("translation", "similarity", "affine")
SIGMA, ITERATIONS, FILL = 0.5, 5, -1.0
PARAMS = (50, 0.9, 40, 5, 35.0, 0.001, 0.001, 5, 1.5)  # the CLI's defaults


def restatements():
    return importlib.import_module("test_global_motion_cpu")


def exact_step(seq):
    """The exact parameters of one step of the scene's global motion: W for the affine scenes, the static background (the
    identity) for two_layer."""
    return np.zeros(6) if seq.name == "two_layer" else restatements().true_motion(seq)


def rmse(a, b, where):
    d = (a.astype(np.float64) - b.astype(np.float64))[where]
    return float(np.sqrt(np.mean(d * d))) if d.size else float("nan")


class NumpyEngine:
    name = "numpy"

    def __init__(self):
        self.r = restatements()

    def fit(self, u, v, model):
        return self.r.global_motion_reference(u, v, None, model, SIGMA, ITERATIONS)["p"]

    def compose(self, first, second):
        return self.r.compose_motion(first, second)

    def warp(self, p, frame):
        return self.r.warp_global_reference(p, frame, FILL)

    def close(self):
        pass


class GpuEngine:
    name = "gpu"

    def __init__(self):
        self.flow2d = importlib.import_module("cuda-flow2d_amd")
        self.ctx = self.flow2d.Context(0)

    def fit(self, u, v, model):
        h, w = u.shape
        pu, pv = self.ctx.plane(w, h, u), self.ctx.plane(w, h, v)
        rec = self.ctx.global_motion(pu, pv, w, h, model, SIGMA, ITERATIONS)[0]
        for q in (pu, pv):
            q.free()
            self.ctx._planes.remove(q)
        return rec.parameters

    def compose(self, first, second):
        gm = self.flow2d.GlobalMotion.from_parameters
        return self.flow2d.compose_global_motion(gm(first), gm(second)).parameters

    def warp(self, p, frame):
        h, w = frame.shape
        pf, out, valid = self.ctx.plane(w, h, frame), self.ctx.plane(w, h), self.ctx.plane(w, h)
        motion = self.ctx.upload_motion([self.flow2d.GlobalMotion.from_parameters(p)])
        self.ctx.warp_global(motion, pf, w, h, out, valid, fill=FILL)
        got = out.download(), valid.download()
        for q in (pf, out, valid, motion):
            q.free()
            self.ctx._planes.remove(q)
        return got

    def close(self):
        self.ctx.close()


def rows_of(engine, seq, flows, source, models):
    """One row per model and frame k >= 1; flows[k] = (u, v) of frame k -> k + 1, or None for the yardstick."""
    step = exact_step(seq)
    rows = []
    for model in models:
        composed, exact = np.zeros(6), np.zeros(6)
        for k in range(1, seq.frame_count):
            exact = engine.compose(exact, step)
            composed = exact if flows is None else engine.compose(composed, engine.fit(flows[k - 1][0], flows[k - 1][1], model))
            # a parameter below 1e-12 is what is left of sums that cancel (a rotation or a zoom about the centre fitted by a
            # translation): its sign would decide whether the border row and column at coordinate 0 are covered
            composed = np.where(np.abs(composed) < 1e-12, 0.0, composed)
            out, valid = engine.warp(composed, seq.frames[k])
            rows.append({"scene": seq.name, "model": "exact" if flows is None else MODEL_NAMES[model], "source": source,
                         "engine": engine.name, "frame": k, "parameter_error": float(np.abs(composed - exact).max()),
                         "covered": float(valid.mean()), "rmse": rmse(out, seq.frames[0], valid == 1),
                         "rmse_unstabilised": rmse(seq.frames[k], seq.frames[0], valid == 1)})
        if flows is None:
            break
    return rows


def true_rows(use_numpy, size, seed, scene_names=scenes.SCENES, frame_count=5):
    engine = NumpyEngine() if use_numpy else GpuEngine()
    try:
        rows = []
        for name in scene_names:
            seq = scenes.make_sequence(name, frame_count, size, size, seed)
            rows += rows_of(engine, seq, None, "exact", (2,))
            rows += rows_of(engine, seq, [(seq.gt_u[k], seq.gt_v[k]) for k in range(frame_count - 1)], "true", (0, 1, 2))
        return rows
    finally:
        engine.close()


def computed_rows(size, seed, frame_count=5):
    flow2d = importlib.import_module("cuda-flow2d_amd")
    engine = GpuEngine()
    try:
        rows = []
        for source, extra in (("grey", {}), ("grey_sor", {"sor_omega": 1.9})):
            flow = flow2d.OpticalFlow(size, size, flow2d.GREY, ctx=engine.ctx)
            try:
                p = flow.params(*PARAMS, **extra)
                for name in scenes.SCENES:
                    seq = scenes.make_sequence(name, frame_count, size, size, seed)
                    flows = [flow.compute_flow(seq.frames[k], seq.frames[k + 1], p)[:2] for k in range(frame_count - 1)]
                    rows += rows_of(engine, seq, flows, source, (0, 1, 2))
            finally:
                flow.close()
        return rows
    finally:
        engine.close()


def format_row(r):
    return "| %-11s | %-11s | %-8s | %-5s | %d | %.2e | %5.1f | %8.4f | %8.4f |" % (
        r["scene"], r["model"], r["source"], r["engine"], r["frame"], r["parameter_error"], 100 * r["covered"], r["rmse"],
        r["rmse_unstabilised"])


HEADER = ("| scene | model | flows | engine | frame k | max error of M(0->k) | covered % | RMSE against frame 0 | unstabilised |\n"
          "|---|---|---|---|---|---|---|---|---|\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true", help="the true-flow rows alone, from the numpy restatements")
    ap.add_argument("--size", type=int, default=256, help="square frames of this side (default 256)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_motion"), help="where README.md goes")
    args = ap.parse_args()
    rows = true_rows(args.numpy, args.size, args.seed, scenes.SCENES, args.frames)
    if not args.numpy:
        rows += computed_rows(args.size, args.seed, args.frames)
    os.makedirs(args.out, exist_ok=True)
    name = "table_numpy.md" if args.numpy else "table.md"
    with open(os.path.join(args.out, name), "w") as f:
        f.write("Stabilisation against frame 0, %d x %d, seed %d, sigma %g px, %d reweighted passes (tools/stabilisation_table.py%s)\n\n"
                % (args.size, args.size, args.seed, SIGMA, ITERATIONS, " --numpy" if args.numpy else ""))
        f.write(HEADER)
        for r in rows:
            f.write(format_row(r) + "\n")
    for r in rows:
        print(format_row(r))


if __name__ == "__main__":
    main()
