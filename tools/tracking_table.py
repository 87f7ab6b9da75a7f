#!/usr/bin/env python3
"""Accuracy of dense point tracking (flow2d_seed_points_2d + flow2d_track_points_2d) on the analytic sequences of
cuda-flow2d_amd/scenes.py (make_sequence): every scene x {true flows, true flows without the boundary test, computed flows for
Grey, Gradient and Grey with red-black SOR (omega 1.9)}.  Tracks are seeded on frame 0 and every later frame (spacing 4, the
default texture threshold) and carried with the paper's thresholds (alpha 0.01 / 0.5, beta 0.01 / 0.002).  Per row:
  alive        tracks alive in the last frame, and how many of the frame-0 seeds are among them
  median, p95  position error (px) of the tracks alive in the last frame against the scene's trajectory()
  precision    terminations whose point is truly lost (not visible) in that frame or the next, over all terminations
  recall       points truly lost (visible in frame k-1, not in frame k) whose track ends in frame k or k+1, over all such;
               r_occ counts only the ends with reason OCCLUDED (two_layer: the background the square covers)

Default: the product on the GPU -- OpticalFlow.compute_flow_bidirectional for the computed flows, Context.seed_points /
Context.track_points for every step.  --numpy runs the same table on the CPU: oracle.compute_flow in both directions and the
numpy restatement of both kernels (tests/test_tracking_cpu.py; bit-identical to the kernels).

    python tools/tracking_table.py [--numpy] [--size 256] [--frames 10] [--seed 0] [--json FILE]

Flow parameters: the CLI's defaults (50 levels at 0.9, 40 x 5 sweeps, alpha 35, median 5, sigma 1.5)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

flow2d = importlib.import_module("cuda-flow2d_amd")
scenes = importlib.import_module("cuda-flow2d_amd.scenes")

PARAMS = (50, 0.9, 40, 5, 35.0, 0.001, 0.001, 5, 1.5)
MODES = (("true", None, 0.0, True), ("true_no_boundaries", None, 0.0, False), ("grey", flow2d.GREY, 0.0, True),
         ("gradient", flow2d.GRADIENT, 0.0, True), ("grey_sor1.9", flow2d.GREY, 1.9, True))
SPACING = 4
F32 = np.float32


def computed_flows(q, constancy, omega, use_numpy):
    """[u, v, back_u, back_v] lists over the pairs of q."""
    n, h, w = q.frames.shape
    out = [[], [], [], []]
    if use_numpy:
        from oracle import oracle as O
        for k in range(n - 1):
            u, v, _ = O.compute_flow(q.frames[k], q.frames[k + 1], *PARAMS, constancy, sor_omega=omega)
            bu, bv, _ = O.compute_flow(q.frames[k + 1], q.frames[k], *PARAMS, constancy, sor_omega=omega)
            for lst, a in zip(out, (u, v, bu, bv)):
                lst.append(a)
        return out
    flow = flow2d.OpticalFlow(w, h, constancy)
    try:
        p = flow.params(*PARAMS, sor_omega=omega)
        for k in range(n - 1):
            for lst, a in zip(out, flow.compute_flow_bidirectional(q.frames[k], q.frames[k + 1], p)[:4]):
                lst.append(a)
    finally:
        flow.close()
    return out


class Tracker:
    """Seeding and tracking through the kernels (GPU) or their numpy restatement."""

    def __init__(self, use_numpy):
        self.use_numpy = use_numpy
        if not use_numpy:
            self.ctx = flow2d.Context(0)

    def __call__(self, frames, flows, boundaries):
        """Tables [n, cap], reasons [n, cap] (of the step into frame k; 1 in frame 0) and the counts after each frame."""
        n, h, w = frames.shape
        cap = n * (-(-w // SPACING)) * (-(-h // SPACING))
        eig = flow2d.DEFAULT_MIN_EIGENVALUE
        xs = np.full((n, cap), np.nan, F32)
        ys = np.full((n, cap), np.nan, F32)
        rs = np.ones((n, cap), np.uint8)
        if self.use_numpy:
            from test_tracking_cpu import seed_reference, track_reference
            xs[0], ys[0], count, _ = seed_reference(frames[0], SPACING, eig, xs[0], ys[0], 0)
            counts = [count]
            for k in range(n - 1):
                xs[k + 1], ys[k + 1], rs[k + 1] = track_reference(flows[0][k], flows[1][k], flows[2][k], flows[3][k], xs[k], ys[k],
                                                                  count, boundaries=boundaries)
                xs[k + 1], ys[k + 1], count, _ = seed_reference(frames[k + 1], SPACING, eig, xs[k + 1], ys[k + 1], count)
                counts.append(count)
            return xs, ys, rs, counts
        ctx = self.ctx
        made = []

        def plane(w_, h_, data=None):
            p = ctx.plane(w_, h_, data)
            made.append(p)
            return p

        tx = [plane(cap, 1) for _ in range(n)]
        ty = [plane(cap, 1) for _ in range(n)]
        reasons = [plane(cap // 4 + 4, 1) for _ in range(n)]
        tx[0].fill_bytes(0xFF)
        ty[0].fill_bytes(0xFF)
        cnt = ctx.counter(0)
        made.append(cnt)
        fr = [plane(w, h, f) for f in frames]
        fl = [[plane(w, h, a) for a in lst] for lst in flows]
        ctx.seed_points(fr[0], w, h, SPACING, tx[0], ty[0], cnt, cap, eig)
        counts = [ctx.read_count(cnt)]
        for k in range(n - 1):
            ctx.track_points(fl[0][k], fl[1][k], fl[2][k], fl[3][k], w, h, tx[k], ty[k], cnt, cap, tx[k + 1], ty[k + 1],
                             reasons[k + 1], boundaries=boundaries)
            ctx.seed_points(fr[k + 1], w, h, SPACING, tx[k + 1], ty[k + 1], cnt, cap, eig)
            counts.append(ctx.read_count(cnt))
        for k in range(n):
            xs[k], ys[k] = tx[k].download(cap, 1)[0], ty[k].download(cap, 1)[0]
            if k:
                rs[k] = reasons[k].download(cap // 4 + 4, 1).view(np.uint8).ravel()[:cap]
        for p in made:
            p.free()
            ctx._planes.remove(p)
        return xs, ys, rs, counts

    def close(self):
        if not self.use_numpy:
            self.ctx.close()


def score(q, xs, ys, rs, counts):
    n = q.frames.shape[0]
    m = counts[-1]
    xs, ys, rs = xs[:, :m], ys[:, :m], rs[:, :m]
    alive = ~np.isnan(xs)
    first = np.where(alive.any(0), alive.argmax(0), -1)
    x0 = np.array([xs[f, i] if f >= 0 else np.nan for i, f in enumerate(first)], np.float64)
    y0 = np.array([ys[f, i] if f >= 0 else np.nan for i, f in enumerate(first)], np.float64)
    errors = []
    vis = np.zeros((n, m), bool)  # the true visibility of every track's point in every frame from its start on
    for start in np.unique(first[first >= 0]):
        pick = first == start
        for k in range(start, n):
            vis[k, pick] = q.visible(x0[pick], y0[pick], k, start=start)
        tx, ty = q.trajectory(x0[pick], y0[pick], n - 1, start=start)
        last = alive[n - 1, pick]
        errors.append(np.hypot(xs[n - 1, pick][last] - tx[last], ys[n - 1, pick][last] - ty[last]))
    err = np.concatenate(errors) if errors else np.zeros(0)
    ends = correct = lost = found = found_occ = 0
    for k in range(1, n):
        ended = alive[k - 1] & ~alive[k]
        truly = ~vis[k] | (~vis[k + 1] if k + 1 < n else False)
        ends += int(ended.sum())
        correct += int((ended & truly).sum())
        gone = alive[k - 1] & vis[k - 1] & ~vis[k]
        ends_next = alive[k] & ~alive[k + 1] if k + 1 < n else np.zeros(m, bool)
        occ_now = ~alive[k] & (rs[k] == 4)
        occ_next = ends_next & (rs[k + 1] == 4) if k + 1 < n else np.zeros(m, bool)
        lost += int(gone.sum())
        found += int((gone & (~alive[k] | ends_next)).sum())
        found_occ += int((gone & (occ_now | occ_next)).sum())
    return {"alive": int(alive[n - 1].sum()), "alive_from_0": int(alive[n - 1, :counts[0]].sum()), "seeds_0": int(counts[0]),
            "tracks": int(m), "median_px": float(np.median(err)) if err.size else None,
            "p95_px": float(np.percentile(err, 95)) if err.size else None, "terminations": ends,
            "precision": correct / ends if ends else None, "lost": lost, "recall": found / lost if lost else None,
            "recall_occ": found_occ / lost if lost else None}


def fmt(v, spec):
    return "-" if v is None else spec % v


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true", help="the CPU oracle and the numpy restatement instead of the GPU")
    ap.add_argument("--size", type=int, default=256, help="square frames of this side (default 256)")
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", help="also write one JSON object per row to this file")
    args = ap.parse_args()
    if not args.numpy and flow2d.device_count() < 1:
        sys.exit("no HIP device: the GPU table needs the MI355X (--numpy runs it on the CPU)")
    n = args.size
    print("# %s, %dx%d, %d frames, seed %d, spacing %d, min eigenvalue %g; flows: CLI defaults" %
          ("numpy restatement + CPU oracle" if args.numpy else "GPU", n, n, args.frames, args.seed, SPACING,
           flow2d.DEFAULT_MIN_EIGENVALUE))
    print("%-12s %-18s %6s %11s %9s %9s %6s %6s %6s %6s %6s" % ("scene", "flows", "alive", "from 0", "median", "p95", "ends",
                                                               "prec", "lost", "recall", "r_occ"))
    rows = []
    tracker = Tracker(args.numpy)
    try:
        for name in scenes.SCENES:
            q = scenes.make_sequence(name, args.frames, n, n, args.seed)
            truth = [list(q.gt_u), list(q.gt_v), list(q.gt_back_u), list(q.gt_back_v)]
            for mode, constancy, omega, boundaries in MODES:
                flows = truth if constancy is None else computed_flows(q, constancy, omega, args.numpy)
                r = score(q, *tracker(q.frames, flows, boundaries))
                print("%-12s %-18s %6d %5d/%5d %9s %9s %6d %6s %6d %6s %6s" % (
                    name, mode, r["alive"], r["alive_from_0"], r["seeds_0"], fmt(r["median_px"], "%.4f"), fmt(r["p95_px"], "%.4f"),
                    r["terminations"], fmt(r["precision"], "%.3f"), r["lost"], fmt(r["recall"], "%.3f"),
                    fmt(r["recall_occ"], "%.3f")))
                rows.append(dict({"scene": name, "flows": mode, "size": n, "frames": args.frames, "seed": args.seed,
                                  "source": "numpy" if args.numpy else "gpu"}, **r))
    finally:
        tracker.close()
    if args.json:
        with open(args.json, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
