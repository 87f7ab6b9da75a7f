#!/usr/bin/env python3
"""What warm-starting a sequence from the previous pair's flow gives: per sequence, data term (Grey, Gradient) and pair the mean
endpoint error over the whole frame of the unseeded flow, of the warm chain at reach 1 and 2 (every pair after the first seeded with
the propagated flow before it) and of the adaptive chain at each --tail, with the levels a pair ran, the error of the prior it ran
from and, for the adaptive chains, how the pair ended (unseeded / seeded / redone) -- on scenes.make_sequence("two_layer") and the
three scenes.make_speckle_sequence motions, the large translation of (11.25, -7.5) per frame among them, FRAMES frames, the CLI's
default parameters, four fill passes, photometric scale 1.

The numpy/oracle rows -- tests/test_propagate_cpu.py's restatement of the propagation, tests/test_prior_cpu.py's of the pyramid
from a prior over the oracle's stages, and the adaptive rule restated here -- are always computed; the GPU rows
(OpticalFlow.compute_flow_sequence_warm) where a device is present, or never with --numpy.
Writes OUT/table.md, or OUT/table_numpy.md when there are no GPU rows.

  python tools/warmstart_table.py [--numpy] [--frames 4] [--tail 0.05 0.005] [--out profiles/warmstart]
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
FILL, PHOTO = 4, 1.0
TERMS = (("Grey", 0), ("Gradient", 1))
MODES = ("unseeded", "seeded", "redone")


def sequences(frames, width, height):
    yield scenes.make_sequence("two_layer", frames, width, height, seed=0)
    for motion in scenes.SPECKLE_MOTIONS:
        yield scenes.make_speckle_sequence(motion, frames, width, height, seed=0)


def epe(u, v, gt_u, gt_v):
    ok = np.isfinite(u) & np.isfinite(v)
    return float(np.hypot(np.where(ok, u, 0) - gt_u, np.where(ok, v, 0) - gt_v).mean())


def next_reach(u, v, pu, pv, tail, used):
    """OpticalFlow2D::WarmNextReach over the record flow2d_flow_error_2d gives with the prior as ground truth: (redo, next)."""
    ok = np.isfinite(pu) & np.isfinite(pv)
    du, dv = (u - pu)[ok].astype(np.float32), (v - pv)[ok].astype(np.float32)
    err = np.sqrt(du * du + dv * dv)
    count = int(ok.sum())
    holds = [count > 0 and float((err > t).sum()) / count <= tail for t in (1, 2, 3)]
    return used > 0 and not holds[used - 1], next((t for t in (1, 2, 3) if holds[t - 1]), 0)


def oracle_rows(seq, term, constancy, tails):
    T, P = importlib.import_module("test_prior_cpu"), importlib.import_module("test_propagate_cpu")
    from oracle import oracle as O
    O.build()
    w, h, n = seq.width, seq.height, seq.frame_count
    plain = [O.compute_flow(seq.frames[k], seq.frames[k + 1], *PARAMS, constancy)[:2] for k in range(n - 1)]
    top = min(PARAMS[0], O.max_warp_level(w, h, PARAMS[1]))
    chains = {}
    for name in ["reach 1", "reach 2"] + ["tail %g" % t for t in tails]:
        tail = float(name.split()[1]) if name.startswith("tail") else None
        reach = 2 if tail is not None else int(name.split()[1])
        flows, cells = [plain[0]], [dict(mode=0, levels=top, prior=None)]
        for k in range(1, n - 1):
            pu, pv, _ = P.propagate_reference(*flows[k - 1], frame_from=seq.frames[k - 1], frame_to=seq.frames[k], photo_scale=PHOTO, fill_passes=FILL)
            cell = dict(prior=epe(pu, pv, seq.gt_u[k], seq.gt_v[k]))
            if reach > 0:
                start = T.start_level(w, h, PARAMS[0], PARAMS[1], float(reach))
                u, v, _ = T.compute_flow_from_prior(O, seq.frames[k], seq.frames[k + 1], pu, pv, *PARAMS, constancy, start)
                cell.update(mode=1, levels=start + 1)
            else:
                u, v = plain[k]
                cell.update(mode=0, levels=top)
            if tail is not None:
                redo, reach = next_reach(u, v, pu, pv, tail, reach if cell["mode"] else 0)
                if redo:
                    u, v = plain[k]
                    cell.update(mode=2, levels=cell["levels"] + top)
                    _, reach = next_reach(u, v, pu, pv, tail, 0)
            flows.append((u, v))
            cells.append(cell)
        chains[name] = (flows, cells)
    rows = []
    for k in range(n - 1):
        row = {"scene": seq.name, "term": term, "engine": "oracle", "pair": k, "unseeded": epe(*plain[k], seq.gt_u[k], seq.gt_v[k]), "chains": {}}
        for name, (flows, cells) in chains.items():
            row["chains"][name] = dict(cells[k], epe=epe(*flows[k], seq.gt_u[k], seq.gt_v[k]))
        rows.append(row)
    return rows


def gpu_rows(flow2d, ctx, seq, term, constancy, tails):
    flow = flow2d.OpticalFlow(seq.width, seq.height, constancy, ctx=ctx)
    n = seq.frame_count
    top = min(PARAMS[0], flow2d.max_warp_level(seq.width, seq.height, PARAMS[1]))
    try:
        p = flow.params(*PARAMS)
        plain = [flow.compute_flow(seq.frames[k], seq.frames[k + 1], p)[:2] for k in range(n - 1)]
        rows = [{"scene": seq.name, "term": term, "engine": "gpu", "pair": k, "unseeded": epe(*plain[k], seq.gt_u[k], seq.gt_v[k]), "chains": {}}
                for k in range(n - 1)]
        for name in ["reach 1", "reach 2"] + ["tail %g" % t for t in tails]:
            tail = float(name.split()[1]) if name.startswith("tail") else None
            us, vs, reports, _ = flow.compute_flow_sequence_warm(seq.frames, p, reach=2.0 if tail is not None else float(name.split()[1]),
                                                                 fill_passes=FILL, photo_scale=PHOTO, tail=tail)
            for k, r in enumerate(reports):
                levels = {0: top, 1: r.levels_run, 2: r.levels_run + top}[r.mode]
                rows[k]["chains"][name] = dict(mode=r.mode, levels=levels, prior=None, epe=epe(us[k], vs[k], seq.gt_u[k], seq.gt_v[k]))
        return rows
    finally:
        flow.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true", help="the numpy/oracle rows alone")
    ap.add_argument("--width", type=int, default=96)
    ap.add_argument("--height", type=int, default=80)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--tail", type=float, nargs="*", default=[0.05, 0.005])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warmstart"))
    args = ap.parse_args()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    with_gpu = not args.numpy and flow2d.device_count() > 0
    rows = []
    for seq in sequences(args.frames, args.width, args.height):
        for term, constancy in TERMS:
            rows += oracle_rows(seq, term, constancy, args.tail)
            print("%s, %s: oracle rows done" % (seq.name, term), flush=True)
    if with_gpu:
        with flow2d.Context(0) as ctx:
            for seq in sequences(args.frames, args.width, args.height):
                for term, constancy in TERMS:
                    rows += gpu_rows(flow2d, ctx, seq, term, constancy, args.tail)
    rows.sort(key=lambda q: (q["scene"], q["term"], q["pair"], q["engine"]))
    names = list(rows[0]["chains"])
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "table.md" if with_gpu else "table_numpy.md")
    with open(path, "w") as f:
        f.write("Mean endpoint error in pixels over the whole frame; in brackets the levels the pair ran and, for the oracle rows, the error "
                "of the prior it was given; adaptive chains also say how the pair ended.\n\n")
        f.write("| scene | data term | pair | engine | unseeded |" + "".join(" %s |" % name for name in names) + "\n")
        f.write("|" + "---|" * (5 + len(names)) + "\n")
        for q in rows:
            cells = []
            for name in names:
                c = q["chains"][name]
                notes = ["%d levels" % c["levels"]] + (["prior %.3f" % c["prior"]] if c["prior"] is not None else [])
                if name.startswith("tail"):
                    notes.append(MODES[c["mode"]])
                cells.append(" %.3f (%s) |" % (c["epe"], ", ".join(notes)))
            f.write("| %s | %s | %d | %s | %.3f |" % (q["scene"], q["term"], q["pair"], q["engine"], q["unseeded"]) + "".join(cells) + "\n")
    print("%d rows -> %s" % (len(rows), path))


if __name__ == "__main__":
    main()
