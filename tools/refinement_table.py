#!/usr/bin/env python3
"""What the edge-aware refinement (flow2d_refine_flow_2d) does to a flow on the analytic scenes (scenes.SCENES): the endpoint
error over all, the non-occluded and the occluded pixels before and after one pass, for r in {3, 5, 7}, with and without the guide
(frame 0, sigma 25 grey levels) and the mask.

Flows:
  true, occlusions smeared   the true flow with the occluded pixels set to the square's motion (4.5, -2.25): what a solver leaves
                             where the foreground covers the background (two_layer only; mask = the true occlusion map)
  true + noise               the true flow plus Gaussian noise of 0.5 px (default_rng(1)); no mask exists
  computed                   the bidirectional flow of the CLI's default parameters; mask = its forward occlusion mask

  python tools/refinement_table.py            every row; needs the GPU (flows and filter run on it)
  python tools/refinement_table.py --numpy    the true-flow rows alone, through the numpy restatement
                                              (tests/test_refine_cpu.py), no device
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
RADII = (3, 5, 7)
SIGMA_GUIDE = 25.0
F32 = np.float32


def epe3(u, v, sc):
    """EPE over all, the non-occluded and the occluded pixels (None where the scene has no occluded pixel)."""
    e = np.hypot(u.astype(np.float64) - sc.gt_u, v.astype(np.float64) - sc.gt_v)
    if sc.occlusion is None or not (sc.occlusion > 0).any():
        return float(e.mean()), float(e.mean()), None
    occ = sc.occlusion > 0
    return float(e.mean()), float(e[~occ].mean()), float(e[occ].mean())


def true_flows(sc):
    """(source, u, v, mask or None) for the corrupted true flows of the scene."""
    out = []
    if sc.name == "two_layer":
        u, v = sc.gt_u.copy(), sc.gt_v.copy()
        u[sc.occlusion > 0], v[sc.occlusion > 0] = 4.5, -2.25
        out.append(("true, occlusions smeared", u, v, np.asarray(sc.occlusion, F32)))
    rng = np.random.default_rng(1)
    u = (sc.gt_u + 0.5 * rng.standard_normal(sc.gt_u.shape)).astype(F32)
    v = (sc.gt_v + 0.5 * rng.standard_normal(sc.gt_v.shape)).astype(F32)
    out.append(("true + noise 0.5", u, v, None))
    return out


def rows_of(sc, source, engine, u, v, mask, refine):
    """One row per radius and variant; refine(u, v, guide or None, mask or None, r, sigma_guide) -> (u, v, record summary)."""
    rows, before = [], epe3(u, v, sc)
    for r in RADII:
        for guide in (False, True):
            for masked in ((False, True) if mask is not None else (False,)):
                ou, ov, rec = refine(u, v, sc.frame_0 if guide else None, mask if masked else None, r, SIGMA_GUIDE if guide else 0.0)
                rows.append({"scene": sc.name, "source": source, "engine": engine, "r": r, "guide": guide, "mask": masked,
                             "before": before, "after": epe3(ou, ov, sc), "record": rec})
    return rows


def numpy_refine(u, v, guide, mask, r, sigma_guide):
    ou, ov, rec = importlib.import_module("test_refine_cpu").refine_reference(u, v, guide, mask, r, sigma_guide)
    return ou, ov, {name: int(rec[name][0]) for name in rec.dtype.names}


def numpy_rows(size, seed):
    rows = []
    for name in scenes.SCENES:
        sc = scenes.make_scene(name, size, size, seed)
        for source, u, v, mask in true_flows(sc):
            rows += rows_of(sc, source, "numpy", u, v, mask, numpy_refine)
    return rows


def gpu_rows(size, seed):
    flow2d = importlib.import_module("cuda-flow2d_amd")
    rows = []
    with flow2d.Context(0) as ctx:
        def gpu_refine(u, v, guide, mask, r, sigma_guide):
            up = lambda a: None if a is None else ctx.plane(size, size, a)  # noqa: E731
            ou, ov, rec = ctx.refine_flow(up(u), up(v), size, size, r, up(guide), up(mask), sigma_guide)
            return ou, ov, rec.summary()

        flow = flow2d.OpticalFlow(size, size, flow2d.GREY, ctx=ctx)
        try:
            p = flow.params(*PARAMS)
            for name in scenes.SCENES:
                sc = scenes.make_scene(name, size, size, seed)
                for source, u, v, mask in true_flows(sc):
                    rows += rows_of(sc, source, "gpu", u, v, mask, gpu_refine)
                planes = [ctx.plane(size, size) for _ in range(6)]
                f0, f1 = ctx.plane(size, size, sc.frame_0), ctx.plane(size, size, sc.frame_1)
                flow.compute_flow_bidirectional_device([f0.ptr, f1.ptr], *[[q.ptr] for q in planes[:4]], p, [planes[4].ptr], [planes[5].ptr])
                ctx.synchronize()
                rows += rows_of(sc, "computed", "gpu", planes[0].download(), planes[1].download(), planes[4].download(), gpu_refine)
        finally:
            flow.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refinement"))
    args = ap.parse_args()
    rows = numpy_rows(args.size, args.seed)
    if not args.numpy:
        rows += gpu_rows(args.size, args.seed)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "table_numpy.md" if args.numpy else "table.md")
    cell = lambda x: "-" if x is None else "%.4f" % x  # noqa: E731
    with open(path, "w") as f:
        f.write("| scene | flow | engine | r | guide | mask | EPE all | EPE noc | EPE occ | after: all | noc | occ | unfilled | filled | changed |\n")
        f.write("|" + "---|" * 15 + "\n")
        for r in rows:
            f.write("| %s | %s | %s | %d | %s | %s | %s | %s | %s | %s | %s | %s | %d | %d | %d |\n" %
                    ((r["scene"], r["source"], r["engine"], r["r"], "yes" if r["guide"] else "no", "yes" if r["mask"] else "no") +
                     tuple(cell(x) for x in r["before"] + r["after"]) +
                     (r["record"]["unfilled"], r["record"]["filled"], r["record"]["changed"])))
    print("%d rows -> %s" % (len(rows), path))


if __name__ == "__main__":
    main()
