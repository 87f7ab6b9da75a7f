#!/usr/bin/env python3
"""What a strain window on the node grid gives against the routes there were before it.  The speckle pattern under the three
deformations of scenes.make_speckle_deformation (one pair each) and under step 2 of the stretch, shear and rotation of
scenes.make_speckle_deformation_sequence (the chained run), at 96 x 80 (11 x 9 nodes) and at 176 x 144 (21 x 17 nodes); grid
r = 7, s = 8, subsets of R = 7, the small-strain measure.  Per scene and size, the RMS and the largest error of exx, eyy, exy and
the vorticity against the scene's true gradients, over the nodes the row delivers, for

  direct       flow2d_node_strain_2d with window 0: the subsets' own gradients
  m, order 1   the window fit of order 1 with m = 1, 2, 3
  m, order 2   the window fit of order 2 with m = 2, 3
  expanded     the route there was: (u, v) of the converged nodes expanded to the frame's grid (flow2d_expand_nodes_2d) and
               flow2d_deformation_2d on that, sampled at the nodes

  python tools/node_strain_table.py --numpy    the rows of the numpy restatements (tests/test_node_strain_cpu.py on the nodes of
                                               tests/test_subset_sequence_cpu.py's chain), no device: writes
                                               profiles/node_strain/table_numpy.md, the committed rows
  python tools/node_strain_table.py            the device's rows (OpticalFlow.correlate_subset*, node_strain, Context.expand_nodes
                                               and deformation) into OUT/table.md; they must equal the committed rows digit for
                                               digit, else exit status 1
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = ((96, 80), (176, 144))
GRID_R, GRID_S, SUBSET_R = 7, 8, 7
FITS = (("direct", 0, 1), ("m = 1, order 1", 1, 1), ("m = 2, order 1", 2, 1), ("m = 3, order 1", 3, 1), ("m = 2, order 2", 2, 2),
        ("m = 3, order 2", 3, 2))
QUANTITIES = ("exx", "eyy", "exy", "vorticity")
HEADER = ("| scene | size | row | nodes | " + " | ".join("%s: RMS / largest" % q for q in QUANTITIES) + " |\n|" + "---|" * (4 + len(QUANTITIES)) + "\n")


def scene_list(width, height):
    sc = importlib.import_module("cuda-flow2d_amd.scenes")
    out = [("pair, " + name, [sc.make_speckle_deformation(name, width, height, seed=0)]) for name in sc.SPECKLE_DEFORMATIONS]
    out += [("sequence step 2, " + name, sc.make_speckle_deformation_sequence(name, 2, None, width, height, seed=0))
            for name in ("stretch", "shear", "rotation")]
    return out


def truth(scene):
    """exx, eyy, exy and the vorticity of the scene's affine motion (small strain), from its ground truth in double."""
    u, v = scene.gt_u.astype(np.float64), scene.gt_v.astype(np.float64)
    h, w = u.shape
    a, b = (u[0, -1] - u[0, 0]) / (w - 1), (u[-1, 0] - u[0, 0]) / (h - 1)
    c, d = (v[0, -1] - v[0, 0]) / (w - 1), (v[-1, 0] - v[0, 0]) / (h - 1)
    return dict(exx=a, eyy=d, exy=0.5 * (b + c), vorticity=c - b)


def line(scene_name, size, row, planes, want):
    valid = np.isfinite(planes["exx"])
    cells = []
    for q in QUANTITIES:
        e = planes[q][valid].astype(np.float64) - want[q]
        cells.append("%.3g / %.3g" % (np.sqrt(np.mean(e * e)), np.abs(e).max()) if valid.any() else "- / -")
    return "| %s | %d x %d | %s | %d | %s |\n" % (scene_name, size[0], size[1], row, int(valid.sum()), " | ".join(cells))


def rows_of(scene_name, size, scene, nodes, strain, expanded):
    """nodes: {name: [nh, nw]}; strain(nodes, window, order) -> planes; expanded(nodes) -> planes sampled at the nodes."""
    want = truth(scene)
    out = [line(scene_name, size, row, strain(nodes, m, order), want) for row, m, order in FITS]
    out.append(line(scene_name, size, "expanded", expanded(nodes), want))
    return out


def at_nodes(planes, nw, nh):
    cy, cx = GRID_R + np.arange(nh) * GRID_S, GRID_R + np.arange(nw) * GRID_S
    return {q: planes[q][np.ix_(cy, cx)] for q in QUANTITIES}


def numpy_rows():
    T = importlib.import_module("test_subset_sequence_cpu")
    N = importlib.import_module("test_node_strain_cpu")
    C = importlib.import_module("test_correlate_cpu")
    D = importlib.import_module("test_deformation_cpu")
    out = []
    for size in SIZES:
        w, h = size

        def strain(nodes, m, order):
            return N.node_strain_reference(nodes["u"], nodes["v"], nodes["state"], [nodes[n] for n in ("ux", "uy", "vx", "vy")], GRID_S, m, order)

        def expanded(nodes):
            nh, nw = nodes["u"].shape
            lost = ~(nodes["state"] >= 1)
            u, v = C.expand_reference(np.where(lost, np.nan, nodes["u"]), np.where(lost, np.nan, nodes["v"]), GRID_R, GRID_S, w, h)
            return at_nodes(D.deformation_reference(u, v), nw, nh)

        for scene_name, scenes in scene_list(w, h):
            if len(scenes) == 1:
                got = T.pair_chain(scenes[0], GRID_R, GRID_S, SUBSET_R)
            else:
                got = T.chained(scenes, GRID_R, GRID_S, SUBSET_R)[0][-1]
            nodes = {name: getattr(got, name) for name in got.NAMES}
            out += rows_of(scene_name, size, scenes[-1], nodes, strain, expanded)
            print(scene_name, size, flush=True)
    return out


def device_rows():
    flow2d = importlib.import_module("cuda-flow2d_amd")
    T = importlib.import_module("test_subset_sequence_cpu")
    out = []
    for size in SIZES:
        w, h = size
        flow = flow2d.OpticalFlow(w, h, flow2d.GREY)
        ctx = flow2d.Context(0)
        try:
            def strain(nodes, m, order):
                return flow.node_strain(nodes, GRID_S, m, order, planes=QUANTITIES, stats=False)[0]

            def expanded(nodes):
                nh, nw = nodes["u"].shape
                lost = ~(nodes["state"] >= 1)
                pu = ctx.plane(nw, nh, np.where(lost, np.nan, nodes["u"]).astype(np.float32))
                pv = ctx.plane(nw, nh, np.where(lost, np.nan, nodes["v"]).astype(np.float32))
                fu, fv = ctx.plane(w, h), ctx.plane(w, h)
                ctx.expand_nodes(pu, pv, nw, nh, GRID_R, GRID_S, fu, fv, w, h)
                planes, _ = ctx.deformation(fu, fv, w, h, planes=QUANTITIES, stats=False)
                return at_nodes(planes, nw, nh)

            for scene_name, scenes in scene_list(w, h):
                d = T.search_range(scenes[0], GRID_R, GRID_S)
                if len(scenes) == 1:
                    nodes = flow.correlate_subset(scenes[0].frame_0, scenes[0].frame_1, [(GRID_R, d, GRID_S)], SUBSET_R)[0]
                else:
                    frames = [scenes[0].frame_0] + [sc.frame_1 for sc in scenes]
                    nodes = flow.correlate_subset_sequence(frames, [(GRID_R, d, GRID_S)], SUBSET_R)[0][-1]
                out += rows_of(scene_name, size, scenes[-1], nodes, strain, expanded)
        finally:
            ctx.close()
            flow.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node_strain"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    committed = os.path.join(ROOT, "profiles", "node_strain", "table_numpy.md")  # the restatement's rows, kept in the repository
    if args.numpy:
        rows = numpy_rows()
        with open(committed, "w") as f:
            f.write(HEADER)
            f.writelines(rows)
        print("%d rows -> %s" % (len(rows), committed))
        return 0
    got = device_rows()
    with open(os.path.join(args.out, "table.md"), "w") as f:
        f.write(HEADER)
        f.writelines(got)
    want = open(committed).readlines()[2:]
    differing = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
    print("%d device rows -> %s; %s" % (len(got), os.path.join(args.out, "table.md"),
                                        "equal to the committed restatement rows" if got == want else "rows %s DIFFER from %s" % (differing, committed)))
    for k in differing:
        print("device:      " + got[k] + "restatement: " + want[k], end="")
    return 0 if got == want else 1


if __name__ == "__main__":
    sys.exit(main())
