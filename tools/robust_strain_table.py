#!/usr/bin/env python3
"""What the robust strain window gives beside the plain one, on the scenes of tools/node_strain_table.py: the speckle pattern
under the three deformations of scenes.make_speckle_deformation (one pair each) and under step 2 of the stretch, shear and rotation
of scenes.make_speckle_deformation_sequence (the chained run), at 96 x 80 (11 x 9 nodes) and at 176 x 144 (21 x 17 nodes); grid
r = 7, s = 8, subsets of R = 7, the small-strain measure.  Per scene, size and fit (m = 1, 2, 3 at order 1; m = 2, 3 at order 2) a
plain row (flow2d_node_strain_2d) and a robust row (flow2d_node_strain_robust_2d, sigma = 0.05 px, K = 8): the nodes delivered,
the RMS and the largest error of exx, eyy, exy and the vorticity against the scene's true gradients, and for the robust row the
record's three counts -- nodes that rejected a tap / rejected taps / suspect nodes.

  python tools/robust_strain_table.py --numpy   the rows of the numpy restatements (tests/test_node_strain_cpu.py and
                                                tests/test_node_strain_robust_cpu.py on the nodes of
                                                tests/test_subset_sequence_cpu.py's chain), no device: writes
                                                profiles/robust_strain/table_numpy.md, the committed rows
  python tools/robust_strain_table.py           the device's rows (OpticalFlow.correlate_subset*, node_strain with and without
                                                sigma=) into OUT/table.md; they must equal the committed rows digit for digit,
                                                else exit status 1
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SIGMA, PASSES = 0.05, 8
HEADER_CELLS = 5


def table_module():
    return importlib.import_module("node_strain_table")


def header(T):
    return ("| scene | size | row | nodes | " + " | ".join("%s: RMS / largest" % q for q in T.QUANTITIES) +
            " | touched / rejected / suspect |\n|" + "---|" * (HEADER_CELLS + len(T.QUANTITIES)) + "\n")


def rows_of(T, scene_name, size, scene, nodes, strain):
    """strain(nodes, window, order, robust) -> (planes, (touched, rejected, suspect) or None)."""
    want = T.truth(scene)
    out = []
    for row, m, order in T.FITS[1:]:  # (the direct form has nothing to reweight)
        for robust in (False, True):
            planes, counts = strain(nodes, m, order, robust)
            line = T.line(scene_name, size, row + (", robust" if robust else ", plain"), planes, want)
            out.append(line[:-1] + " %s |\n" % ("%d / %d / %d" % tuple(counts) if robust else "-"))
    return out


def numpy_rows():
    T = table_module()
    S = importlib.import_module("test_subset_sequence_cpu")
    N = importlib.import_module("test_node_strain_cpu")
    R = importlib.import_module("test_node_strain_robust_cpu")
    out = []
    for size in T.SIZES:
        w, h = size

        def strain(nodes, m, order, robust):
            if not robust:
                return N.node_strain_reference(nodes["u"], nodes["v"], nodes["state"], None, T.GRID_S, m, order), None
            ref = R.node_strain_robust_reference(nodes["u"], nodes["v"], nodes["state"], T.GRID_S, m, order, sigma=SIGMA, iterations=PASSES)
            return ref, R.robust_words(ref)

        for scene_name, scenes in T.scene_list(w, h):
            if len(scenes) == 1:
                got = S.pair_chain(scenes[0], T.GRID_R, T.GRID_S, T.SUBSET_R)
            else:
                got = S.chained(scenes, T.GRID_R, T.GRID_S, T.SUBSET_R)[0][-1]
            nodes = {name: getattr(got, name) for name in got.NAMES}
            out += rows_of(T, scene_name, size, scenes[-1], nodes, strain)
            print(scene_name, size, flush=True)
    return out


def device_rows():
    T = table_module()
    flow2d = importlib.import_module("cuda-flow2d_amd")
    S = importlib.import_module("test_subset_sequence_cpu")
    out = []
    for size in T.SIZES:
        w, h = size
        flow = flow2d.OpticalFlow(w, h, flow2d.GREY)
        try:
            def strain(nodes, m, order, robust):
                if not robust:
                    return flow.node_strain(nodes, T.GRID_S, m, order, planes=T.QUANTITIES, stats=False)[0], None
                planes, stats = flow.node_strain(nodes, T.GRID_S, m, order, planes=T.QUANTITIES, sigma=SIGMA, iterations=PASSES)
                counts = flow2d.node_strain_robust_counts(stats)
                return planes, [counts[k] for k in ("touched", "rejected", "suspect")]

            for scene_name, scenes in T.scene_list(w, h):
                d = S.search_range(scenes[0], T.GRID_R, T.GRID_S)
                if len(scenes) == 1:
                    nodes = flow.correlate_subset(scenes[0].frame_0, scenes[0].frame_1, [(T.GRID_R, d, T.GRID_S)], T.SUBSET_R)[0]
                else:
                    frames = [scenes[0].frame_0] + [sc.frame_1 for sc in scenes]
                    nodes = flow.correlate_subset_sequence(frames, [(T.GRID_R, d, T.GRID_S)], T.SUBSET_R)[0][-1]
                out += rows_of(T, scene_name, size, scenes[-1], nodes, strain)
        finally:
            flow.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust_strain"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    T = table_module()
    committed = os.path.join(ROOT, "profiles", "robust_strain", "table_numpy.md")  # the restatements' rows, kept in the repository
    if args.numpy:
        rows = numpy_rows()
        with open(committed, "w") as f:
            f.write(header(T))
            f.writelines(rows)
        print("%d rows -> %s" % (len(rows), committed))
        return 0
    got = device_rows()
    with open(os.path.join(args.out, "table.md"), "w") as f:
        f.write(header(T))
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
