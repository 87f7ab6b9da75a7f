#!/usr/bin/env python3
"""What moving the reference frame of a loading sequence gains (SequenceOptions::reference_every, flow2d_compose_nodes_2d).
The speckle pattern at 96 x 80, grid r = 7, s = 8, subsets of R = 7, the defaults elsewhere; every pair chain -- step 1 and the
first step after a reference change -- searches a range of 6.  Two sequences of fifteen steps: a rotation of 4 degrees per step to
60 degrees, and a stretch (1 + 0.04 k) x (1 - 0.02 k) to ux = 0.6, past max_gradient = 0.5 at step 13.  For a fixed reference
(N = 0) and a new reference every N = 3 and N = 5 steps, per step: the judged nodes -- the four corners of the subset, moved by the
true motion, lie at least 2 px inside the frame --, how many of them are found (usable, endpoint error below 0.05 px against the
true motion from frame 0), the nodes of the grid found in a wrong place, the largest error of a found node and the composition's
record.  Last, the RMS of the Green-Lagrange strain of the delivered 60-degree field, from its own gradients (window 0): a rigid
rotation has none.

  python tools/subset_reference_table.py --numpy   the rows of the numpy restatement (tests/test_subset_reference_cpu.py, sequential
                                                   sums), no device: writes profiles/subset_reference/table_numpy.md, the committed rows
  python tools/subset_reference_table.py           the device's rows (OpticalFlow.correlate_subset_sequence with reference_every) into
                                                   OUT/table.md; they must equal the committed rows digit for digit, else exit status 1
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HEADER = ("| sequence | reference | frame 0 -> | judged | found / wrong | largest error of a found node | "
          "composition (composed, no base, outside, no increment) |\n|" + "---|" * 7 + "\n")
POLICIES = (0, 3, 5)


def lines(T, what, unit, reference_every, rows):
    out = []
    for row in rows:
        c = row["compose"]
        out.append("| %s | %s | %g %s | %d | %d / %d | %.4f | %s |\n" % (
            what, "every %d steps" % reference_every if reference_every else "fixed", row["amount"], unit, row["judged"], row["good"],
            row["wrong"], row["largest_good_error"], "-" if c is None else "%d, %d, %d, %d" % tuple(c[1:])))
    return out


def strain_line(reference_every, field):
    N = importlib.import_module("test_node_strain_cpu")
    ref = N.node_strain_reference(field.u, field.v, field.state, [field.ux, field.uy, field.vx, field.vy], 8, 0, measure=N.GREEN)
    e = np.stack([ref[n][ref["valid"]].astype(np.float64) for n in ("exx", "eyy", "exy")])
    rms = float(np.sqrt((e * e).mean())) if e.size else float("nan")
    return "| rotation | %s | 60 degrees: RMS of exx, eyy, exy (Green-Lagrange, window 0) over %d nodes | | | %.6f | |\n" % (
        "every %d steps" % reference_every if reference_every else "fixed", int(ref["valid"].sum()), rms)


def table(T, rows_of):
    """rows_of(name, reference_every) -> (rows, delivered fields)."""
    out, strain = [], []
    for name, unit in (("rotation", "degrees"), ("stretch", "ux")):
        for n in POLICIES:
            rows, delivered = rows_of(name, n)
            out += lines(T, name, unit, n, rows)
            if name == "rotation":
                strain.append(strain_line(n, delivered[-1]))
    return out + strain


def numpy_rows(T):
    return table(T, lambda name, n: (T.rotation_rows if name == "rotation" else T.stretch_rows)(n))


def device_rows(T):
    flow2d = importlib.import_module("cuda-flow2d_amd")

    def rows_of(name, n):
        c = T.ROTATION if name == "rotation" else T.STRETCH
        scenes = T.rotation_scenes() if name == "rotation" else T.stretch_scenes()
        frames = [scenes[0].frame_0] + [sc.frame_1 for sc in scenes]
        flow = flow2d.OpticalFlow(c["width"], c["height"], flow2d.GREY)
        try:
            nodes = flow.correlate_subset_sequence(frames, [(c["r"], c["d"], c["s"])], c["R"], reference_every=n)[0]
            records = [None if not q.nodes else np.frombuffer(bytes(q), T.COMPOSE_DTYPE) for q in flow.compose_records]
        finally:
            flow.close()
        delivered = [T.composed_field([step[p] for p in T.PLANES], step["state"], step["score"], None) for step in nodes]
        return T.step_rows(scenes, delivered, records, c["r"], c["s"], c["R"], c["step_size"]), delivered

    return table(T, rows_of)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset_reference"))
    args = ap.parse_args()
    T = importlib.import_module("test_subset_reference_cpu")
    os.makedirs(args.out, exist_ok=True)
    committed = os.path.join(ROOT, "profiles", "subset_reference", "table_numpy.md")  # the restatement's rows, kept in the repository
    if args.numpy:
        rows = numpy_rows(T)
        with open(committed, "w") as f:
            f.write(HEADER)
            f.writelines(rows)
        print("%d rows -> %s" % (len(rows), committed))
        return 0
    got = device_rows(T)
    with open(os.path.join(args.out, "table.md"), "w") as f:
        f.write(HEADER)
        f.writelines(got)
    want = open(committed).readlines()[2:]
    differing = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
    print("%d device rows -> %s; %s" % (len(got), os.path.join(args.out, "table.md"),
                                        "equal to the committed restatement rows" if got == want else "rows %s DIFFER from %s" % (differing, committed)))
    for k in differing[:10]:
        print("device:    " + got[k] + "committed: " + want[k], end="")
    return 0 if got == want else 1


if __name__ == "__main__":
    sys.exit(main())
