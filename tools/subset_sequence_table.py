#!/usr/bin/env python3
"""What starting a step of a loading sequence from the previous step's deformation gains over correlating every pair on its own.
The speckle pattern at 96 x 80 rotates about its centre by 4 degrees per step, six steps, every frame against frame 0; grid r = 7,
s = 8, subsets of R = 7, 20 iterations, epsilon 1e-3, max_gradient 0.5.  Per step: the nodes that are judged -- the four corners
of the subset, moved by the true motion, lie at least 2 px inside the frame --; how many of them the pair chain alone finds (a
search of the range the motion needs, validated by replacement, the refinement from zero gradients with max_shift 2) and how many
the chained run finds (two prediction passes, the refinement from the previous step with max_shift 4) -- found: converged with
an endpoint error below 0.05 px --; the nodes of the whole grid that converged to a wrong place; the chained run's largest error
of a found node, its record and its prediction records.

  python tools/subset_sequence_table.py --numpy    the rows of the numpy restatement (tests/test_subset_sequence_cpu.py, sequential
                                                   sums), no device: writes profiles/subset_sequence/table_numpy.md, the committed rows
  python tools/subset_sequence_table.py            the device's rows (OpticalFlow.correlate_subset_sequence and correlate_subset) into
                                                   OUT/table.md; they must equal the committed rows digit for digit, else exit status 1
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HEADER = ("| frame 0 -> | search range | judged | pair alone: found / wrong | chained: found / wrong | chained, largest error of a found node | "
          "chained record | prediction passes (kept, predicted, empty) |\n|" + "---|" * 8 + "\n")


def line(degrees, d, pair, chain, record, prediction):
    return "| %g degrees | %d | %d | %d / %d | %d / %d | %.4f | %s | %s |\n" % (
        degrees, d, chain["judged"], pair["good"], pair["wrong"], chain["good"], chain["wrong"], chain["largest_good_error"],
        json.dumps(record), "; ".join("%d, %d, %d" % (p["kept"], p["predicted"], p["empty"]) for p in prediction) or "-")


def numpy_rows(T):
    rows, _ = T.rotation_rows()
    out = []
    for k, row in enumerate(rows):
        pair = T.pair_row(k + 1)
        out.append(line(row["degrees"], pair["range"], pair["pair"], row["chained"], row["record"], row.get("prediction", [])))
    return out


def device_rows(T):
    flow2d = importlib.import_module("cuda-flow2d_amd")
    S = importlib.import_module("test_subset_cpu")
    c = T.ROTATION
    scenes = T.rotation_scenes()
    r, s, R = c["r"], c["s"], c["R"]
    frames = [scenes[0].frame_0] + [sc.frame_1 for sc in scenes]

    def refined(nodes):
        got = S.Refined()
        for name in S.Refined.NAMES:
            setattr(got, name, nodes[name])
        return got

    flow = flow2d.OpticalFlow(c["width"], c["height"], flow2d.GREY)
    try:
        first = T.search_range(scenes[0], r, s)
        nodes, _, steps, _ = flow.correlate_subset_sequence(frames, [(r, first, s)], R)
        out = []
        for k, scene in enumerate(scenes):
            d = T.search_range(scene, r, s)
            alone, _, _, _ = flow.correlate_subset(scene.frame_0, scene.frame_1, [(r, d, s)], R)
            record = steps[k].subset.summary()
            prediction = [steps[k].prediction[p].summary() for p in range(2)] if k else []
            out.append(line(c["step_size"] * (k + 1), d, T.judge(scene, refined(alone), r, s, R), T.judge(scene, refined(nodes[k]), r, s, R),
                            record, prediction))
        return out
    finally:
        flow.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subset_sequence"))
    args = ap.parse_args()
    T = importlib.import_module("test_subset_sequence_cpu")
    os.makedirs(args.out, exist_ok=True)
    committed = os.path.join(ROOT, "profiles", "subset_sequence", "table_numpy.md")  # the restatement's rows, kept in the repository
    if args.numpy:
        rows = numpy_rows(T)
        with open(committed, "w") as f:
            f.write(HEADER)
            f.writelines(rows)
        print("%d steps -> %s" % (len(rows), committed))
        return 0
    got = device_rows(T)
    with open(os.path.join(args.out, "table.md"), "w") as f:
        f.write(HEADER)
        f.writelines(got)
    want = open(committed).readlines()[2:]
    differing = [k for k, (a, b) in enumerate(zip(got, want)) if a != b]
    print("%d device rows -> %s; %s" % (len(got), os.path.join(args.out, "table.md"),
                                        "equal to the committed restatement rows" if got == want else "rows %s DIFFER from %s" % (differing, committed)))
    return 0 if got == want else 1


if __name__ == "__main__":
    sys.exit(main())
