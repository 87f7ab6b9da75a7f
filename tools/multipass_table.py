#!/usr/bin/env python3
"""What the multi-pass window correlation gains over one pass on noisy frames: per case the mean endpoint error, the nodes off by
more than 1 px, the candidates scored (the sum of the passes' `candidates` counts) and the candidates times the window's pixels
(multiply-adds per sum), for one pass (radius 4, range 12, spacing 4) and for the schedule 15:12:16 -> 7:3:8 -> 4:2:4 with the
median test between the passes and at the end.  Cases: 160 x 128 speckle scenes `affine` and `large_translation`, seeds 0 and 1,
with Gaussian noise of sigma 30 grey levels on both frames and without noise; nodes at least 28 px from every border.

  python tools/multipass_table.py --numpy    the rows of the numpy restatement (tests/test_multipass_cpu.py), no device:
                                             writes profiles/multipass/table_numpy.md, the committed rows
  python tools/multipass_table.py            the device's rows (OpticalFlow.correlate_multipass, Context.correlate_offset) into
                                             OUT/table.md; they must equal the committed rows digit for digit, else exit status 1
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CASES = [(motion, seed, sigma) for sigma in (30.0, 0.0) for motion in ("affine", "large_translation") for seed in (0, 1)]
HEADER = "| scene | seed | noise sigma | method | nodes | mean EPE | off by > 1 px | candidates | candidates x N |\n|" + "---|" * 9 + "\n"


def lines(rows):
    out = []
    for q in rows:
        for method in ("single", "multi"):
            m = q[method]
            out.append("| %s | %d | %g | %s | %d | %s | %d | %d | %d |\n" % (
                q["motion"], q["seed"], q["sigma"], "one pass 4:12:4" if method == "single" else "15:12:16, 7:3:8, 4:2:4, validated",
                m["nodes"], m["epe"], m["off_by_1px"], m["candidates"], m["candidates_x_N"]))
    return out


def device_engines(T):
    """(single, chain, close): the device's counterparts of correlate_offset_reference and multipass_reference."""
    flow2d = importlib.import_module("cuda-flow2d_amd")
    ctx = flow2d.Context(0)
    flows = {}

    def single(f0, f1, lo, scale, r, d, s):
        h, w = f0.shape
        u, v, score, rec = ctx.correlate_offset(ctx.plane(w, h, f0), ctx.plane(w, h, f1), w, h, lo, scale, r, d, s)
        return u, v, score, np.frombuffer(bytes(rec), T.PASS_DTYPE)

    def chain(f0, f1, lo, scale, passes):
        h, w = f0.shape
        if (w, h) not in flows:
            flows[(w, h)] = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
        u, v, score, reports, used = flows[(w, h)].correlate_multipass(f0, f1, passes)
        assert (np.float32(used[0]), np.float32(used[1])) == (np.float32(lo), np.float32(scale))
        return u, v, score, [(q.nw, q.nh, np.frombuffer(bytes(q.correlation), T.PASS_DTYPE), np.frombuffer(bytes(q.validation), T.VALIDATION_DTYPE))
                             for q in reports], None

    def close():
        for flow in flows.values():
            flow.close()
        ctx.close()

    return single, chain, close


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multipass"))
    args = ap.parse_args()
    T = importlib.import_module("test_multipass_cpu")
    os.makedirs(args.out, exist_ok=True)
    committed = os.path.join(ROOT, "profiles", "multipass", "table_numpy.md")  # the restatement's rows, kept in the repository
    if args.numpy:
        rows = [T.accuracy_row(*case) for case in CASES]
        with open(committed, "w") as f:
            f.write(HEADER)
            f.writelines(lines(rows))
        print("%d cases -> %s" % (len(rows), committed))
        return 0
    single, chain, close = device_engines(T)
    try:
        rows = [T.accuracy_row(*case, single=single, chain=chain) for case in CASES]
    finally:
        close()
    got = lines(rows)
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
