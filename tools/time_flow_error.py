#!/usr/bin/env python3
"""Times flow2d_flow_error_2d (partials + final launch) at 4096^2 on the MI355X with device events, in three forms: record
only (16 B/px read), with an occlusion plane (20 B/px), and with the mask and both per-pixel planes written (28 B/px).  Prints
one JSON line per form: microseconds per call and the algorithmic bytes over that time, also as a fraction of 8 TB/s.
Run it under `rocprofv3 --kernel-trace --stats` for the kernels' own times (profiles/accuracy/).

    python tools/time_flow_error.py [--size 4096] [--calls 50]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
flow2d = importlib.import_module("cuda-flow2d_amd")

PEAK_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    if flow2d.device_count() < 1:
        sys.exit("no HIP device: timing needs the MI355X")
    n = args.size
    rng = np.random.default_rng(0)
    gt = [rng.uniform(-20, 20, (n, n)).astype(np.float32) for _ in range(2)]
    est = [(g + rng.normal(0, 1, (n, n))).astype(np.float32) for g in gt]
    occ = (rng.random((n, n)) < 0.1).astype(np.float32)
    with flow2d.Context(0) as ctx:
        u, v, gu, gv, m = (ctx.plane(n, n, a) for a in est + gt + [occ])
        epe, ae = ctx.plane(n, n), ctx.plane(n, n)
        lib = flow2d.hip_lib()
        need = lib.flow2d_flow_error_workspace_bytes(n, n, 1)
        ws, stats = ctx.plane(need // 4, 1), ctx.plane(64, 1)
        start, stop = ctx.event(), ctx.event()
        forms = (("record", None, None, None, 16), ("record+mask", m, None, None, 20), ("record+mask+planes", m, epe, ae, 28))
        for name, mask, pe, pa, bpp in forms:
            def call():
                rc = lib.flow2d_flow_error_2d(ctx.handle, u.ptr, v.ptr, gu.ptr, gv.ptr, mask.ptr if mask else None, n, n, u.pitch,
                                              pe.ptr if pe else None, pa.ptr if pa else None, stats.ptr, ws.ptr, need)
                if rc:
                    raise flow2d.Flow2DError(rc, "flow2d_flow_error_2d")
            for _ in range(5):
                call()
            ctx.synchronize()
            ctx.record(start)
            for _ in range(args.calls):
                call()
            ctx.record(stop)
            us = ctx.elapsed_ms(start, stop) * 1e3 / args.calls
            bytes_ = bpp * n * n
            print(json.dumps({"form": name, "size": n, "calls": args.calls, "us_per_call": round(us, 2),
                              "algorithmic_bytes": bytes_, "tb_per_s": round(bytes_ / us / 1e6, 3),
                              "fraction_of_8tbs": round(bytes_ / (us * 1e-6) / PEAK_BYTES_PER_S, 3)}))


if __name__ == "__main__":
    main()
