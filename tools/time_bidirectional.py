"""Bidirectional flow with occlusion masks against the same work done without it, one stream (developer tool).
usage: python tools/time_bidirectional.py [--reps N] [workload ...]     (default: cfg1_rub cfg2_1024_grey cfg3_4096_gradient)

Per workload, the median of N timed regions (device events around the region on the stream that runs it, then a synchronise):
  (a) two eager ComputeFlowDevice calls on one stream: frame 0 -> frame 1, then frame 1 -> frame 0
  (b) ComputeFlowBidirectionalDevice without mask planes (the pyramids of both frames built once)
  (c) ComputeFlowBidirectionalDevice with both masks
  (d) information only: a scattered lock-step group of two (ComputeFlowGroupDevice, count 2, the frames swapped in the second
      pair; OpticalFlowBatch2D with one lane) followed by two flow2d_consistency_2d launches on the lane's stream
Kernel durations come from a separate `rocprofv3 --kernel-trace --stats` run of this tool (profiles/bidirectional/README.md)."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F = importlib.import_module("cuda-flow2d_amd")
import bench  # noqa: E402

DEFAULT = ["cfg1_rub", "cfg2_1024_grey", "cfg3_4096_gradient"]


def timed(lib, handle, fn, reps):
    """Median ms of `reps` regions: event, fn(), event on the context's stream, synchronise (after two untimed runs)."""
    evs = [C.c_void_p(), C.c_void_p()]
    for e in evs:
        F._check(lib.flow2d_event_create(handle, C.byref(e)), "flow2d_event_create")
    for _ in range(2):
        fn()
    F._check(lib.flow2d_synchronize(handle), "flow2d_synchronize")
    out = []
    for _ in range(reps):
        lib.flow2d_event_record(handle, evs[0])
        fn()
        lib.flow2d_event_record(handle, evs[1])
        F._check(lib.flow2d_synchronize(handle), "flow2d_synchronize")
        ms = C.c_float()
        F._check(lib.flow2d_event_elapsed_ms(handle, evs[0], evs[1], C.byref(ms)), "flow2d_event_elapsed_ms")
        out.append(ms.value)
    for e in evs:
        lib.flow2d_event_destroy(handle, e)
    return float(np.median(out))


def run(name, reps):
    cfg = bench.WORKLOADS[name]
    w, h = cfg["w"], cfg["h"]
    f0, f1 = bench.workload_pair(name, cfg, 0)
    lib = F.hip_lib()
    ctx = F.Context(0)
    flow = F.OpticalFlow(w, h, cfg["constancy"], ctx=ctx)
    p = flow.params(cfg["levels"], cfg["scale"], cfg["outer"], cfg["inner"], cfg["alpha"], 0.001, 0.001, cfg["median"],
                    cfg["sigma"])
    frames = [ctx.plane(w, h, f0), ctx.plane(w, h, f1)]
    u, v, bu, bv, o0, o1 = (ctx.plane(w, h) for _ in range(6))
    fr = [q.ptr for q in frames]

    def two_calls():
        flow.compute_flow_device(fr[0], fr[1], u.ptr, v.ptr, p)
        flow.compute_flow_device(fr[1], fr[0], bu.ptr, bv.ptr, p)

    def bidirectional(masks):
        occ = ([o0.ptr], [o1.ptr]) if masks else (None, None)
        flow.compute_flow_bidirectional_device(fr, [u.ptr], [v.ptr], [bu.ptr], [bv.ptr], p, *occ)

    res = {"workload": name, "w": w, "h": h, "reps": reps,
           "a_two_calls_ms": timed(lib, ctx.handle, two_calls, reps),
           "b_bidirectional_ms": timed(lib, ctx.handle, lambda: bidirectional(False), reps),
           "c_bidirectional_masks_ms": timed(lib, ctx.handle, lambda: bidirectional(True), reps)}
    flow.close()

    # (d): a lock-step group of the two directions on one lane, then the two masks on the lane's stream
    batch = F.OpticalFlowBatch(w, h, cfg["constancy"], lanes=1, group_size=2)
    lane = F.host_lib().flow2d_host_batch_lane_context(batch.handle, 0)

    def group():
        batch.compute_flow_batch_device_grouped([fr[0], fr[1]], [fr[1], fr[0]], [u.ptr, bu.ptr], [v.ptr, bv.ptr], p)
        for a, b, out in ((u, bu, o0), (bu, u, o1)):
            c, d = (v, bv) if a is u else (bv, v)
            F._check(lib.flow2d_consistency_2d(lane, a.ptr, c.ptr, b.ptr, d.ptr, w, h, a.pitch, C.c_float(0.01),
                                               C.c_float(0.5), out.ptr), "flow2d_consistency_2d")

    res["d_group_plus_masks_ms"] = timed(lib, lane, group, reps)
    batch.close()
    res["b_over_a"] = res["b_bidirectional_ms"] / res["a_two_calls_ms"]
    res["c_minus_b_over_b"] = (res["c_bidirectional_masks_ms"] - res["b_bidirectional_ms"]) / res["b_bidirectional_ms"]
    ctx.close()
    return res


def main():
    args = sys.argv[1:]
    reps = 7
    if "--reps" in args:
        i = args.index("--reps")
        reps = int(args[i + 1])
        del args[i:i + 2]
    for name in args or DEFAULT:
        print(json.dumps(run(name, reps)), flush=True)


if __name__ == "__main__":
    main()
