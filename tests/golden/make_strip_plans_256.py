"""Writes tests/golden/strip_plans_256.json: the strip plans at 256 CUs of every level the benchmark's configurations can hand to
the strip solver (a superset: every pyramid level of 16 x 16 pixels and more), for the sweep counts of a launch (5, the 4 + 4 of a
chunked level, the 2 and 4 half-sweep stages of SOR, 1 and 3) and for a single pair and the lock-step group sizes of bench.py.

Run it on the commit whose plans are to be kept: it reads them through flow2d_fused_block_order on a zeroed stand-in for a context
(no device; a context without a CU count plans for 256), so it works on libraries from before the planning count existed.
tests/test_planning_cus_cpu.py asserts that the library still plans exactly these."""
import ctypes
import hashlib
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

# (width, height, levels, scale) of bench.py's workloads
PYRAMIDS = [(584, 388, 20, 0.9), (4096, 4096, 8, 0.5), (1024, 1024, 5, 0.5), (1920, 1080, 8, 0.5), (8192, 8192, 12, 0.5)]
INNER = (1, 2, 3, 4, 5)
INSTANCES = (1, 2, 8, 16, 32)


def level_sizes():
    """Level sizes as OpticalFlow2D computes them: ceil(size * powf(scale, level))."""
    sizes = set()
    for w, h, levels, scale in PYRAMIDS:
        for level in range(levels):
            s = np.float32(np.power(np.float32(scale), np.float32(level)))
            lw, lh = int(np.ceil(np.float32(w) * s)), int(np.ceil(np.float32(h) * s))
            if lw >= 16 and lh >= 16:
                sizes.add((lw, lh))
    return sorted(sizes)


def plan_of_order(order):
    """(rows_interior, rows_edge, strips_interior, blocks_x, blocks) read off a launch order (grid x 4: bx, by, y0, y1)."""
    live = order[order[:, 0] >= 0]
    blocks_x = int(live[:, 0].max()) + 1
    column = lambda bx: live[live[:, 0] == bx][np.argsort(live[live[:, 0] == bx][:, 1])]
    side = column(0)
    rows_edge = int(side[0, 3] - side[0, 2])
    middle = column(1) if blocks_x >= 3 else side
    border_aware = blocks_x >= 3 and len(middle) >= 3 and int(middle[1, 3] - middle[1, 2]) != rows_edge
    rows_interior = int(middle[1, 3] - middle[1, 2]) if border_aware else rows_edge
    return rows_interior, rows_edge, len(middle), blocks_x, len(live)


def order_at_256(lib, w, h, inner, instances):
    fake = ctypes.create_string_buffer(4096)  # a context without a CU count: the planners take 256
    cap = 1 << 17
    buf = (ctypes.c_int * (4 * cap))()
    grid = ctypes.c_size_t(0)
    rc = lib.flow2d_fused_block_order(ctypes.addressof(fake), w, h, inner, instances, buf, cap, ctypes.byref(grid))
    assert rc == 0, (rc, w, h, inner, instances)
    return np.frombuffer(buf, np.int32, 4 * grid.value).reshape(-1, 4).copy()


def records(lib):
    out = []
    for w, h in level_sizes():
        for inner in INNER:
            for instances in INSTANCES:
                order = order_at_256(lib, w, h, inner, instances)
                out.append([w, h, inner, instances, *plan_of_order(order), len(order),
                            hashlib.sha1(np.ascontiguousarray(order, "<i4").tobytes()).hexdigest()])
    return out


if __name__ == "__main__":
    lib = importlib.import_module("cuda-flow2d_amd").hip_lib()
    path = os.path.join(ROOT, "tests", "golden", "strip_plans_256.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in records(lib)) + "\n]\n")
    print("wrote", path)
