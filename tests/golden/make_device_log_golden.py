"""Generates tests/golden/device_log_golden.npz: log(I + 1.0f) of the two 96 x 64 frames of ref_kernels_golden.npz
(tile_in_f0 / tile_in_f1) AS AN MI355X FORMS IT, through the product's flow2d_log_frame_2d -- the function every HIP kernel of the
log-derivative term calls (the device library's logf).

With these planes behind oracle_set_log_source the CPU tests hold the oracle's solve_2d_log to the reference kernel's recorded
outputs (tile_sweep_log_*, tile_solve_log_*) bit for bit without a GPU (tests/test_oracle.py::test_ref_golden_log_derivatives);
tests/test_gpu_log_derivatives.py::test_log_frame_fixture_is_what_the_device_returns notices when the device library's logf
moves.  The fixture holds the entry's output only.

Run where an MI355X is:   python tests/golden/make_device_log_golden.py [output.npz]
(default: tests/golden/device_log_golden.npz, the committed file itself).
"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main():
    flow2d = importlib.import_module("cuda-flow2d_amd")
    g = np.load(os.path.join(HERE, "ref_kernels_golden.npz"))
    out = {}
    with flow2d.Context(0) as ctx:
        for name in ("f0", "f1"):
            frame = np.ascontiguousarray(g["tile_in_" + name], np.float32)
            h, w = frame.shape
            dst = ctx.plane(w, h)
            ctx.log_frame(ctx.plane(w, h, frame), dst, w, h)
            out["log_" + name] = dst.download()
            libm = np.log(frame.astype(np.float64) + 1.0).astype(np.float32)
            print("log_%s: %d x %d, %d of %d words differ from float64 log rounded to float32" %
                  (name, w, h, int((out["log_" + name].view(np.uint32) != libm.view(np.uint32)).sum()), w * h))
    path = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(HERE, "device_log_golden.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
