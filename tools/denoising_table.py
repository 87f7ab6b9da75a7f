#!/usr/bin/env python3
"""What motion-compensated temporal denoising (flow2d_denoise_2d, OpticalFlow.denoise_sequence) gains on the analytic sequences
of cuda-flow2d_amd/scenes.py: every scene x noise level x radius in {1, 2} x range_sigma off / on x masks on / off x flow source.
The noise is seeded Gaussian noise added to the exact frames (5 frames); per row the RMSE of all frames against the clean
ones before and after, and on two_layer also over the pixels whose content is hidden in some neighbour frame.

Flow sources
  true          the scenes' exact flows between any two frames and, with masks, their exact visibility, through Context.denoise
                on the GPU and through the numpy restatement of the definition (tests/test_denoise_cpu.py) on the CPU: the two
                columns must agree to the last digit, the kernel being bit-identical to the restatement
  jacobi / sor  flows and masks computed from the NOISY frames by OpticalFlow.denoise_sequence with the CLI's defaults
                (Jacobi sweeps) and with --sor 1.9; GPU only

    python tools/denoising_table.py [--numpy] [--size 256] [--seed 0] [--out profiles/denoising]

--numpy runs the true-flow rows alone, on the CPU, and leaves the GPU columns empty.  Without it the GPU rows and the numpy rows
are written side by side.  Either way: OUT/README.md (with the timings of tools/time_denoising.py when
OUT/time_denoising_4096.json is there) and OUT/table.jsonl."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

flow2d = importlib.import_module("cuda-flow2d_amd")
scenes = importlib.import_module("cuda-flow2d_amd.scenes")

PARAMS = (50, 0.9, 40, 5, 35.0, 0.001, 0.001, 5, 1.5)
FRAMES = 5
NOISE = (4.0, 8.0, 16.0)
NOISE_COMPUTED = (8.0,)  # the rows with computed flows: every one recomputes the flows of the whole sequence
RADII = (1, 2)
SOURCES = ("true", "jacobi", "sor")
F32 = np.float32


def noisy(frames, seed, sigma):
    """Seeded Gaussian noise of standard deviation `sigma` added to the exact frames."""
    rng = np.random.default_rng(1000 + seed)
    return (frames.astype(np.float64) + rng.normal(0, sigma, frames.shape)).astype(F32)


def range_sigma_of(noise):
    """The photometric scale of the "on" rows: three noise standard deviations, so noise alone keeps most of a sample's weight."""
    return 3.0 * noise


def true_neighbours(seq, frames, k, radius, masks):
    js = [j for j in range(k - radius, k + radius + 1) if j != k and 0 <= j < seq.frame_count]
    flows = [seq.flow_between(k, j) for j in js]
    occs = [(~f[2]).astype(F32) for f in flows] if masks else None
    return [frames[j] for j in js], [f[0] for f in flows], [f[1] for f in flows], occs


def hidden_pixels(seq, radius):
    """Per frame: the pixels whose content is not seen in some neighbour within `radius`."""
    out = []
    for k in range(seq.frame_count):
        hid = np.zeros((seq.height, seq.width), bool)
        for j in range(k - radius, k + radius + 1):
            if j != k and 0 <= j < seq.frame_count:
                hid |= ~seq.flow_between(k, j)[2]
        out.append(hid)
    return np.stack(out)


class TrueFlowFuser:
    """Frame k fused with its neighbours along the true flows: Context.denoise on the GPU, the restatement with use_numpy."""

    def __init__(self, use_numpy, w, h):
        self.use_numpy = use_numpy
        if not use_numpy:
            self.ctx = flow2d.Context(0)
            self.centre, self.out = self.ctx.plane(w, h), self.ctx.plane(w, h)
            self.planes = [[self.ctx.plane(w, h) for _ in range(4)] for _ in range(2 * max(RADII))]

    def __call__(self, centre, frames, us, vs, occs, range_sigma):
        if self.use_numpy:
            from test_denoise_cpu import denoise_reference
            return denoise_reference(centre, frames, us, vs, occs, range_sigma)[0]
        n = len(frames)
        for k in range(n):
            for plane, a in zip(self.planes[k], (frames[k], us[k], vs[k], None if occs is None else occs[k])):
                if a is not None:
                    plane.upload(a)
        h, w = centre.shape
        self.ctx.denoise(self.centre.upload(centre), [p[0] for p in self.planes[:n]], [p[1] for p in self.planes[:n]],
                         [p[2] for p in self.planes[:n]], w, h, self.out,
                         None if occs is None else [p[3] for p in self.planes[:n]], range_sigma)
        self.ctx.synchronize()
        return self.out.download()

    def close(self):
        if not self.use_numpy:
            self.ctx.close()


def rmse(a, b, sel=None):
    e = a.astype(np.float64) - b.astype(np.float64)
    e = e if sel is None else e[sel]
    return float(np.sqrt((e * e).mean())) if e.size else float("nan")


def row_of(name, noise, radius, range_sigma, masks, source, engine, clean, noised, fused, hidden):
    return {"scene": name, "noise": noise, "radius": radius, "range_sigma": range_sigma, "masks": masks, "flows": source,
            "engine": engine, "rmse_before": rmse(noised, clean), "rmse_after": rmse(fused, clean),
            "hidden_before": rmse(noised, clean, hidden) if name == "two_layer" else None,
            "hidden_after": rmse(fused, clean, hidden) if name == "two_layer" else None}


def true_rows(use_numpy, size, seed, scene_names=scenes.SCENES, noise_levels=NOISE):
    """The rows with the scenes' true flows, from the GPU or (use_numpy) from the restatement."""
    rows = []
    fuser = TrueFlowFuser(use_numpy, size, size)
    try:
        for name in scene_names:
            seq = scenes.make_sequence(name, FRAMES, size, size, seed)
            for noise in noise_levels:
                noised = noisy(seq.frames, seed, noise)
                for radius in RADII:
                    hidden = hidden_pixels(seq, radius)
                    for range_sigma in (0.0, range_sigma_of(noise)):
                        for masks in (True, False):
                            fused = np.stack([fuser(noised[k], *true_neighbours(seq, noised, k, radius, masks), range_sigma)
                                              for k in range(FRAMES)])
                            rows.append(row_of(name, noise, radius, range_sigma, masks, "true", "numpy" if use_numpy else "gpu",
                                               seq.frames, noised, fused, hidden))
    finally:
        fuser.close()
    return rows


def computed_rows(size, seed):
    """The rows with flows and masks computed from the noisy frames: OpticalFlow.denoise_sequence, Jacobi and SOR 1.9."""
    rows = []
    flow = flow2d.OpticalFlow(size, size, flow2d.GREY)
    try:
        for name in scenes.SCENES:
            seq = scenes.make_sequence(name, FRAMES, size, size, seed)
            for noise in NOISE_COMPUTED:
                noised = noisy(seq.frames, seed, noise)
                for source, params in (("jacobi", flow.params(*PARAMS)), ("sor", flow.params(*PARAMS, sor_omega=1.9))):
                    for radius in RADII:
                        hidden = hidden_pixels(seq, radius)
                        for range_sigma in (0.0, range_sigma_of(noise)):
                            for masks in (True, False):
                                fused = flow.denoise_sequence(noised, params, radius, range_sigma, masks)
                                rows.append(row_of(name, noise, radius, range_sigma, masks, source, "gpu", seq.frames, noised,
                                                   fused, hidden))
    finally:
        flow.close()
    return rows


def key_of(r):
    return (r["scene"], r["noise"], r["radius"], r["range_sigma"], r["masks"], r["flows"])


def fmt(v):
    return "-" if v is None or v != v else "%.4f" % v


def timing_section(path):
    if not os.path.exists(path):
        return []
    t = json.load(open(path))
    lines = ["", "## Speed at %d x %d (tools/time_denoising.py, %s)" % (t["size"], t["size"], t["device"]), "",
             "Medians of %d launches each, the variants alternating in one process.  `fused` is one flow2d_denoise_2d launch;"
             % t["launches"],
             "`N warps` is N launches of flow2d_registration_2d, what warping the neighbours took before this entry (and it",
             "does not average anything yet).  The fraction is of 8 TB/s on the 8 + 16 N algorithmic bytes per pixel (8 + 12 N",
             "without masks).", "",
             "| N | fused, no masks (ms) | N warps (ms) | fused / warps | fraction of 8 TB/s | fused, masks (ms) | fraction of 8 TB/s |",
             "|---|---|---|---|---|---|---|"]
    for r in t["kernels"]:
        lines.append("| %d | %.3f | %.3f | %.2f | %.2f | %.3f | %.2f |" % (
            r["n"], r["fused_ms"], r["warps_ms"], r["fused_ms"] / r["warps_ms"], r["fraction_no_masks"], r["fused_masks_ms"],
            r["fraction_masks"]))
    lines += ["", "flow2d_compose_flow_2d with masks: %.3f ms." % t["compose_ms"]]
    s = t.get("sequence")
    if s:
        lines += ["", "Whole path, radius 1, masks on, %d frames, medians of %d runs: OpticalFlow.denoise_sequence_device takes %.1f ms per frame; one"
                  % (s["frames"], s.get("runs", 3), s["per_frame_ms"]),
                  "ComputeFlowBidirectionalDevice pair (both flows, both masks) takes %.1f ms.  A sequence of n frames computes n - 1"
                  % s["pair_ms"],
                  "pairs, so per frame the fusion adds %.1f %% to the flow computation."
                  % (100.0 * (s["per_frame_ms"] * s["frames"] - s["pair_ms"] * (s["frames"] - 1)) / (s["pair_ms"] * (s["frames"] - 1)))]
    return lines


def write_readme(out_dir, gpu_rows, numpy_rows, size, seed):
    by_key = {key_of(r): r for r in numpy_rows}
    lines = ["# Motion-compensated temporal denoising: what it gains", "",
             "Written by `tools/denoising_table.py --size %d --seed %d`: the analytic sequences of `cuda-flow2d_amd/scenes.py`, %d frames,"
             % (size, seed, FRAMES),
             "seeded Gaussian noise added to the exact frames.  RMSE in grey levels of all frames against the clean ones, before",
             "and after `flow2d_denoise_2d`; on two_layer also over the pixels whose content is hidden in some neighbour frame.",
             "`true` rows use the scenes' exact flows (and visibility as masks).  range sigma is 0 (off) or three noise standard",
             "deviations."]
    if gpu_rows:
        lines += ["The GPU column is `Context.denoise`, the numpy column the restatement of the definition: they agree because the",
                  "kernel is bit-identical to it.  `jacobi` / `sor` rows are `OpticalFlow.denoise_sequence` with flows and masks computed",
                  "from the noisy frames (the CLI's defaults; `--sor 1.9`); they have no numpy column."]
    else:
        lines += ["**This file was written with `--numpy`, without a GPU: the GPU columns are empty, the rows with computed flows",
                  "(Jacobi, SOR 1.9) are missing, and the numpy column is the restatement of the definition alone.**"]
    if not os.path.exists(os.path.join(out_dir, "time_denoising_4096.json")):
        lines += ["**No timing has been measured: `tools/time_denoising.py` has not been run for this file.**"]
    lines += ["",
             "| scene | noise | radius | range sigma | masks | flows | before | after (GPU) | after (numpy) | hidden before | hidden after (GPU) | hidden after (numpy) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in gpu_rows if gpu_rows else numpy_rows:  # (--numpy: no GPU column)
        n = by_key.get(key_of(r))
        g = r if gpu_rows else None
        lines.append("| %s | %g | %d | %g | %s | %s | %s | %s | %s | %s | %s | %s |" % (
            r["scene"], r["noise"], r["radius"], r["range_sigma"], "on" if r["masks"] else "off", r["flows"], fmt(r["rmse_before"]),
            fmt(g["rmse_after"]) if g else "-", fmt(n["rmse_after"]) if n else "-", fmt(r["hidden_before"]),
            fmt(g["hidden_after"]) if g else "-", fmt(n["hidden_after"]) if n else "-"))
    lines += timing_section(os.path.join(out_dir, "time_denoising_4096.json"))
    with open(os.path.join(out_dir, "README.md"), "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--numpy", action="store_true", help="the true-flow rows alone, from the numpy restatement")
    ap.add_argument("--size", type=int, default=256, help="square frames of this side (default 256)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoising"), help="where README.md and table.jsonl go")
    args = ap.parse_args()
    numpy_rows = true_rows(True, args.size, args.seed)
    if args.numpy:
        rows = numpy_rows
    else:
        if flow2d.device_count() < 1:
            sys.exit("no HIP device: the GPU table needs the MI355X (--numpy runs the true-flow rows on the CPU)")
        rows = true_rows(False, args.size, args.seed) + computed_rows(args.size, args.seed)
    print("%-12s %5s %6s %6s %5s %-7s %-6s %8s %8s %8s %8s" % ("scene", "noise", "radius", "sigma", "masks", "flows", "engine",
                                                           "before", "after", "hid.bef", "hid.aft"))
    for r in rows:
        print("%-12s %5g %6d %6g %5s %-7s %-6s %8s %8s %8s %8s" % (
            r["scene"], r["noise"], r["radius"], r["range_sigma"], "on" if r["masks"] else "off", r["flows"], r["engine"],
            fmt(r["rmse_before"]), fmt(r["rmse_after"]), fmt(r["hidden_before"]), fmt(r["hidden_after"])))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "table.jsonl"), "w") as f:
        for r in ([] if args.numpy else rows) + numpy_rows:
            f.write(json.dumps(r) + "\n")
    write_readme(args.out, [] if args.numpy else rows, numpy_rows, args.size, args.seed)


if __name__ == "__main__":
    main()
