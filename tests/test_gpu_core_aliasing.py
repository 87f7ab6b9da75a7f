"""The alias rule of the core entries of include/flow2d_c_abi.h -- the launchers of the reference's kernels and their fused forms --
and the footprint of their kernels, with every plane of a call carved out of ONE allocation.

One table (ROWS) names, for every core entry and variant, the planes it reads and the planes it writes.  Three tests walk it, each
at 100 x 70 in a 128 x 80 container (more than one workgroup, a partial one at both edges) and at 5 x 4 in a 40 x 30 container:

  test_refusals         every (written, read) and (written, written) pair: the written plane 16 bytes, a row, minus a row and all
                        rows but one into the other, and its base on the other's (where the entry is not in place); then, under
                        set_batch(3, stride) for the three stride kinds, one instance, two instances and minus one instance into
                        it.  Every placement returns FLOW2D_ERR_INVALID_ARGUMENT and, after synchronize, no word of the
                        allocation has changed.
  test_tightest_legal   the written plane exactly behind the read one's last row, exactly in front of its first, exactly count x
                        stride away under a batch, and interleaved A0 B0 A1 B1: FLOW2D_OK, every written plane holds the bytes of
                        the same call on separate allocations (which the other files hold to the oracle), and every other word --
                        rows between instances, pitch padding, the guard, the read planes -- is what was uploaded.  Everything
                        around the level rectangles is NaN bit patterns: a kernel that reads beyond its rows changes its output,
                        one that writes beyond its rectangle changes the mirror.
  test_in_place         the additions with operand_1 on operand_0 and the red-black iteration on flow_du / flow_dv against the
                        oracle; the same operand one row further on is refused.

test_tightest_legal_at_width_one repeats the second for the entries that take a single column, and
test_solve_level_counts_the_rows_it_zeroes holds flow2d_solve_level to the container_height rows its per-sweep path zeroes.
test_the_table_covers_the_core_section holds the table to the list of core entries in the header."""
import importlib
import os
import re
import zlib

import numpy as np
import pytest
from numpy.lib.stride_tricks import as_strided

from test_gpu_batch_kernels import POISON, Tall, hip, pitch_of, stride_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, U32 = np.float32, np.uint32
SIZES = [(100, 70, 128, 80), (5, 4, 40, 30)]
COUNT = 3
KINDS = ("contiguous", "rows", "bytes")
HX, HY = F32(1.25), F32(1.1)
INVALID_ARGUMENT = 1


def package():
    return importlib.import_module("cuda-flow2d_amd")


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def nan_words(n):
    """n NaN bit patterns, the payloads a hash of the word's index."""
    return (U32(0x7FC00000) | ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) >> np.uint64(7)).astype(U32) & U32(0x3FFFFF)).astype(U32)


_TAPS = {}


def taps_of(sigma):
    if sigma not in _TAPS:
        _TAPS[sigma] = package().gaussian_kernel(sigma)
    return _TAPS[sigma]


def status_of(call):
    try:
        call()
    except package().Flow2DError as e:
        return e.status
    return 0


# ---- one allocation, planes at byte offsets ----------------------------------------------------------------------------------------
class View:
    """A plane at a byte offset of a Block: the `ptr` / `pitch` the Context wrappers ask for."""

    def __init__(self, block, offset):
        assert offset % 16 == 0 and 0 <= offset < block.bytes
        self.ptr, self.pitch, self.offset = block.ptr + offset, block.pitch, offset


class Block:
    """One device allocation of at least `nbytes` bytes in rows of the pitch of a cw-wide container; `host` mirrors what was
    uploaded, word for word, and starts as NaN bit patterns."""

    def __init__(self, ctx, cw, nbytes):
        self.ctx, self.pitch = ctx, pitch_of(cw)
        self.rows = -(-nbytes // self.pitch)
        self.plane = ctx.plane(cw, self.rows)
        assert self.plane.pitch == self.pitch
        self.ptr, self.bytes = self.plane.ptr, self.rows * self.pitch
        self.host = nan_words(self.bytes // 4)

    def window(self, flat, offset, count, stride, rows):
        """(instances, rows, pitch) view of a mirror of the allocation: the plane at `offset`.  Nothing may lie outside."""
        assert offset % 4 == 0 and offset >= 0 and offset + (count - 1) * stride + rows * self.pitch <= self.bytes, "a plane leaves its allocation"
        return as_strided(flat[offset // 4:], shape=(count, rows, self.pitch // 4), strides=(stride, self.pitch, 4))

    def upload(self):
        assert hip().flow2d_copy_h2d_2d(self.ctx.handle, self.ptr, self.pitch, self.host.ctypes.data, self.pitch, self.pitch, self.rows) == 0
        self.ctx.synchronize()
        return self

    def download(self):
        out = np.empty_like(self.host)
        assert hip().flow2d_copy_d2h_2d(self.ctx.handle, out.ctypes.data, self.pitch, self.ptr, self.pitch, self.pitch, self.rows) == 0
        self.ctx.synchronize()
        return out

    def free(self):
        self.plane.free()
        self.ctx._planes.remove(self.plane)


# ---- the table ---------------------------------------------------------------------------------------------------------------------
class Row:
    """One entry in one variant.  reads / writes: the names of its planes (a plane worked on in place is written, and named in
    `inplace`).  call(ctx, P, g): the call on the planes P[name], g = (w, h, cw, ch); it may return the names of the written
    planes whose content is the entry's contract (default: all of them).  dims(name, g): columns and rows of a plane's level
    region (default w x h) -- the rows are the extent of its byte range.  regions(name, g): the rectangles (row, column, rows,
    columns) a written plane is written in (default: its level region).  identical: (written, read) pairs that may be one plane.
    sizes: which of SIZES the variant exists at, batch: whether the entry honours flow2d_context_set_batch -- with the reason
    where a case cannot exist."""

    def __init__(self, name, symbols, reads, writes, call, inplace=(), dims=None, regions=None, identical=(), sizes=(0, 1), batch=True,
                 reason=""):
        self.name, self.symbols, self.reads, self.writes, self.call = name, symbols.split(), list(reads), list(writes), call
        self.inplace, self.identical, self.sizes, self.batch, self.reason = set(inplace), set(identical), sizes, batch, reason
        self._dims, self._regions = dims, regions
        assert (sizes == (0, 1) and batch) or reason, "a case that is left out needs its reason"

    def planes(self):
        return self.reads + [n for n in self.writes if n not in self.reads]

    def dims(self, name, g):
        return self._dims(name, g) if self._dims and self._dims(name, g) else (g[0], g[1])

    def regions(self, name, g):
        if self._regions and self._regions(name, g):
            return self._regions(name, g)
        cols, rows = self.dims(name, g)
        return [(0, 0, rows, cols)]

    def data(self, name, g, instance):
        """What a read (or in-place) plane holds: frames in grey levels, coefficients positive, everything else around zero."""
        cols, rows = self.dims(name, g)
        rng = np.random.default_rng(zlib.crc32(("%s/%s" % (self.name, name)).encode()) + 7919 * instance)
        if name in ("f0", "f1"):
            return rng.uniform(0.0, 255.0, (rows, cols)).astype(F32)
        if name in ("phi", "ksi"):
            return rng.uniform(0.05, 2.0, (rows, cols)).astype(F32)
        return (rng.normal(0.0, 1.0, (rows, cols)) * (4.0 if name in ("u", "v") else 1.0)).astype(F32)


ROWS = []


def row(*args, **kwargs):
    ROWS.append(Row(*args, **kwargs))


def halves(n, least=2):
    """The sizes of a halving pyramid below n: 100 -> 50, 25, 13; 70 -> 35, 18, 9; 5 -> 3, 2; 4 -> 2."""
    out = []
    while len(out) < 3 and n > least:
        n = (n + 1) // 2
        out.append(n)
    return out


def columns_of(widths):
    out, col = [], 0
    for lw in widths:
        out.append(col)
        col += (lw + 3) // 4 * 4
    return out


def rows_of(heights):
    return [sum(heights[:k]) for k in range(len(heights))]


row("add", "flow2d_add_2d", ["b"], ["a"], lambda c, P, g: c.add(P["a"], P["b"], g[0], g[1]), inplace=["a"], identical=[("a", "b")])
row("add_pair", "flow2d_add_2d_pair", ["b", "d"], ["a", "c"], lambda c, P, g: c.add_pair(P["a"], P["b"], P["c"], P["d"], g[0], g[1]),
    inplace=["a", "c"], identical=[("a", "b"), ("c", "d")])
for n in (1, 3):
    row("copy_planes_%d" % n, "flow2d_copy_planes", ["s%d" % i for i in range(n)], ["d%d" % i for i in range(n)],
        lambda c, P, g, n=n: c.copy_planes([P["s%d" % i] for i in range(n)], [P["d%d" % i] for i in range(n)], g[0], g[1]), batch=False,
        reason="not subject to flow2d_context_set_batch (the header: its tables name every plane): under a batch it acts as without")
row("convolution_rows", "flow2d_convolution_rows", ["src"], ["dst"],
    lambda c, P, g: c.convolution_rows(P["dst"], P["src"], g[0], g[1], *taps_of(1.5)))
row("convolution_columns", "flow2d_convolution_columns", ["src"], ["dst"],
    lambda c, P, g: c.convolution_columns(P["dst"], P["src"], g[0], g[1], *taps_of(1.5)))
for sigma, kind in ((1.5, "streamed"), (8.3, "tiled")):
    row("gaussian_blur_%s" % kind, "flow2d_gaussian_blur", ["src"], ["dst"],
        lambda c, P, g, sigma=sigma: c.gaussian_blur(P["dst"], P["src"], g[0], g[1], *taps_of(sigma)))

# resample: `strong` takes the x pass' LDS kernel (in >= 2 out), `other` the plain one; the y pass has one kernel, two ratios
RATIOS = {"strong": lambda n: max(2, n * 2 // 5), "other": lambda n: max(2, n * 4 // 5)}
for tag, out_of in RATIOS.items():
    row("resample_x_" + tag, "flow2d_resample_x", ["src"], ["dst"],
        lambda c, P, g, f=out_of: c.resample_x(P["src"], P["dst"], f(g[0]), g[1], g[0]),
        dims=lambda name, g, f=out_of: (f(g[0]), g[1]) if name == "dst" else None)
    row("resample_y_" + tag, "flow2d_resample_y", ["src"], ["dst"],
        lambda c, P, g, f=out_of: c.resample_y(P["src"], P["dst"], g[0], f(g[1]), g[1]),
        dims=lambda name, g, f=out_of: (g[0], f(g[1])) if name == "dst" else None)
    row("resample_x_pair_" + tag, "flow2d_resample_x_pair", ["sa", "sb"], ["da", "db"],
        lambda c, P, g, f=out_of: c.resample_x_pair(P["sa"], P["da"], P["sb"], P["db"], f(g[0]), g[1], g[0]),
        dims=lambda name, g, f=out_of: (f(g[0]), g[1]) if name in ("da", "db") else None)
    row("resample_y_pair_" + tag, "flow2d_resample_y_pair", ["sa", "sb"], ["da", "db"],
        lambda c, P, g, f=out_of: c.resample_y_pair(P["sa"], P["da"], P["sb"], P["db"], g[0], f(g[1]), g[1]),
        dims=lambda name, g, f=out_of: (g[0], f(g[1])) if name in ("da", "db") else None)
XY = {"down": lambda g: (max(2, g[0] * 4 // 5), max(2, g[1] * 4 // 5)), "up": lambda g: (min(g[2], g[0] + 20), min(g[3], g[1] + 7))}
for tag, out_of in XY.items():
    row("resample_xy_" + tag, "flow2d_resample_xy_pair", ["sa"], ["da"],
        lambda c, P, g, f=out_of: c.resample_xy(P["sa"], P["da"], g[0], g[1], *f(g)), dims=lambda name, g, f=out_of: f(g) if name == "da" else None)
    row("resample_xy_pair_" + tag, "flow2d_resample_xy_pair", ["sa", "sb"], ["da", "db"],
        lambda c, P, g, f=out_of: c.resample_xy(P["sa"], P["da"], g[0], g[1], *f(g), P["sb"], P["db"]),
        dims=lambda name, g, f=out_of: f(g) if name in ("da", "db") else None)


def packed_regions(name, g):
    widths = halves(g[0])
    return [(0, col, g[1], lw) for lw, col in zip(widths, columns_of(widths))] if name in ("pa", "pb") else None


def packed_dims(name, g):
    widths = halves(g[0])
    return (columns_of(widths)[-1] + widths[-1], g[1]) if name in ("pa", "pb") else None


row("resample_x_levels", "flow2d_resample_x_levels", ["sa"], ["pa"],
    lambda c, P, g: c.resample_x_levels(P["sa"], P["pa"], g[0], g[1], halves(g[0]), columns_of(halves(g[0]))), dims=packed_dims, regions=packed_regions)
row("resample_x_levels_pair", "flow2d_resample_x_levels", ["sa", "sb"], ["pa", "pb"],
    lambda c, P, g: c.resample_x_levels(P["sa"], P["pa"], g[0], g[1], halves(g[0]), columns_of(halves(g[0])), P["sb"], P["pb"]), dims=packed_dims,
    regions=packed_regions)


def level_heights(g):
    return halves(g[1], 1)[:len(halves(g[0]))]


def level_dims(name, g):  # the packed planes are read with all their rows, the outputs written from their first to their last region row
    if name in ("pa", "pb"):
        return packed_dims(name, g)
    return (halves(g[0])[0], sum(level_heights(g))) if name in ("oa", "ob") else None


def level_regions(name, g):
    heights = level_heights(g)
    return [(r, 0, lh, lw) for lw, lh, r in zip(halves(g[0]), heights, rows_of(heights))] if name in ("oa", "ob") else None


def y_levels(c, P, g, pair):
    heights = level_heights(g)
    widths = halves(g[0])[:len(heights)]
    c.resample_y_levels(P["pa"], P["oa"], g[1], widths, heights, columns_of(halves(g[0]))[:len(heights)], rows_of(heights),
                        P["pb"] if pair else None, P["ob"] if pair else None)


row("resample_y_levels", "flow2d_resample_y_levels", ["pa"], ["oa"], lambda c, P, g: y_levels(c, P, g, False), dims=level_dims, regions=level_regions)
row("resample_y_levels_pair", "flow2d_resample_y_levels", ["pa", "pb"], ["oa", "ob"], lambda c, P, g: y_levels(c, P, g, True), dims=level_dims,
    regions=level_regions)

row("registration", "flow2d_registration_2d", ["f0", "f1", "u", "v"], ["out"],
    lambda c, P, g: c.registration(P["f0"], P["f1"], P["u"], P["v"], g[0], g[1], HX, HY, P["out"]))
PREVIOUS = {(100, 70): (37, 20), (5, 4): (2, 3)}  # the previous level of the general form


def upsample(c, P, g, previous, entry="upsample_registration"):
    getattr(c, entry)(P["u"], P["v"], previous[0], previous[1], P["ou"], P["ov"], P["f0"], P["f1"], g[0], g[1], HX, HY, P["out"])


row("upsample_registration", "flow2d_upsample_registration_2d", ["u", "v", "f0", "f1"], ["ou", "ov", "out"],
    lambda c, P, g: upsample(c, P, g, PREVIOUS[g[:2]]), dims=lambda name, g: PREVIOUS[g[:2]] if name in ("u", "v") else None)
DOUBLED = "an exactly doubled level has even sides: 100 x 70 from 50 x 35; 5 x 4 has none"
row("upsample_registration_doubled", "flow2d_upsample_registration_2d", ["u", "v", "f0", "f1"], ["ou", "ov", "out"],
    lambda c, P, g: upsample(c, P, g, (g[0] // 2, g[1] // 2)), dims=lambda name, g: (g[0] // 2, g[1] // 2) if name in ("u", "v") else None,
    sizes=(0,), reason=DOUBLED)
row("upsample_registration_coarsest", "flow2d_upsample_registration_2d", ["f0", "f1"], ["ou", "ov", "out"],
    lambda c, P, g: c.upsample_registration(None, None, 0, 0, P["ou"], P["ov"], P["f0"], P["f1"], g[0], g[1], HX, HY, P["out"]))
row("upsample_registration_half", "flow2d_upsample_registration_half_2d", ["u", "v", "f0", "f1"], ["ou", "ov", "out"],
    lambda c, P, g: upsample(c, P, g, (g[0] // 2, g[1] // 2), "upsample_registration_half"),
    dims=lambda name, g: (g[0] // 2, g[1] // 2) if name in ("u", "v", "ou", "ov") else None, sizes=(0,), reason=DOUBLED)

for window in (3, 5, 7):
    row("median%d" % window, "flow2d_median_2d", ["src"], ["dst"], lambda c, P, g, k=window: c.median(P["src"], g[0], g[1], k, P["dst"]))
    row("median%d_pair" % window, "flow2d_median_2d_pair", ["sa", "sb"], ["da", "db"],
        lambda c, P, g, k=window: c.median_pair(P["sa"], P["sb"], g[0], g[1], k, P["da"], P["db"]))
    row("add_median%d" % window, "flow2d_add_median_2d_pair", ["sa", "aa"], ["da"],
        lambda c, P, g, k=window: c.add_median(P["sa"], P["aa"], g[0], g[1], k, P["da"]))
    row("add_median%d_pair" % window, "flow2d_add_median_2d_pair", ["sa", "aa", "sb", "ab"], ["da", "db"],
        lambda c, P, g, k=window: c.add_median(P["sa"], P["aa"], g[0], g[1], k, P["da"], P["sb"], P["ab"], P["db"]))
    row("add_median%d_pair_half" % window, "flow2d_add_median_2d_pair_half", ["sa", "aa", "sb", "ab"], ["da", "db"],
        lambda c, P, g, k=window: c.add_median_half(P["sa"], P["aa"], g[0], g[1], k, P["da"], P["sb"], P["ab"], P["db"]),
        dims=lambda name, g: ((g[0] + 1) // 2, (g[1] + 1) // 2) if name in ("sa", "sb") else None)

SOLVER_READS = ["f0", "f1", "u", "v", "du", "dv"]
SWEEPS = {0: "flow2d_solve_2d", 1: "flow2d_solve_2d_grad", 2: "flow2d_solve_2d_grad_untiled", 3: "flow2d_solve_2d_log"}
row("compute_phi_ksi", "flow2d_compute_phi_ksi", SOLVER_READS, ["phi", "ksi"],
    lambda c, P, g: c.compute_phi_ksi(*[P[n] for n in SOLVER_READS], g[0], g[1], HX, HY, 0.001, 0.001, P["phi"], P["ksi"]))
for constancy, symbol in SWEEPS.items():
    row("sweep_constancy%d" % constancy, symbol, SOLVER_READS + ["phi", "ksi"], ["tdu", "tdv"],
        lambda c, P, g, k=constancy: c.solve_sweep(*[P[n] for n in SOLVER_READS + ["phi", "ksi"]], g[0], g[1], HX, HY, 35.0, P["tdu"], P["tdv"], k))
for constancy in (0, 1, 2):
    row("sor_constancy%d" % constancy, "flow2d_solve_2d_sor", ["f0", "f1", "u", "v", "phi", "ksi"], ["du", "dv"],
        lambda c, P, g, k=constancy: c.sor_iteration(*[P[n] for n in SOLVER_READS + ["phi", "ksi"]], g[0], g[1], HX, HY, 35.0, 1.4, k),
        inplace=["du", "dv"])
LEVEL_WRITES = ["du", "dv", "phi", "ksi", "tdu", "tdv"]


def solve_level(c, P, g, algorithm, constancy, inner):
    """(the level's rows are the container's: the zeroing of flow_du / flow_dv stays inside the level)"""
    pair = c.solve_level(*[P[n] for n in ["f0", "f1", "u", "v"] + LEVEL_WRITES], g[0], g[1], HX, HY, 3.5, 0.001, 0.001, 2, inner, constancy,
                         algorithm, container_height=g[1])
    return ("tdu", "tdv") if pair[0] is P["tdu"] else ("du", "dv")  # the other planes hold intermediates: nobody's contract


for algorithm in (1, 2, 4, 0):
    for constancy in (0, 1, 3):
        if (algorithm, constancy) == (4, 3):
            continue  # the tiles have no LogDerivatives term (flow2d_solver_algorithm_for: -1); AUTO and the strips run it below
        row("solve_level_algorithm%d_constancy%d" % (algorithm, constancy), "flow2d_solve_level", ["f0", "f1", "u", "v"], LEVEL_WRITES,
            lambda c, P, g, a=algorithm, k=constancy: solve_level(c, P, g, a, k, 3))
# AUTO with a single sweep per outer iteration: the one-workgroup solver at 5 x 4 (up to 64 x 32), the per-sweep kernels at 100 x 70
row("solve_level_auto_single_sweep", "flow2d_solve_level", ["f0", "f1", "u", "v"], LEVEL_WRITES, lambda c, P, g: solve_level(c, P, g, 0, 0, 1))
row("solve_level_one_workgroup", "flow2d_solve_level", ["f0", "f1", "u", "v"], LEVEL_WRITES, lambda c, P, g: solve_level(c, P, g, 3, 1, 3),
    sizes=(1,), reason="the one-workgroup solver takes levels up to 64 x 64: 5 x 4 only (100 x 70 is FLOW2D_ERR_UNSUPPORTED)")

# Core entries without a row, and why none can exist at the two sizes of this file.
WITHOUT_A_ROW = {
    "flow2d_resample_xy_levels": "eligible only for a width that is a multiple of 32 (FLOW2D_ERR_UNSUPPORTED before the planes are looked at): "
                                 "neither 100 nor 5; tests/test_gpu_resample_xy_levels.py holds its byte ranges and its surroundings",
}

CASES = [pytest.param(r, k, id="%s-%dx%d" % (r.name, SIZES[k][0], SIZES[k][1])) for r in ROWS for k in r.sizes]


# ---- placing, filling, comparing ---------------------------------------------------------------------------------------------------
def place(row, g, pitch, count, stride, moved=None, rows_of_slot=None):
    """Byte offsets of the row's planes in one allocation, and its size: every plane in a slot of its own, two instance strides from the
    slot's start and with four behind its last instance; moved = (name, other, delta): `name` at `other` + delta instead."""
    step = stride if count > 1 else (rows_of_slot or g[3]) * pitch
    span = (count - 1) * stride + (rows_of_slot or g[3]) * pitch
    slot = (span + 6 * step + 15) // 16 * 16
    offsets = {name: k * slot + 2 * step for k, name in enumerate(row.planes())}
    if moved:
        name, other, delta = moved
        assert -2 * step <= delta <= 4 * step
        offsets[name] = offsets[other] + delta
    return offsets, slot * len(row.planes())


def fill(row, g, block, offsets, count, stride):
    """The inputs' data (every instance its own) and POISON where a plane is written; NaN bit patterns stay everywhere else."""
    block.host = nan_words(block.bytes // 4)
    for name in row.planes():
        cols, rows = row.dims(name, g)
        window = block.window(block.host, offsets[name], count, stride, rows)
        if name in row.reads or name in row.inplace:
            for b in range(count):
                window[b, :rows, :cols] = bits(row.data(name, g, b))
        else:
            for r0, c0, nr, nc in row.regions(name, g):
                window[:, r0:r0 + nr, c0:c0 + nc] = POISON
    return block.upload()


def run(ctx, row, g, block, offsets, count, stride):
    """The row's call on the planes at `offsets`: (status, what the call returned)."""
    P = {name: View(block, offsets[name]) for name in row.planes()}
    for name in row.planes():  # every byte the entry may touch lies inside the allocation
        block.window(block.host, offsets[name], count, stride, row.dims(name, g)[1])
    result = []
    if count > 1:
        with ctx.set_batch(count, stride):
            status = status_of(lambda: result.append(row.call(ctx, P, g)))
    else:
        status = status_of(lambda: result.append(row.call(ctx, P, g)))
    return status, (result[0] if result else None)


_REFERENCES = {}


def reference(ctx, row, g, count):
    """The same call on separate allocations, one Tall per plane: {written plane: per instance, per region, the bits}, and the
    names of the planes that count.  Computed once per (row, size, count).  The surroundings here are Tall's POISON, a finite
    value, where the carved run has NaN bit patterns: a kernel that reads beyond its level on ANY side computes from different
    values in the two runs, whichever plane lies next to it."""
    key = (row.name, g, count)
    if key not in _REFERENCES:
        w, h, cw, ch = g
        stride = pitch_of(cw) * ch
        talls = {}
        for name in row.planes():
            t = talls[name] = Tall(ctx, cw, ch, count, stride)
            cols, rows = row.dims(name, g)
            if name in row.reads or name in row.inplace:
                t.fill([row.data(name, g, b) for b in range(count)])
            else:
                for r0, c0, nr, nc in row.regions(name, g):
                    t.rects(t.host)[:, r0:r0 + nr, c0:c0 + nc] = POISON
                t.upload()
        result = []
        with ctx.set_batch(count, stride):
            assert status_of(lambda: result.append(row.call(ctx, talls, g))) == 0, "%s: refused on separate allocations" % row.name
        ctx.synchronize()
        strict = result[0] or tuple(row.writes)
        got = {}
        for name in row.writes:
            rects = talls[name].rects(talls[name].download())
            got[name] = [[rects[b, r0:r0 + nr, c0:c0 + nc].copy() for r0, c0, nr, nc in row.regions(name, g)] for b in range(count)]
            outside = talls[name].rects(talls[name].download()).copy()
            for r0, c0, nr, nc in row.regions(name, g):
                outside[:, r0:r0 + nr, c0:c0 + nc] = talls[name].rects(talls[name].host)[:, r0:r0 + nr, c0:c0 + nc]
            assert np.array_equal(outside, talls[name].rects(talls[name].host)), "%s on separate allocations wrote outside %s" % (row.name, name)
        for name in row.reads:
            if name not in row.inplace:
                talls[name].check(None, "%s on separate allocations: the input %s" % (row.name, name))
        for t in talls.values():
            t.plane.free()
            ctx._planes.remove(t.plane)
        _REFERENCES[key] = got, strict
    return _REFERENCES[key]


def describe(row, g, block, offsets, count, stride, word):
    byte = word * 4
    for name in row.planes():
        for b in range(count):
            base = offsets[name] + b * stride
            if base <= byte < base + row.dims(name, g)[1] * block.pitch:
                return "row %d, column %d of instance %d of %s" % ((byte - base) // block.pitch, (byte - base) % block.pitch // 4, b, name)
    return "no plane's rows"


def check_legal(ctx, row, g, count, stride, moved, what, rows_of_slot=None):
    w, h, cw, ch = g
    pitch = pitch_of(cw)
    offsets, size = place(row, g, pitch, count, stride, moved, rows_of_slot)
    block = Block(ctx, cw, size)
    try:
        fill(row, g, block, offsets, count, stride)
        status, _ = run(ctx, row, g, block, offsets, count, stride)
        ctx.synchronize()
        assert status == 0, "%s: status %d for planes that share no byte" % (what, status)
        got = block.download()
        results, strict = reference(ctx, row, g, count)
        want = block.host.copy()
        for name in row.writes:
            cols, rows = row.dims(name, g)
            into, seen = block.window(want, offsets[name], count, stride, rows), block.window(got, offsets[name], count, stride, rows)
            for b in range(count):
                for (r0, c0, nr, nc), rect in zip(row.regions(name, g), results[name][b]):
                    into[b, r0:r0 + nr, c0:c0 + nc] = rect if name in strict else seen[b, r0:r0 + nr, c0:c0 + nc]
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            pytest.fail("%s: %d words differ from the call on separate allocations and the uploaded surroundings; first at byte %d (%s): "
                        "got 0x%08x, want 0x%08x" % (what, bad.size, int(bad[0]) * 4, describe(row, g, block, offsets, count, stride, int(bad[0])),
                                                     got[bad[0]], want[bad[0]]))
    finally:
        block.free()


def pairs_of(row):
    """Every (written, other) pair: the written planes against the read ones and against each other."""
    out = [(x, r) for x in row.writes for r in row.reads if r != x]
    return out + [(row.writes[i], row.writes[j]) for i in range(len(row.writes)) for j in range(i + 1, len(row.writes))]


def covering_pairs(row):
    """(written, read) pairs in which every written and every read plane occurs."""
    reads = [r for r in row.reads if r not in row.inplace]
    return [(row.writes[k % len(row.writes)], reads[k % len(reads)]) for k in range(max(len(row.writes), len(reads)))]


# ---- the tests ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,size", CASES)
def test_refusals(ctx, row, size):
    g = SIZES[size]
    w, h, cw, ch = g
    pitch = pitch_of(cw)
    layouts = [(1, pitch * ch, "no batch")] + ([(COUNT, stride_of(kind, pitch, ch), kind) for kind in KINDS] if row.batch else [])
    accepted, calls = [], 0
    for count, stride, kind in layouts:
        offsets, size_bytes = place(row, g, pitch, count, stride)
        block = Block(ctx, cw, size_bytes)
        fill(row, g, block, offsets, count, stride)
        for written, other in pairs_of(row):
            rows_written, rows_other = row.dims(written, g)[1], row.dims(other, g)[1]
            assert rows_written >= 2 and rows_other >= 2
            if count == 1:
                deltas = [16, pitch, -pitch, (rows_other - 1) * pitch] + ([] if (written, other) in row.identical else [0])
            else:
                deltas = [stride, 2 * stride, -stride]
            for delta in deltas:
                moved, _ = place(row, g, pitch, count, stride, (written, other, delta))
                status, _ = run(ctx, row, g, block, moved, count, stride)
                calls += 1
                if status != INVALID_ARGUMENT:
                    accepted.append("%s at %s %+d bytes (%s): status %d" % (written, other, delta, kind, status))
        ctx.synchronize()
        unchanged = np.array_equal(block.download(), block.host)
        block.free()
        assert not accepted, "%s: %d of %d placements were not refused: %s" % (row.name, len(accepted), calls, "; ".join(accepted[:12]))
        assert unchanged, "%s (%s): a refused call changed the allocation" % (row.name, kind)
    assert calls >= 4


@pytest.mark.parametrize("row,size", CASES)
def test_tightest_legal(ctx, row, size):
    tightest_legal(ctx, row, SIZES[size])


WIDTH_ONE = (1, 7, 40, 30)


@pytest.mark.parametrize("name", ["add", "gaussian_blur_streamed", "registration", "upsample_registration_coarsest"])
def test_tightest_legal_at_width_one(ctx, name):
    """One column: the bilinear sample of the warps reads the second column of its pair from the row's padding (NaN here, POISON
    in the run on separate allocations) and never selects it -- pitch_bytes covers that read, as the header says."""
    tightest_legal(ctx, next(r for r in ROWS if r.name == name), WIDTH_ONE)


def test_solve_level_counts_the_rows_it_zeroes(ctx):
    """The per-sweep path zeroes flow_du / flow_dv over level width x container_height: with a container higher than the level a
    plane between the level's last row and the container's is refused, read or written, and one exactly container_height rows
    behind is accepted, left as it was, and the level is the one of the call on separate allocations."""
    g = SIZES[0]
    w, h, cw, ch = g
    pitch = pitch_of(cw)
    row = next(r for r in ROWS if r.name == "solve_level_algorithm1_constancy0")
    names = ["f0", "f1", "u", "v"] + LEVEL_WRITES

    def call(P):
        return ctx.solve_level(*[P[n] for n in names], w, h, HX, HY, 3.5, 0.001, 0.001, 2, 3, 0, 1, container_height=ch)

    offsets, size = place(row, g, pitch, 1, pitch * ch)
    block = Block(ctx, cw, size)
    fill(row, g, block, offsets, 1, pitch * ch)
    for moved_plane in ("f0", "v", "phi", "tdv"):
        for zeroed in ("du", "dv"):
            for rows in (h, ch - 1):
                at, _ = place(row, g, pitch, 1, pitch * ch, (moved_plane, zeroed, rows * pitch))
                P = {n: View(block, at[n]) for n in names}
                assert status_of(lambda: call(P)) == INVALID_ARGUMENT, "%s %d rows behind %s, which is zeroed over %d" % (moved_plane, rows, zeroed, ch)
    ctx.synchronize()
    assert np.array_equal(block.download(), block.host), "a refused call changed the allocation"
    at, _ = place(row, g, pitch, 1, pitch * ch, ("f0", "du", ch * pitch))
    P = {n: View(block, at[n]) for n in names}
    block.window(block.host, at["f0"], 1, 0, h)[0, :, :w] = bits(row.data("f0", g, 0))
    block.upload()
    pair = call(P)
    ctx.synchronize()
    got = block.download()
    result = ("tdu", "tdv") if pair[0] is P["tdu"] else ("du", "dv")
    results, strict = reference(ctx, row, g, 1)
    assert result == tuple(strict)
    for n in result:
        assert np.array_equal(block.window(got, at[n], 1, 0, h)[0, :, :w], results[n][0][0]), "the level in " + n
    for n in ("f0", "f1", "u", "v"):
        assert np.array_equal(block.window(got, at[n], 1, 0, ch)[0], block.window(block.host, at[n], 1, 0, ch)[0]), "the input " + n
    for n in ("du", "dv"):  # rows h .. ch of the level's columns: zero (the memset) or untouched, nothing else
        below = block.window(got, at[n], 1, 0, ch)[0, h:, :w]
        assert not below.any() or np.array_equal(below, block.window(block.host, at[n], 1, 0, ch)[0, h:, :w])
    block.free()


def tightest_legal(ctx, row, g):
    w, h, cw, ch = g
    pitch = pitch_of(cw)
    for k, (written, read) in enumerate(covering_pairs(row)):
        rows_written, rows_read = row.dims(written, g)[1], row.dims(read, g)[1]
        tag = "%s, %s against %s" % (row.name, written, read)
        check_legal(ctx, row, g, 1, pitch * ch, (written, read, rows_read * pitch), tag + ": exactly behind its last row")
        check_legal(ctx, row, g, 1, pitch * ch, (written, read, -rows_written * pitch), tag + ": exactly in front of its first row")
        if not row.batch:
            continue
        kind = KINDS[k % len(KINDS)]
        stride = stride_of(kind, pitch, ch)
        check_legal(ctx, row, g, COUNT, stride, (written, read, COUNT * stride), tag + ": exactly count x stride behind it (%s)" % kind)
        # A0 B0 A1 B1 A2 B2: the written plane's instances between the read one's (no instance of any plane may meet the next one)
        tallest = max(row.dims(name, g)[1] for name in row.planes())
        between = max(rows_read + rows_written, tallest)
        check_legal(ctx, row, g, COUNT, between * pitch, (written, read, rows_read * pitch), tag + ": interleaved, stride %d rows" % between,
                    rows_of_slot=between)


@pytest.mark.parametrize("w,h,cw,ch", SIZES)
def test_in_place(ctx, oracle, w, h, cw, ch):
    g = (w, h, cw, ch)
    pitch = pitch_of(cw)
    add, add_pair = (next(r for r in ROWS if r.name == name) for name in ("add", "add_pair"))
    block = Block(ctx, cw, 8 * ch * pitch)
    x, y = add.data("a", g, 0), add.data("b", g, 1)
    block.window(block.host, 0, 1, 0, h)[0, :, :w] = bits(x)
    block.window(block.host, 4 * ch * pitch, 1, 0, h)[0, :, :w] = bits(y)
    block.upload()
    a, c = View(block, 0), View(block, 4 * ch * pitch)
    assert status_of(lambda: ctx.add(a, View(block, pitch), w, h)) == INVALID_ARGUMENT, "add_2d: operand_1 one row into operand_0"
    assert status_of(lambda: ctx.add_pair(a, a, c, View(block, 4 * ch * pitch + pitch), w, h)) == INVALID_ARGUMENT
    assert status_of(lambda: ctx.add_pair(a, View(block, pitch), c, c, w, h)) == INVALID_ARGUMENT
    ctx.synchronize()
    assert np.array_equal(block.download(), block.host), "a refused addition changed the allocation"
    ctx.add(a, a, w, h)
    ctx.synchronize()
    want = block.host.copy()
    block.window(want, 0, 1, 0, h)[0, :, :w] = bits(oracle.add(x, x, w, h))
    assert np.array_equal(block.download(), want), "add_2d with operand_1 on operand_0"
    block.upload()
    ctx.add_pair(a, a, c, c, w, h)
    ctx.synchronize()
    block.window(want, 4 * ch * pitch, 1, 0, h)[0, :, :w] = bits(oracle.add(y, y, w, h))
    assert np.array_equal(block.download(), want), "add_2d_pair with both operand_1 on their operand_0"
    block.free()

    sor = next(r for r in ROWS if r.name == "sor_constancy1")
    names = SOLVER_READS + ["phi", "ksi"]
    offsets, size = place(sor, g, pitch, 1, pitch * ch)
    block = Block(ctx, cw, size)
    fill(sor, g, block, offsets, 1, pitch * ch)
    P = {name: View(block, offsets[name]) for name in names}
    shifted = dict(P, dv=View(block, offsets["du"] + pitch))
    assert status_of(lambda: ctx.sor_iteration(*[shifted[n] for n in names], w, h, HX, HY, 35.0, 1.4, 1)) == INVALID_ARGUMENT
    ctx.sor_iteration(*[P[n] for n in names], w, h, HX, HY, 35.0, 1.4, 1)
    ctx.synchronize()
    du, dv = oracle.sor_iteration(*[sor.data(n, g, 0) for n in names], w, h, HX, HY, 35.0, 1.4, 1)
    want = block.host.copy()
    block.window(want, offsets["du"], 1, 0, h)[0, :, :w] = bits(du)
    block.window(want, offsets["dv"], 1, 0, h)[0, :, :w] = bits(dv)
    assert np.array_equal(block.download(), want), "solve_2d_sor in place on flow_du / flow_dv"
    block.free()


def core_entries():
    """The list the header's core section gives, checked against its declarations (parsed as tests/test_host_cpu.py does)."""
    header = open(os.path.join(ROOT, "include", "flow2d_c_abi.h")).read()
    declared = set(re.findall(r"FLOW2D_API\s+[\w\s\*]+?\b(flow2d_\w+)\s*\(", header))
    listed = re.search(r"The core entries:(.*?)\*/", header, re.S)
    assert listed, "include/flow2d_c_abi.h does not list its core entries"
    names = set(re.findall(r"flow2d_\w+", listed.group(1).split("Their alias rule", 1)[0]))
    assert names and names <= declared, "listed as core entries but not declared: %s" % sorted(names - declared)
    return names


# The files that hold the launchers of the reference's kernels, and what else they define: no plane, or a rule of its own.
CORE_SOURCES = ("pyramid_ops.hip", "median.hip", "solve.hip", "solve_level.hip")
NOT_A_CORE_ENTRY = {
    "flow2d_gaussian_kernel": "host arithmetic: taps into a host array, no device plane",
    "flow2d_half_base_flow_launches": "a process-wide counter",
    "flow2d_resample_xy_levels_launches": "a process-wide counter",
    "flow2d_log_frame_2d": "a checker's helper, not batch-aware; compares the extents of its two planes itself (tests/test_gpu_log_derivatives.py)",
    "flow2d_solver_algorithm_for": "host logic, no plane",
    "flow2d_solve_level_takes_half_base": "host logic, no plane",
    "flow2d_timing_enable": "timing records, no plane",
    "flow2d_timing_launch_filter": "timing records, no plane",
    "flow2d_timing_count": "timing records, no plane",
    "flow2d_timing_get": "timing records, no plane",
    "flow2d_timing_reset": "timing records, no plane",
}


def defined_in_the_core_sources():
    """Every C entry the four files define: a launcher added to one of them later is either listed in the header and given a row,
    or named above with its reason."""
    names = set()
    for source in CORE_SOURCES:
        text = open(os.path.join(ROOT, "cuda-flow2d_amd", "csrc", source)).read()
        names |= set(re.findall(r'^(?:extern "C" )?(?:int|unsigned long long|size_t|const char\*) (flow2d_\w+)\(', text, re.M))
    return names


def test_the_table_covers_the_core_section():
    covered = {s for r in ROWS for s in r.symbols} | set(WITHOUT_A_ROW)
    core = core_entries()
    defined = defined_in_the_core_sources()
    assert core == defined - set(NOT_A_CORE_ENTRY), "defined in %s but neither a core entry of the header nor excluded: %s; listed but not defined there: %s" % (
        ", ".join(CORE_SOURCES), sorted(defined - set(NOT_A_CORE_ENTRY) - core), sorted(core - defined))
    assert set(NOT_A_CORE_ENTRY) <= defined
    assert core == covered, "core entries without a row: %s; rows of no core entry: %s" % (sorted(core - covered), sorted(covered - core))
    assert not {s for r in ROWS for s in r.symbols} & set(WITHOUT_A_ROW)
    # ... and every variant the entries have: the windows, the data terms, the algorithms
    names = {r.name for r in ROWS}
    assert {"median%d%s" % (k, f) for k in (3, 5, 7) for f in ("", "_pair")} <= names
    assert {"add_median%d%s" % (k, f) for k in (3, 5, 7) for f in ("", "_pair", "_pair_half")} <= names
    assert {"solve_level_algorithm%d_constancy%d" % (a, k) for a in (1, 2, 4, 0) for k in (0, 1, 3)} - names == {"solve_level_algorithm4_constancy3"}
    assert package().hip_lib().flow2d_solver_algorithm_for(4, 100, 70, pitch_of(128), 2, 3, 3) == -1  # why that one has no row
