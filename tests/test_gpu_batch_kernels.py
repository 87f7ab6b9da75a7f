"""Every C-ABI launcher that honours flow2d_context_set_batch, held to the CPU oracle PER INSTANCE and bit for bit.

Layout of every case: one allocation per logical plane, `count` instances one below the other, each a cw x ch container
with the w x h level in its top-left corner, `stride` bytes apart, and a guard of one more stride behind the last one.
Strides: pitch * ch (contiguous), pitch * (ch + 3) (padding rows) and pitch * ch + 16 (no multiple of the pitch: every
instance starts 16 bytes further into a 256-byte line than the one before).  Outputs are poisoned with 0x7f bytes; after the
call the WHOLE allocation is compared as 32-bit words: each instance's rectangle is the oracle's result for that instance's
own inputs (every instance has its own seed), every other word -- container remainder, padding, guard -- is what it was.
Read-only inputs are compared with what was uploaded.  Then the batch is switched off and the same call must touch
instance 0 only.

Which test holds which entry of include/flow2d_c_abi.h (every FLOW2D_API function that takes a plane pointer):

  flow2d_add_2d, flow2d_add_2d_pair                      test_add, test_grid_z_at_large_counts (pair)
  flow2d_convolution_rows, flow2d_convolution_columns,
  flow2d_gaussian_blur                                   test_gaussian (radii 1..6 streamed, 9 and 24 on the tile branch)
  flow2d_median_2d, flow2d_median_2d_pair,
  flow2d_add_median_2d_pair                              test_median, test_grid_z_at_large_counts (pair, window 3)
  flow2d_registration_2d                                 test_registration, test_grid_z_at_large_counts
  flow2d_upsample_registration_2d                        test_upsample_registration (exact 2x, general ratio, coarsest form)
  flow2d_resample_x, flow2d_resample_y,
  flow2d_resample_x_pair, flow2d_resample_y_pair,
  flow2d_resample_xy_pair                                test_resample, test_grid_z_at_large_counts (x_pair, xy_pair)
  flow2d_resample_x_levels, flow2d_resample_y_levels     test_resample_levels (power-of-two and general scale)
  flow2d_compute_phi_ksi, flow2d_solve_2d,
  flow2d_solve_2d_grad, flow2d_solve_2d_grad_untiled,
  flow2d_solve_2d_sor                                    test_solver_pieces
  flow2d_solve_2d_log                                    test_solve_2d_log_against_the_reference_kernel (levels on the 16 x 8
                                                         grid), test_solve_2d_log_batch_equals_lone_calls (off it: the lone
                                                         call against the oracle fed the device's logarithms, the batch
                                                         against the lone call)
  flow2d_solve_level                                     test_solve_level, test_solve_level_auto_leaves_the_tiles_in_a_group,
                                                         test_solve_level_log_batch_equals_lone_calls (the LogDerivatives term:
                                                         as for flow2d_solve_2d_log)
  flow2d_memset_2d, flow2d_copy_d2d                      test_memset_2d, test_copy_d2d
  flow2d_consistency_2d, flow2d_interpolate_2d,
  flow2d_flow_error_2d                                   test_newest_entries_padded_strides (contiguous strides: their own files)
  flow2d_copy_h2d_2d, flow2d_copy_d2h_2d,
  flow2d_copy_planes                                     test_exceptions_act_as_without_a_batch (named as exceptions in the header)
  flow2d_track_points_2d, flow2d_seed_points_2d          FLOW2D_ERR_UNSUPPORTED under a batch: tests/test_tracking_cpu.py
  flow2d_plane_alloc, flow2d_plane_free                  no batch meaning; used under a batch by test_newest_entries_padded_strides

Not reached here: the branch of the fused strip launcher that launches a group instance by instance once a single pair's strips
reach 128 rows.  The planner only gives such strips to levels of about 4096 x 4096 and more, which is beyond the small planes
of this file; the lock-step pipeline tests of tests/test_gpu_flow.py run it at full size, and
tests/test_gpu_planning_cus.py::test_groups at 417 x 900 under the plan of an 8-CU device, per instance and with padded strides.
"""
import importlib

import numpy as np
import pytest
from numpy.lib.stride_tricks import as_strided

from conftest import in_container, level_fields
from test_bidirectional_cpu import consistency_reference
from test_flow_error_cpu import flow_error_reference
from test_interpolation_cpu import interpolation_reference

pytestmark = pytest.mark.gpu

F32 = np.float32
U32 = np.uint32
POISON = U32(0x7F7F7F7F)
# (level w, level h, container w, container h): the edges of test_gpu_kernels.py, and one size on the streaming strips
SIZES = [(100, 70, 128, 80), (5, 4, 40, 30), (257, 33, 300, 40), (16, 8, 16, 8)]
STRIPS = (700, 133, 704, 140)
COUNTS = (2, 3, 5)
STRIDES = ("contiguous", "rows", "bytes")
LAYOUTS = [(n, k) for n in COUNTS for k in STRIDES]
HX, HY = F32(1.25), F32(1.1)


def hip():
    return importlib.import_module("cuda-flow2d_amd").hip_lib()


def stride_of(kind, pitch, ch):
    return {"contiguous": pitch * ch, "rows": pitch * (ch + 3), "bytes": pitch * ch + 16}[kind]


def pitch_of(cw):
    return hip().flow2d_plane_pitch_bytes(cw)


class Tall:
    """`count` instances of a cw x ch container, `stride` bytes apart, in one device allocation that ends with a guard of one
    more stride; `host` mirrors what was uploaded, word for word.  Has the `ptr` / `pitch` the Context wrappers ask for."""

    def __init__(self, ctx, cw, ch, count, stride):
        self.ctx, self.cw, self.ch, self.count, self.stride = ctx, cw, ch, count, stride
        self.pitch = pitch_of(cw)
        assert stride % 16 == 0 and stride >= self.pitch * ch
        self.rows = -(-((count + 1) * stride) // self.pitch)
        self.plane = ctx.plane(cw, self.rows)
        assert self.plane.pitch == self.pitch
        self.ptr = self.plane.ptr
        self.host = np.full(self.rows * self.pitch // 4, POISON, U32)
        self.upload()

    def rects(self, flat, n=None):
        """(instances, ch, pitch) view of a mirror of the allocation."""
        return as_strided(flat, shape=(self.count if n is None else n, self.ch, self.pitch // 4), strides=(self.stride, self.pitch, 4))

    @staticmethod
    def _stack(arrays):
        return np.stack([np.ascontiguousarray(a, F32) for a in arrays]).view(U32)

    def fill(self, arrays, row=0, col=0):
        """Instance b gets arrays[b % len(arrays)] at (row, col) of its container."""
        a = self._stack(arrays)
        self.rects(self.host)[:, row:row + a.shape[1], col:col + a.shape[2]] = a[np.arange(self.count) % len(a)]
        return self.upload()

    def upload(self):
        rc = hip().flow2d_copy_h2d_2d(self.ctx.handle, self.ptr, self.pitch, self.host.ctypes.data, self.pitch, self.pitch, self.rows)
        assert rc == 0
        self.ctx.synchronize()
        return self

    def download(self):
        out = np.empty_like(self.host)
        rc = hip().flow2d_copy_d2h_2d(self.ctx.handle, out.ctypes.data, self.pitch, self.ptr, self.pitch, self.pitch, self.rows)
        assert rc == 0
        self.ctx.synchronize()
        return out

    def want(self, results, upto=None):
        """The mirror with the first `upto` (all) instances' rectangles replaced.  results: None, a list of level-sized arrays
        (one per instance, cycled), or a list of (arrays, row, col) regions."""
        flat = self.host.copy()
        if results is None:
            return flat
        n = self.count if upto is None else upto
        regions = results if isinstance(results[0], tuple) else [(results, 0, 0)]
        for arrays, row, col in regions:
            a = self._stack(arrays)
            self.rects(flat, n)[:, row:row + a.shape[1], col:col + a.shape[2]] = a[np.arange(n) % len(a)]
        return flat

    def check(self, results, what, upto=None, nan_equal=False, got=None):
        got = self.download() if got is None else got
        want = self.want(results, upto)
        same = got == want
        if nan_equal:  # NaNs that arithmetic produced: the payload is the processor's choice
            same |= np.isnan(got.view(F32)) & np.isnan(want.view(F32))
        if not same.all():
            bad = np.flatnonzero(~same)
            byte = int(bad[0]) * 4
            b, rest = divmod(byte, self.stride)
            pytest.fail("%s: %d words differ; first at byte %d = instance %d (of %d), row %d, column %d: got 0x%08x, want 0x%08x"
                        % (what, bad.size, byte, b, self.count, rest // self.pitch, rest % self.pitch // 4, got[bad[0]], want[bad[0]]))


def drive(ctx, count, stride, call, outputs, inputs=(), what="", lone=True):
    """The batched call: every output allocation word for word, the inputs unchanged; then, the batch switched off, the same
    call again: instance 0 only.  outputs: (Tall, results[, nan_equal])."""
    for out in outputs:
        out[0].upload()
    with ctx.set_batch(count, stride):
        call()
    ctx.synchronize()
    for out in outputs:
        out[0].check(out[1], what, nan_equal=len(out) > 2 and out[2])
    for t in inputs:
        t.check(None, what + ": an input")
    if not lone:
        return
    for out in outputs:
        out[0].upload()
    call()
    ctx.synchronize()
    for out in outputs:
        out[0].check(out[1], what + ", batch switched off", upto=1, nan_equal=len(out) > 2 and out[2])


def fields(oracle, w, h, count, seed):
    """Six lists (f0, f1, u, v, du, dv) of per-instance level-sized planes; every instance has its own seed."""
    per = []
    for b in range(count):
        f0, f1, u, v, du, dv = level_fields(oracle, w, h, 1000 * seed + b)
        rng = np.random.default_rng(7919 * seed + b)
        per.append(((f0 + rng.uniform(-1, 1, f0.shape)).astype(F32), f1, u, v, du, dv))
    return [list(q) for q in zip(*per)]


def talls(ctx, cw, ch, count, stride, n):
    return [Tall(ctx, cw, ch, count, stride) for _ in range(n)]


def rotate(*indices):
    return COUNTS[sum(indices) % len(COUNTS)]


# ---- element-wise ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,kind", LAYOUTS)
@pytest.mark.parametrize("w,h,cw,ch", SIZES)
def test_add(ctx, oracle, w, h, cw, ch, count, kind):
    """add_2d and add_2d_pair, in place: plane set a and plane set b of every instance independent of each other."""
    stride = stride_of(kind, pitch_of(cw), ch)
    a, b, c, d, _, _ = fields(oracle, w, h, count, 1)
    ta, tb, tc, td = (t.fill(x) for t, x in zip(talls(ctx, cw, ch, count, stride, 4), (a, b, c, d)))
    sum_ab = [oracle.add(x, y, w, h) for x, y in zip(a, b)]
    sum_cd = [oracle.add(x, y, w, h) for x, y in zip(c, d)]
    drive(ctx, count, stride, lambda: ctx.add(ta, tb, w, h), [(ta, sum_ab)], [tb], "add_2d")
    drive(ctx, count, stride, lambda: ctx.add_pair(ta, tb, tc, td, w, h), [(ta, sum_ab), (tc, sum_cd)], [tb, td], "add_2d_pair")


# ---- Gaussian -------------------------------------------------------------------------------------------------------------
SIGMAS = [0.45, 0.7, 1.0, 1.5, 1.9, 2.2, 3.0, 8.3]  # radii 1..6 stream; 9 and 24 take the tile kernel, one launch per instance


@pytest.mark.parametrize("kind", STRIDES)
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("w,h,cw,ch", SIZES + [STRIPS])
def test_gaussian(ctx, flow2d, oracle, w, h, cw, ch, sigma, kind):
    count = rotate(SIGMAS.index(sigma), (SIZES + [STRIPS]).index((w, h, cw, ch)))
    stride = stride_of(kind, pitch_of(cw), ch)
    src = fields(oracle, w, h, count, 2)[0]
    taps, r = flow2d.gaussian_kernel(sigma)
    assert r == int(3 * sigma)
    tsrc, dst = Tall(ctx, cw, ch, count, stride).fill(src), Tall(ctx, cw, ch, count, stride)
    drive(ctx, count, stride, lambda: ctx.convolution_rows(dst, tsrc, w, h, taps, r),
          [(dst, [oracle.convolution_rows(s, w, h, taps, r) for s in src])], [tsrc], "convolution_rows radius %d" % r)
    drive(ctx, count, stride, lambda: ctx.convolution_columns(dst, tsrc, w, h, taps, r),
          [(dst, [oracle.convolution_cols(s, w, h, taps, r) for s in src])], [tsrc], "convolution_columns radius %d" % r)
    drive(ctx, count, stride, lambda: ctx.gaussian_blur(dst, tsrc, w, h, taps, r),
          [(dst, [oracle.convolution(s, w, h, sigma) for s in src])], [tsrc], "gaussian_blur radius %d" % r)


# ---- median ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", STRIDES)
@pytest.mark.parametrize("window", [3, 5, 7])
@pytest.mark.parametrize("w,h,cw,ch", SIZES + [STRIPS])
def test_median(ctx, oracle, w, h, cw, ch, window, kind):
    """median_2d, median_2d_pair and add_median_2d_pair (one and two plane sets): (5, 4) runs the plain kernel for every window
    and (16, 8) for window 7, the other sizes the streaming kernels.  NaNs and negative zeros in instance 1 only: the windows
    redone in the reference's sort order must be that instance's."""
    count = rotate(window, (SIZES + [STRIPS]).index((w, h, cw, ch)))
    stride = stride_of(kind, pitch_of(cw), ch)
    _, _, u, v, du, dv = fields(oracle, w, h, count, 3)
    for b in range(count):
        u[b][::3, ::5] = 0.0  # ties
    rng = np.random.default_rng(w + window)
    u[1][rng.random((h, w)) < 0.05] = np.nan
    u[1][rng.random((h, w)) < 0.10] = -0.0
    u[1][0, 0] = np.nan
    v[1][h - 1, w - 1] = -0.0
    du[1][::2, 1::3] = -u[1][::2, 1::3]  # sums of +0
    du[1][rng.random((h, w)) < 0.03] = np.nan
    tu, tv, tdu, tdv = (t.fill(x) for t, x in zip(talls(ctx, cw, ch, count, stride, 4), (u, v, du, dv)))
    ou, ov = talls(ctx, cw, ch, count, stride, 2)
    med_u = [oracle.median(x, w, h, window) for x in u]
    med_v = [oracle.median(x, w, h, window) for x in v]
    drive(ctx, count, stride, lambda: ctx.median(tu, w, h, window, ou), [(ou, med_u)], [tu], "median_2d")
    drive(ctx, count, stride, lambda: ctx.median_pair(tu, tv, w, h, window, ou, ov), [(ou, med_u), (ov, med_v)], [tu, tv], "median_2d_pair")
    sum_u = [oracle.median(oracle.add(x, y, w, h), w, h, window) for x, y in zip(u, du)]
    sum_v = [oracle.median(oracle.add(x, y, w, h), w, h, window) for x, y in zip(v, dv)]
    drive(ctx, count, stride, lambda: ctx.add_median(tu, tdu, w, h, window, ou), [(ou, sum_u)], [tu, tdu], "add_median_2d_pair, one set")
    drive(ctx, count, stride, lambda: ctx.add_median(tu, tdu, w, h, window, ou, tv, tdv, ov), [(ou, sum_u), (ov, sum_v)],
          [tu, tdu, tv, tdv], "add_median_2d_pair, two sets")


# ---- warp -----------------------------------------------------------------------------------------------------------------
def wild_flow(u, v, w, h):
    """NaN and far out-of-range displacements (the warp falls back to frame 0 there)."""
    u[0, 0] = np.nan
    v[h - 1, w - 1] = 1e9
    u[h // 2, w // 2] = -1e9


@pytest.mark.parametrize("count,kind", LAYOUTS)
@pytest.mark.parametrize("w,h,cw,ch", SIZES)
def test_registration(ctx, oracle, w, h, cw, ch, count, kind):
    stride = stride_of(kind, pitch_of(cw), ch)
    f0, f1, u, v, _, _ = fields(oracle, w, h, count, 4)
    u, v = [(x * F32(4)).astype(F32) for x in u], [(x * F32(4)).astype(F32) for x in v]
    wild_flow(u[1], v[1], w, h)  # in one instance only
    planes = [t.fill(x) for t, x in zip(talls(ctx, cw, ch, count, stride, 4), (f0, f1, u, v))]
    out = Tall(ctx, cw, ch, count, stride)
    want = [oracle.registration(a, b, c, d, w, h, HX, HY) for a, b, c, d in zip(f0, f1, u, v)]
    drive(ctx, count, stride, lambda: ctx.registration(*planes, w, h, HX, HY, out), [(out, want)], planes, "registration_2d")


@pytest.mark.parametrize("kind", STRIDES)
@pytest.mark.parametrize("iw,ih,w,h,cw,ch", [(50, 35, 100, 70, 128, 80), (8, 4, 16, 8, 16, 8),        # exactly 2x
                                             (37, 20, 100, 70, 128, 80), (300, 40, 257, 33, 300, 40),  # any other ratio
                                             (2, 3, 16, 8, 16, 8)])
def test_upsample_registration(ctx, oracle, iw, ih, w, h, cw, ch, kind):
    """The previous level's flow resampled and frame 1 warped by it, in the exact-2x form, the general one and the coarsest
    level's (no previous flow: zeros over the level).  The resampled NaN of instance 1 is a NaN arithmetic made: its payload is
    not compared; everything else is."""
    count = rotate(iw, ih)
    stride = stride_of(kind, pitch_of(cw), ch)
    _, _, u, v, _, _ = fields(oracle, iw, ih, count, 5)
    u, v = [(x * F32(4)).astype(F32) for x in u], [(x * F32(4)).astype(F32) for x in v]
    wild_flow(u[1], v[1], iw, ih)
    f0, f1, _, _, _, _ = fields(oracle, w, h, count, 6)
    pu, pv, p0, p1 = (t.fill(x) for t, x in zip(talls(ctx, cw, ch, count, stride, 4), (u, v, f0, f1)))
    ou, ov, out = talls(ctx, cw, ch, count, stride, 3)
    up_u = [np.ascontiguousarray(oracle.resample(in_container(x, cw, ch), iw, ih, w, h)[:h, :w]) for x in u]
    up_v = [np.ascontiguousarray(oracle.resample(in_container(x, cw, ch), iw, ih, w, h)[:h, :w]) for x in v]
    want = [oracle.registration(a, b, c, d, w, h, HX, HY) for a, b, c, d in zip(f0, f1, up_u, up_v)]
    drive(ctx, count, stride, lambda: ctx.upsample_registration(pu, pv, iw, ih, ou, ov, p0, p1, w, h, HX, HY, out),
          [(ou, up_u, True), (ov, up_v, True), (out, want)], [pu, pv, p0, p1], "upsample_registration_2d")
    zeros = np.zeros((h, w), F32)
    still = [oracle.registration(a, b, zeros, zeros, w, h, HX, HY) for a, b in zip(f0, f1)]
    drive(ctx, count, stride, lambda: ctx.upsample_registration(None, None, 0, 0, ou, ov, p0, p1, w, h, HX, HY, out),
          [(ou, [zeros]), (ov, [zeros]), (out, still)], [p0, p1], "upsample_registration_2d, coarsest level")


# ---- resample -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", STRIDES)
@pytest.mark.parametrize("w,h,cw,ch", SIZES)
def test_resample(ctx, oracle, w, h, cw, ch, kind):
    """The single-plane, two-plane and one-launch forms: down-sampling by 2 and more (the x pass stages through LDS), by less
    than 2, and up-sampling."""
    stride = stride_of(kind, pitch_of(cw), ch)
    outs = [(w // 2, h // 2), (max(2, w // 9), max(2, h // 5)), (max(2, w * 4 // 5), max(2, h * 4 // 5)), (min(cw, w + 20), min(ch, h + 7))]
    for k, (ow, oh) in enumerate(outs):
        count = rotate(k, SIZES.index((w, h, cw, ch)))
        a, b, _, _, _, _ = fields(oracle, w, h, count, 7 + k)
        sa, sb = Tall(ctx, cw, ch, count, stride).fill(a), Tall(ctx, cw, ch, count, stride).fill(b)
        xa = [np.ascontiguousarray(oracle.resample_x(in_container(q, cw, ch), ow, h, w)[:h, :ow]) for q in a]
        xb = [np.ascontiguousarray(oracle.resample_x(in_container(q, cw, ch), ow, h, w)[:h, :ow]) for q in b]
        ya = [oracle.resample(in_container(q, cw, ch), w, h, ow, oh)[:oh, :ow] for q in a]
        yb = [oracle.resample(in_container(q, cw, ch), w, h, ow, oh)[:oh, :ow] for q in b]
        ta, tb = Tall(ctx, cw, ch, count, stride).fill(xa), Tall(ctx, cw, ch, count, stride).fill(xb)  # the x pass' result, for the y pass
        da, db = talls(ctx, cw, ch, count, stride, 2)
        tag = " %dx%d -> %dx%d" % (w, h, ow, oh)
        drive(ctx, count, stride, lambda: ctx.resample_x(sa, da, ow, h, w), [(da, xa)], [sa], "resample_x" + tag)
        drive(ctx, count, stride, lambda: ctx.resample_y(ta, da, ow, oh, h), [(da, ya)], [ta], "resample_y" + tag)
        drive(ctx, count, stride, lambda: ctx.resample_x_pair(sa, da, sb, db, ow, h, w), [(da, xa), (db, xb)], [sa, sb], "resample_x_pair" + tag)
        drive(ctx, count, stride, lambda: ctx.resample_y_pair(ta, da, tb, db, ow, oh, h), [(da, ya), (db, yb)], [ta, tb], "resample_y_pair" + tag)
        drive(ctx, count, stride, lambda: ctx.resample_xy(sa, da, w, h, ow, oh), [(da, ya)], [sa], "resample_xy_pair, one plane" + tag)
        drive(ctx, count, stride, lambda: ctx.resample_xy(sa, da, w, h, ow, oh, sb, db), [(da, ya), (db, yb)], [sa, sb], "resample_xy_pair" + tag)


@pytest.mark.parametrize("kind", STRIDES)
@pytest.mark.parametrize("w,h,scale,levels", [(256, 12, 0.5, 3), (1024, 64, 0.5, 6),  # every ratio a power of two: the register kernel
                                              (100, 70, 0.33, 3), (257, 40, 0.3, 3)])
def test_resample_levels(ctx, oracle, w, h, scale, levels, kind):
    """The x passes of all pyramid levels in one trip (every level's segment of the packed plane) and the y passes of all levels
    in one launch (every level's region of the output plane), for both planes, per instance."""
    count = rotate(w, levels)
    cw, ch = w, h + 2
    stride = stride_of(kind, pitch_of(cw), ch)
    widths = [int(np.ceil(F32(w) * F32(scale) ** F32(l))) for l in range(levels, 0, -1)]
    heights = [int(np.ceil(F32(h) * F32(scale) ** F32(l))) for l in range(levels, 0, -1)]
    columns, col, rows, row = [], 0, [], 0
    for lw, lh in zip(widths, heights):
        columns.append(col)
        col += (lw + 3) // 4 * 4
        rows.append(row)
        row += lh
    assert col <= pitch_of(cw) // 4 and row <= h
    a, b, _, _, _, _ = fields(oracle, w, h, count, 11)
    sa, sb = Tall(ctx, cw, ch, count, stride).fill(a), Tall(ctx, cw, ch, count, stride).fill(b)
    pa, pb, oa, ob = talls(ctx, cw, ch, count, stride, 4)
    seg_a = [([np.ascontiguousarray(oracle.resample_x(q, lw, h, w)[:, :lw]) for q in a], 0, c) for lw, c in zip(widths, columns)]
    seg_b = [([np.ascontiguousarray(oracle.resample_x(q, lw, h, w)[:, :lw]) for q in b], 0, c) for lw, c in zip(widths, columns)]
    drive(ctx, count, stride, lambda: ctx.resample_x_levels(sa, pa, w, h, widths, columns, sb, pb), [(pa, seg_a), (pb, seg_b)], [sa, sb],
          "resample_x_levels")
    drive(ctx, count, stride, lambda: ctx.resample_x_levels(sa, pa, w, h, widths, columns), [(pa, seg_a)], [sa], "resample_x_levels, one plane")
    for arrays, r0, c0 in seg_a:  # the packed planes of the y passes: the oracle's x passes
        pa.fill(arrays, r0, c0)
    for arrays, r0, c0 in seg_b:
        pb.fill(arrays, r0, c0)
    reg_a = [([np.ascontiguousarray(oracle.resample(q, w, h, lw, lh)[:lh, :lw]) for q in a], r, 0) for lw, lh, r in zip(widths, heights, rows)]
    reg_b = [([np.ascontiguousarray(oracle.resample(q, w, h, lw, lh)[:lh, :lw]) for q in b], r, 0) for lw, lh, r in zip(widths, heights, rows)]
    drive(ctx, count, stride, lambda: ctx.resample_y_levels(pa, oa, h, widths, heights, columns, rows, pb, ob), [(oa, reg_a), (ob, reg_b)],
          [pa, pb], "resample_y_levels")
    drive(ctx, count, stride, lambda: ctx.resample_y_levels(pa, oa, h, widths, heights, columns, rows), [(oa, reg_a)], [pa],
          "resample_y_levels, one plane")


# ---- solver pieces --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,kind", LAYOUTS)
@pytest.mark.parametrize("w,h,cw,ch", SIZES)
def test_solver_pieces(ctx, flow2d, oracle, w, h, cw, ch, count, kind):
    """compute_phi_ksi, one Jacobi sweep of solve_2d / solve_2d_grad / solve_2d_grad_untiled (one launch per instance on the
    host), and one red-black SOR iteration in place."""
    stride = stride_of(kind, pitch_of(cw), ch)
    per = fields(oracle, w, h, count, 13)
    d = [t.fill(x) for t, x in zip(talls(ctx, cw, ch, count, stride, 6), per)]
    phi, ksi, tdu, tdv = talls(ctx, cw, ch, count, stride, 4)
    coeff = [oracle.compute_phi_ksi(*q, w, h, HX, HY, 0.001, 0.001) for q in zip(*per)]
    ophi, oksi = [c[0] for c in coeff], [c[1] for c in coeff]
    drive(ctx, count, stride, lambda: ctx.compute_phi_ksi(*d, w, h, HX, HY, 0.001, 0.001, phi, ksi), [(phi, ophi), (ksi, oksi)], d,
          "compute_phi_ksi")
    phi.fill(ophi), ksi.fill(oksi)
    for constancy in (flow2d.GREY, flow2d.GRADIENT, flow2d.GRADIENT_UNTILED):
        sweeps = [oracle.solve_sweep(*q, p, k, w, h, HX, HY, 35.0, constancy) for q, p, k in zip(zip(*per), ophi, oksi)]
        drive(ctx, count, stride, lambda: ctx.solve_sweep(*d, phi, ksi, w, h, HX, HY, 35.0, tdu, tdv, constancy),
              [(tdu, [s[0] for s in sweeps]), (tdv, [s[1] for s in sweeps])], d + [phi, ksi], "sweep, constancy %d" % constancy)
        sor = [oracle.sor_iteration(*q, p, k, w, h, HX, HY, 35.0, 1.4, constancy) for q, p, k in zip(zip(*per), ophi, oksi)]
        drive(ctx, count, stride, lambda: ctx.sor_iteration(*d, phi, ksi, w, h, HX, HY, 35.0, 1.4, constancy),
              [(d[4], [s[0] for s in sor]), (d[5], [s[1] for s in sor])], d[:4] + [phi, ksi], "solve_2d_sor, constancy %d" % constancy)
        d[4].upload(), d[5].upload()  # (the increments as they were)


@pytest.fixture(scope="module")
def RK():
    from oracle import ref_kernels
    if not ref_kernels.available():
        # these tests only run where a HIP device is (-m gpu): there the prebuilt oracle/_ref must have travelled with the
        # snapshot.  A skip would let the pin to the reference's own kernels disappear without anybody noticing.
        pytest.fail("oracle/_ref holds no reference kernels: build them with `make -C oracle ref` where /root/reference "
                    "exists (python -c 'import __graft_entry__ as g; g.build()') and ship oracle/_ref with the snapshot")
    return ref_kernels


@pytest.mark.parametrize("count,kind", [(2, "rows"), (3, "bytes"), (5, "contiguous"), (3, "rows")])
@pytest.mark.parametrize("w,h,cw,ch", [(16, 8, 16, 8), (96, 64, 96, 64), (160, 72, 192, 80)])
def test_solve_2d_log_against_the_reference_kernel(ctx, flow2d, oracle, RK, w, h, cw, ch, count, kind):
    """The oracle takes log(I + 1) from the CPU's libm and is no bit-exact checker of solve_2d_log; the reference's own kernel
    is, on levels that are multiples of its 16 x 8 block: every instance against it, bit for bit."""
    stride = stride_of(kind, pitch_of(cw), ch)
    per = fields(oracle, w, h, count, 17)
    coeff = [oracle.compute_phi_ksi(*q, w, h, HX, HY, 0.001, 0.001) for q in zip(*per)]
    ophi, oksi = [c[0] for c in coeff], [c[1] for c in coeff]
    with RK.RefKernels(cw, ch) as R:
        ref = [R.sweep(RK.LOG_DERIVATIVES, *q, p, k, HX, HY, 35.0) for q, p, k in zip(zip(*per), ophi, oksi)]
    d = [t.fill(x) for t, x in zip(talls(ctx, cw, ch, count, stride, 8), per + [ophi, oksi])]
    tdu, tdv = talls(ctx, cw, ch, count, stride, 2)
    drive(ctx, count, stride, lambda: ctx.solve_sweep(*d, w, h, HX, HY, 35.0, tdu, tdv, flow2d.LOG_DERIVATIVES),
          [(tdu, [s[0] for s in ref]), (tdv, [s[1] for s in ref])], d, "solve_2d_log")


@pytest.mark.parametrize("count,kind", [(2, "rows"), (3, "bytes"), (5, "contiguous")])
@pytest.mark.parametrize("w,h,cw,ch", SIZES[:3])
def test_solve_2d_log_batch_equals_lone_calls(ctx, flow2d, oracle, w, h, cw, ch, count, kind):
    """Off the reference's 16 x 8 grid the reference's kernel is no checker (it reads a shared-memory slot no thread wrote
    there); the oracle is, once its log(I + 1) comes from the device (oracle.device_logs): the product's unbatched call on
    instance b's planes alone equals the oracle's sweep of instance b word for word, and instance b of the batched call
    equals that unbatched call, exactly."""
    stride = stride_of(kind, pitch_of(cw), ch)
    per = fields(oracle, w, h, count, 19)
    coeff = [oracle.compute_phi_ksi(*q, w, h, HX, HY, 0.001, 0.001) for q in zip(*per)]
    per = per + [[c[0] for c in coeff], [c[1] for c in coeff]]
    lone = []
    for b in range(count):
        one = [t.fill([x[b]]) for t, x in zip(talls(ctx, cw, ch, 1, pitch_of(cw) * ch, 8), per)]
        o_du, o_dv = talls(ctx, cw, ch, 1, pitch_of(cw) * ch, 2)
        ctx.solve_sweep(*one, w, h, HX, HY, 35.0, o_du, o_dv, flow2d.LOG_DERIVATIVES)
        ctx.synchronize()
        lone.append([o.rects(o.download())[0, :h, :w].view(F32).copy() for o in (o_du, o_dv)])
        with oracle.device_logs(ctx):
            want = oracle.solve_sweep(*[np.ascontiguousarray(x[b], F32) for x in per], w, h, HX, HY, 35.0, oracle.LOG_DERIVATIVES)
        for got, o in zip(lone[b], want):
            assert np.array_equal(got.view(np.uint32), o.view(np.uint32)), ("solve_2d_log against the oracle", b)
    d = [t.fill(x) for t, x in zip(talls(ctx, cw, ch, count, stride, 8), per)]
    tdu, tdv = talls(ctx, cw, ch, count, stride, 2)
    drive(ctx, count, stride, lambda: ctx.solve_sweep(*d, w, h, HX, HY, 35.0, tdu, tdv, flow2d.LOG_DERIVATIVES),
          [(tdu, [s[0] for s in lone]), (tdv, [s[1] for s in lone])], d, "solve_2d_log against lone calls")


# ---- the level loop -------------------------------------------------------------------------------------------------------
ITERATIONS = [(2, 3), (1, 7), (2, 0)]  # (1, 7): FUSED in chunks, the result handed back from the third plane pair
LEVEL_SIZES = [(100, 70, 128, 80), (52, 61, 64, 64)]
LEVEL_LAYOUTS = [(2, "contiguous"), (3, "rows"), (5, "bytes"), (3, "bytes"), (2, "rows"), (5, "contiguous"), (3, "contiguous")]


def level_supported(algorithm, w, h, inner, sor):
    """What include/flow2d_c_abi.h says each algorithm can run (flow2d_solver_algorithm, sor_omega)."""
    if algorithm == 2:
        return inner >= 1
    if algorithm == 3:
        return w <= 64 and h <= 64 and not sor
    if algorithm == 4:
        return 1 <= inner <= (2 if sor else 5)
    return True


def check_level(pair, other, scratch, results, w, h, ch, what, upto=None):
    """The pair *result_in_temp names: the oracle's level in every instance.  Outside the level rectangles nothing is written,
    with one exception the header states: flow_du / flow_dv may be zeroed over level width x container height.  Inside them the
    other planes hold intermediate increments and coefficients, which are nobody's contract."""
    for t, res in zip(pair, results):
        got = t.download()
        for b in range(t.count):
            below = t.rects(got)[b, h:ch, :w]
            if below.size and not below.any():
                below[...] = POISON
        t.check(res, what, upto=upto, got=got)
    for t in list(other) + list(scratch):
        got = t.download()
        want = t.want(None)
        loose = t.rects(want)
        loose[:, :h, :w] = t.rects(got)[:, :h, :w]
        for b in range(t.count):
            below = t.rects(got)[b, h:ch, :w]
            if below.size and not below.any():
                loose[b, h:ch, :w] = 0
        assert np.array_equal(got, want), what + ": a word outside the level rectangles was written"


def run_level(ctx, flow2d, oracle, w, h, cw, ch, count, kind, outer, inner, constancy, algorithm, omega):
    stride = stride_of(kind, pitch_of(cw), ch)
    f0, f1, u, v, _, _ = fields(oracle, w, h, count, 23)
    d = [t.fill(x) for t, x in zip(talls(ctx, cw, ch, count, stride, 4), (f0, f1, u, v))]
    written = talls(ctx, cw, ch, count, stride, 6)  # du, dv, phi, ksi, tdu, tdv
    x, y = Tall(ctx, cw, ch, count, stride).fill(u), Tall(ctx, cw, ch, count, stride).fill(v)
    what = "solve_level algorithm %d constancy %d %dx%d omega %g" % (algorithm, constancy, outer, inner, omega)

    def call():
        return ctx.solve_level(*d, *written, w, h, HX, HY, 3.5, 0.001, 0.001, outer, inner, constancy, algorithm, container_height=ch,
                               sor_omega=omega)

    with ctx.set_batch(count, stride):
        if level_supported(algorithm, w, h, inner, omega != 0.0):
            pair = call()
        else:
            with pytest.raises(flow2d.Flow2DError) as e:
                call()
            assert e.value.status == 5
            pair = None
        ctx.add(x, y, w, h)  # count and stride are still in force: every instance gets its sum
    ctx.synchronize()
    x.check([oracle.add(a, b, w, h) for a, b in zip(u, v)], what + ": add_2d behind it")
    if pair is None:
        return None
    if omega:
        want = [oracle.solve_level_sor(a, b, c, e, w, h, HX, HY, 3.5, 0.001, 0.001, outer, inner, omega, constancy) for a, b, c, e in zip(f0, f1, u, v)]
    else:
        want = [oracle.solve_level(a, b, c, e, w, h, HX, HY, 3.5, 0.001, 0.001, outer, inner, constancy)[:2] for a, b, c, e in zip(f0, f1, u, v)]
    results = [[q[0] for q in want], [q[1] for q in want]]
    du, dv, phi, ksi, tdu, tdv = written
    assert pair in ((du, dv), (tdu, tdv))
    other = (tdu, tdv) if pair[0] is du else (du, dv)
    check_level(pair, other, (phi, ksi), results, w, h, ch, what)
    for t in d:
        t.check(None, what + ": an input")
    for t in written:
        t.upload()
    pair = call()  # the batch switched off: instance 0 only
    ctx.synchronize()
    other = (tdu, tdv) if pair[0] is du else (du, dv)
    check_level(pair, other, (phi, ksi), results, w, h, ch, what + ", batch switched off", upto=1)
    for t in written:  # ... and really only instance 0
        got = t.download()
        assert (got[t.stride // 4:] == POISON).all(), what + ", batch switched off: a later instance was written"
    return pair[0] is tdu


@pytest.mark.parametrize("omega", [0.0, 1.4])
@pytest.mark.parametrize("outer,inner", ITERATIONS)
@pytest.mark.parametrize("constancy", [0, 1, 2])
@pytest.mark.parametrize("algorithm", [1, 2, 3, 4, 0])
@pytest.mark.parametrize("w,h,cw,ch", LEVEL_SIZES)
def test_solve_level(ctx, flow2d, oracle, w, h, cw, ch, algorithm, constancy, outer, inner, omega):
    """Every algorithm x data term x iteration counts x Jacobi / red-black SOR under a batch (the per-sweep, SOR and
    single-workgroup paths run instance by instance inside the library): the pair `*result_in_temp` names holds the oracle's
    level in every instance, nothing outside the levels is written, what the header says an algorithm cannot run is refused
    with FLOW2D_ERR_UNSUPPORTED, and either way the context is left in batch mode."""
    k = algorithm + 5 * constancy + 15 * ITERATIONS.index((outer, inner)) + (45 if omega else 0) + 3 * LEVEL_SIZES.index((w, h, cw, ch))
    count, kind = LEVEL_LAYOUTS[k % len(LEVEL_LAYOUTS)]
    in_temp = run_level(ctx, flow2d, oracle, w, h, cw, ch, count, kind, outer, inner, constancy, algorithm, omega)
    if in_temp is not None and algorithm == 1 and not omega:  # the reference's swap parity (cuda_operation_solve_2d.cpp:288-289)
        assert in_temp == ((outer * inner) % 2 == 1)
    if in_temp is not None and (algorithm == 3 or (algorithm == 1 and omega)):  # in place
        assert not in_temp


@pytest.mark.parametrize("constancy", [0, 1, 2])
@pytest.mark.parametrize("kind", STRIDES)
def test_solve_level_auto_leaves_the_tiles_in_a_group(ctx, flow2d, oracle, constancy, kind):
    """300 x 200 = 60 000 pixels: AUTO runs a single pair on the LDS tiles (<= 600^2), a group of three on the strips
    (60 000 x 3^2 is more).  Both are the oracle's bits; the timing record names the algorithm that ran."""
    w, h, cw, ch, count = 300, 200, 320, 208, 3
    ctx.timing_enable(1)
    run_level(ctx, flow2d, oracle, w, h, cw, ch, count, kind, 2, 3, constancy, flow2d.SOLVER_AUTO, 0.0)
    ctx.synchronize()
    used = [r.algorithm for r in ctx.timing_records()]
    assert used == [flow2d.SOLVER_FUSED, flow2d.SOLVER_TILED], used  # the group's call, then the lone one
    ctx.timing_enable(0)


_LONE_LOG_LEVELS = {}  # (algorithm, outer, inner, instance) -> (du, dv, result_in_temp) of the lone call, shared by the layouts


@pytest.mark.parametrize("omega", [0.0, 1.4])
@pytest.mark.parametrize("count,kind", [(3, "rows"), (2, "bytes")])
@pytest.mark.parametrize("outer,inner", ITERATIONS[:2])
@pytest.mark.parametrize("algorithm", [1, 2, 3, 4, 0])
def test_solve_level_log_batch_equals_lone_calls(ctx, flow2d, oracle, algorithm, outer, inner, count, kind, omega):
    """The level loop with the LogDerivatives term under a batch.  Every lone call equals the oracle's level word for word
    (the oracle's log(I + 1) taken from the device: oracle.device_logs), every instance of the group's call is the lone call
    on that instance's planes, bit for bit, *result_in_temp is the lone call's, and nothing outside the level rectangles is
    written (check_level).  The term has neither LDS tiles nor a red-black form: those requests are refused with
    FLOW2D_ERR_UNSUPPORTED and leave the context in batch mode."""
    w, h, cw, ch = LEVEL_SIZES[1]
    stride, lone_stride = stride_of(kind, pitch_of(cw), ch), pitch_of(cw) * ch
    f0, f1, u, v, _, _ = fields(oracle, w, h, count, 29)
    what = "solve_level, log term, algorithm %d %dx%d omega %g" % (algorithm, outer, inner, omega)

    def solve(planes, written):
        return ctx.solve_level(*planes, *written, w, h, HX, HY, 3.5, 0.001, 0.001, outer, inner, flow2d.LOG_DERIVATIVES, algorithm,
                               container_height=ch, sor_omega=omega)

    d = [t.fill(x) for t, x in zip(talls(ctx, cw, ch, count, stride, 4), (f0, f1, u, v))]
    written = talls(ctx, cw, ch, count, stride, 6)  # du, dv, phi, ksi, tdu, tdv
    if algorithm == 4 or omega:
        x, y = Tall(ctx, cw, ch, count, stride).fill(u), Tall(ctx, cw, ch, count, stride).fill(v)
        with ctx.set_batch(count, stride):
            with pytest.raises(flow2d.Flow2DError) as e:
                solve(d, written)
            assert e.value.status == 5
            ctx.add(x, y, w, h)  # count and stride are still in force: every instance gets its sum
        ctx.synchronize()
        x.check([oracle.add(a, b, w, h) for a, b in zip(u, v)], what + ": add_2d behind the refusal")
        return
    for b in range(count):  # (instance b's planes do not depend on the count: fields() seeds every instance by its index)
        if (algorithm, outer, inner, b) not in _LONE_LOG_LEVELS:
            one = [t.fill([x[b]]) for t, x in zip(talls(ctx, cw, ch, 1, lone_stride, 4), (f0, f1, u, v))]
            o = talls(ctx, cw, ch, 1, lone_stride, 6)
            pair = solve(one, o)
            ctx.synchronize()
            assert pair in ((o[0], o[1]), (o[4], o[5]))
            _LONE_LOG_LEVELS[algorithm, outer, inner, b] = tuple(t.rects(t.download())[0, :h, :w].view(F32).copy() for t in pair) + (pair[0] is o[4],)
            with oracle.device_logs(ctx):  # the lone call itself: the oracle's words, its log(I + 1) taken from the device
                want = oracle.solve_level(*[in_container(x[b], cw, ch) for x in (f0, f1, u, v)], w, h, HX, HY, 3.5, 0.001, 0.001, outer,
                                          inner, oracle.LOG_DERIVATIVES)[:2]
            for got, o_ in zip(_LONE_LOG_LEVELS[algorithm, outer, inner, b][:2], want):
                assert np.array_equal(got.view(U32), o_[:h, :w].view(U32)), what + ": lone call of instance %d against the oracle" % b
    lone = [_LONE_LOG_LEVELS[algorithm, outer, inner, b] for b in range(count)]
    with ctx.set_batch(count, stride):
        pair = solve(d, written)
    ctx.synchronize()
    du, dv, phi, ksi, tdu, tdv = written
    assert pair in ((du, dv), (tdu, tdv))
    in_temp = pair[0] is tdu
    assert [q[2] for q in lone] == [in_temp] * count, what + ": *result_in_temp of the group's call and of the lone calls"
    check_level(pair, (du, dv) if in_temp else (tdu, tdv), (phi, ksi), [[q[0] for q in lone], [q[1] for q in lone]], w, h, ch, what)
    for t in d:
        t.check(None, what + ": an input")


# ---- memory ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,kind", LAYOUTS)
@pytest.mark.parametrize("w,h,cw,ch", SIZES)
def test_memset_2d(ctx, w, h, cw, ch, count, kind):
    """flow2d_memset_2d: whole containers at the contiguous stride are ONE call (stride == pitch x height); every other stride,
    and a height below the container's, is a loop over the instances.  Rows narrower than the pitch, a width that is no whole
    number of floats; bytes outside untouched."""
    pitch = pitch_of(cw)
    stride = stride_of(kind, pitch, ch)
    t = Tall(ctx, cw, ch, count, stride)
    for width_bytes, height in ((4 * w, ch), (pitch, ch), (4 * w - 2, h), (pitch, h)):
        def call():
            assert hip().flow2d_memset_2d(ctx.handle, t.ptr, pitch, 0xA5, width_bytes, height) == 0
        for n in (count, 1):
            t.upload()
            with ctx.set_batch(n, stride if n > 1 else 0):
                call()
            ctx.synchronize()
            want = t.host.copy()
            as_strided(want.view(np.uint8), shape=(n, ch, pitch), strides=(stride, pitch, 1))[:, :height, :width_bytes] = 0xA5
            assert np.array_equal(t.download(), want), (width_bytes, height, n)


@pytest.mark.parametrize("count,kind", LAYOUTS)
@pytest.mark.parametrize("w,h,cw,ch", SIZES)
def test_copy_d2d(ctx, oracle, w, h, cw, ch, count, kind):
    """flow2d_copy_d2d: `bytes` bytes of every instance, nothing else."""
    pitch = pitch_of(cw)
    stride = stride_of(kind, pitch, ch)
    src = Tall(ctx, cw, ch, count, stride).fill(fields(oracle, w, h, count, 29)[2])
    dst = Tall(ctx, cw, ch, count, stride)
    for nbytes in (pitch * (h - 1) + 4 * w, pitch * ch, 16):
        for n in (count, 1):
            dst.upload()
            with ctx.set_batch(n, stride if n > 1 else 0):
                assert hip().flow2d_copy_d2d(ctx.handle, dst.ptr, src.ptr, nbytes) == 0
            ctx.synchronize()
            want = dst.host.copy()
            copied = as_strided(src.host.view(np.uint8), shape=(n, nbytes), strides=(stride, 1))
            as_strided(want.view(np.uint8), shape=(n, nbytes), strides=(stride, 1))[...] = copied
            assert np.array_equal(dst.download(), want), (nbytes, n)
            src.check(None, "copy_d2d: the source")


def test_exceptions_act_as_without_a_batch(ctx, flow2d, oracle):
    """What the header names as exceptions: flow2d_copy_h2d_2d / flow2d_copy_d2h_2d move exactly the region asked for and
    flow2d_copy_planes the planes its tables name, batch or no batch."""
    w, h, cw, ch, count = 100, 70, 128, 80, 3
    pitch = pitch_of(cw)
    stride = stride_of("rows", pitch, ch)
    data = fields(oracle, w, h, count, 31)[2]
    t, other = Tall(ctx, cw, ch, count, stride), Tall(ctx, cw, ch, count, stride)
    src = Tall(ctx, cw, ch, count, stride).fill(data)
    back = np.full((h + 2, w), POISON, U32)
    one = np.ascontiguousarray(data[0])
    with ctx.set_batch(count, stride):
        assert hip().flow2d_copy_h2d_2d(ctx.handle, t.ptr, pitch, one.ctypes.data, 4 * w, 4 * w, h) == 0
        assert hip().flow2d_copy_d2h_2d(ctx.handle, back.ctypes.data, 4 * w, src.ptr, pitch, 4 * w, h) == 0
        ctx.copy_planes([src], [other], w, h)
    ctx.synchronize()
    t.check([one], "copy_h2d_2d under a batch", upto=1)
    assert np.array_equal(back[:h], one.view(U32)) and (back[h:] == POISON).all()
    other.check([one], "copy_planes under a batch", upto=1)
    src.check(None, "the source")


# ---- the newest entries, at the two padded strides --------------------------------------------------------------------------
def flows_near(rng, w, h):
    t = rng.uniform(-6, 6, 2).astype(F32)
    u0 = (t[0] + rng.normal(0, 0.3, (h, w))).astype(F32)
    v0 = (t[1] + rng.normal(0, 0.3, (h, w))).astype(F32)
    u1 = (-t[0] + rng.normal(0, 0.3, (h, w))).astype(F32)
    v1 = (-t[1] + rng.normal(0, 0.3, (h, w))).astype(F32)
    for a in (u0, v0, u1, v1):
        wild = rng.random((h, w)) < 0.1
        a[wild] = rng.uniform(-40, 40, wild.sum())
        a[rng.random((h, w)) < 0.01] = np.nan
    return u0, v0, u1, v1


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("kind", ["rows", "bytes"])
@pytest.mark.parametrize("w,h,cw,ch", [(100, 70, 128, 80), (257, 33, 300, 40)])
def test_newest_entries_padded_strides(ctx, flow2d, w, h, cw, ch, kind, count):
    """flow2d_consistency_2d and flow2d_interpolate_2d against the numpy restatements of their definitions, bit for bit;
    flow2d_flow_error_2d: the EPE plane and every exact field of the record against the restatement of its definition, the AE
    plane and the double sums (which that restatement only meets within a tolerance) against the product's own lone call."""
    stride = stride_of(kind, pitch_of(cw), ch)
    rng = np.random.default_rng(w + count)
    cases = [flows_near(rng, w, h) for _ in range(count)]
    planes = [Tall(ctx, cw, ch, count, stride).fill([c[i] for c in cases]) for i in range(4)]
    out = Tall(ctx, cw, ch, count, stride)
    masks = [consistency_reference(*c, 0.02, 0.75).astype(F32) for c in cases]
    drive(ctx, count, stride, lambda: ctx.consistency(*planes, w, h, out, 0.02, 0.75), [(out, masks)], planes, "consistency_2d")

    frames = [[rng.uniform(0, 255, (h, w)).astype(F32) for _ in range(count)] for _ in range(2)]
    occ = [[(rng.random((h, w)) < 0.3).astype(F32) for _ in range(count)], [rng.uniform(-0.5, 1.5, (h, w)).astype(F32) for _ in range(count)]]
    occ[1][1][rng.random((h, w)) < 0.02] = np.nan
    tf = [Tall(ctx, cw, ch, count, stride).fill(q) for q in frames + occ]
    want = [interpolation_reference(frames[0][b], frames[1][b], *cases[b], 0.3, occ[0][b], occ[1][b], 2, 0.5) for b in range(count)]
    drive(ctx, count, stride, lambda: ctx.interpolate(tf[0], tf[1], *planes, w, h, 0.3, out, tf[2], tf[3], 2, 0.5), [(out, want)],
          planes + tf, "interpolate_2d")

    # flow error: estimate = forward flow, ground truth = minus the backward flow (with its NaNs: invalid pixels), a few sentinels
    gt = [[(-c[2]).astype(F32) for c in cases], [(-c[3]).astype(F32) for c in cases]]
    gt[0][0][::7, ::5] = 1e10
    tg = [Tall(ctx, cw, ch, count, stride).fill(q) for q in gt]
    epe, ae = talls(ctx, cw, ch, count, stride, 2)
    with ctx.set_batch(count, stride):
        records = ctx.flow_error(planes[0], planes[1], tg[0], tg[1], w, h, occlusion=tf[2], epe=epe, ae=ae, instances=count)
    ctx.synchronize()
    refs = [flow_error_reference(cases[b][0], cases[b][1], gt[0][b], gt[1][b], occ[0][b]) for b in range(count)]
    epe.check([r[1].astype(F32) for r in refs], "flow_error_2d: the EPE plane", nan_equal=True)
    lone_ae = []
    for b in range(count):
        got, ref = records[b], refs[b][0]
        assert got["invalid_ground_truth"] == ref["invalid_ground_truth"] and got["nonfinite_estimate"] == ref["nonfinite_estimate"], b
        for name in ("all", "noc", "occ"):
            for key in ("count", "above", "fl", "max_epe"):
                assert got[name][key] == ref[name][key], (b, name, key)
        one = [Tall(ctx, cw, ch, 1, pitch_of(cw) * ch).fill([q[b]]) for q in ([c[0] for c in cases], [c[1] for c in cases], gt[0], gt[1], occ[0])]
        l_epe, l_ae = talls(ctx, cw, ch, 1, pitch_of(cw) * ch, 2)
        lone = ctx.flow_error(one[0], one[1], one[2], one[3], w, h, occlusion=one[4], epe=l_epe, ae=l_ae, instances=1)[0]
        assert got == lone, b
        lone_ae.append(l_ae.rects(l_ae.download())[0, :h, :w].view(F32).copy())
    ae.check(lone_ae, "flow_error_2d: the AE plane against lone calls")
    for t in planes[:2] + tg + [tf[2]]:
        t.check(None, "flow_error_2d: an input")


# ---- grid.z = planes x count at counts that are not tiny ---------------------------------------------------------------------
@pytest.mark.parametrize("count,kind", [(257, "contiguous"), (257, "rows"), (257, "bytes"), (32767, "contiguous")])
def test_grid_z_at_large_counts(ctx, oracle, count, kind):
    """The launchers that put the batch into grid.z, with two planes (2 x 32767 = 65534 is the last grid.z the limit allows) and
    with one: a 16 x 8 level in a 16 x 8 container per instance.  The instances cycle through 7 distinct inputs -- coprime to
    every block size -- so the oracle runs 7 times and a wrong instance or plane index still shows; all instances and the guard
    are compared."""
    w, h, cw, ch, distinct = 16, 8, 16, 8, 7
    stride = stride_of(kind, pitch_of(cw), ch)
    f0, f1, u, v, du, dv = fields(oracle, w, h, distinct, 37)
    a, b, c, d = (Tall(ctx, cw, ch, count, stride).fill(x) for x in (u, du, v, dv))
    drive(ctx, count, stride, lambda: ctx.add_pair(a, b, c, d, w, h),
          [(a, [oracle.add(x, y, w, h) for x, y in zip(u, du)]), (c, [oracle.add(x, y, w, h) for x, y in zip(v, dv)])], [b, d],
          "add_2d_pair x %d" % count, lone=False)
    a.upload(), c.upload()
    oa, ob = talls(ctx, cw, ch, count, stride, 2)
    drive(ctx, count, stride, lambda: ctx.median_pair(a, c, w, h, 3, oa, ob),
          [(oa, [oracle.median(x, w, h, 3) for x in u]), (ob, [oracle.median(x, w, h, 3) for x in v])], [a, c],
          "median_2d_pair x %d" % count, lone=False)
    drive(ctx, count, stride, lambda: ctx.resample_x_pair(a, oa, c, ob, 6, h, w),
          [(oa, [np.ascontiguousarray(oracle.resample_x(x, 6, h, w)[:, :6]) for x in u]),
           (ob, [np.ascontiguousarray(oracle.resample_x(x, 6, h, w)[:, :6]) for x in v])], [a, c], "resample_x_pair x %d" % count, lone=False)
    drive(ctx, count, stride, lambda: ctx.resample_xy(a, oa, 9, 5, w, h, c, ob),
          [(oa, [oracle.resample(x, 9, 5, w, h) for x in u]), (ob, [oracle.resample(x, 9, 5, w, h) for x in v])], [a, c],
          "resample_xy_pair x %d" % count, lone=False)
    uu, vv = [(x * F32(3)).astype(F32) for x in u], [(x * F32(3)).astype(F32) for x in v]
    wild_flow(uu[3], vv[3], w, h)
    a.fill(uu), c.fill(vv)
    p0, p1 = Tall(ctx, cw, ch, count, stride).fill(f0), Tall(ctx, cw, ch, count, stride).fill(f1)
    drive(ctx, count, stride, lambda: ctx.registration(p0, p1, a, c, w, h, HX, HY, oa),
          [(oa, [oracle.registration(q0, q1, x, y, w, h, HX, HY) for q0, q1, x, y in zip(f0, f1, uu, vv)])], [p0, p1, a, c],
          "registration_2d x %d" % count, lone=False)
