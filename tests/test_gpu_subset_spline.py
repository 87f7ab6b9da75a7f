"""flow2d_bspline_prefilter_2d, flow2d_subset_refine_spline_2d and flow2d_subset_refine2_spline_2d on the device against their numpy
restatement (tests/test_subset_spline_cpu.py).  The prefilter: every bit, in planes with a padded pitch and poisoned surroundings.
The refinements: by test_gpu_subset.compare's rule -- states and records exactly, the float planes within max(one fp32 ulp, 16 x
the spread of the restatement's three summation orders on that input); the kernels sum in the restatement's "butterfly" order, so
the bytes are expected to match and each case prints whether they did.  The layers above the entries are in
tests/test_gpu_subset_spline_host.py."""
import contextlib
import ctypes

import numpy as np
import pytest

import test_subset_spline_cpu as S
from test_correlate_cpu import F32, U32, bits, correlate_reference, frame_range, random_frames, scenes_module
from test_gpu_batch_kernels import Tall, pitch_of, stride_of
from test_gpu_multipass import POISON, padded, release
from test_gpu_subset import compare, speckle_case
from test_gpu_subset2 import OUT_NAMES, compare2
from test_gpu_wide_planes import (GRID_R, GRID_S, H as TALL_H, HIGH_LINE, LINE, W as TALL_W, below_the_line, node_bits, on_both, record_bytes,
                                  speckle_case as tall_speckle_case, subset_outputs, subsets_show_a_wrap, wrapped_rows_differ)
from test_subset_cpu import SUBSET_DTYPE, Refined, small_case
from test_subset_masked_cpu import all_orders_masked, random_mask

pytestmark = pytest.mark.gpu
F64 = np.float64
NAMES8 = ("u", "v", "ux", "uy", "vx", "vy", "score", "state")
_shared = {}


def shared(key, make):
    """A reference made once and shared (read-only)."""
    if key not in _shared:
        _shared[key] = make()
    return _shared[key]


def graph_calls(flow2d):
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    return lib


@contextlib.contextmanager
def captured(flow2d, ctx, call):
    """The graph of one call() on the context's stream."""
    lib = graph_calls(flow2d)
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    graph = ctypes.c_void_p()
    try:
        call()
    finally:
        assert lib.flow2d_capture_end(ctx.handle, ctypes.byref(graph)) == 0
    try:
        yield lambda: lib.flow2d_graph_launch(ctx.handle, graph)
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)


# ---- the prefilter ----------------------------------------------------------------------------------------------------------------------
def run_prefilter(ctx, a):
    """The coefficient bits of `a` from planes five columns wider and three rows taller: the source's padding NaN, the destination's
    poison, which must still be there."""
    h, w = a.shape
    src = padded(ctx, a)
    dst = ctx.plane(w + 5, h + 3).fill_bytes(0x7F)
    assert ctx.bspline_prefilter(src, w, h, out=dst) is dst
    ctx.synchronize()
    got = dst.download().view(U32)
    assert (got[h:] == POISON).all() and (got[:, w:] == POISON).all(), "written beyond the plane"
    assert np.array_equal(bits(src.download(w, h)), bits(a)), "the source was written"
    release(ctx, [src, dst])
    return got[:h, :w]


def plane_of(w, h, seed):
    return np.random.default_rng(seed).uniform(0, 255, (h, w)).astype(F32)


@pytest.mark.parametrize("w,h", [(5, 3), (1, 7), (7, 1), (67, 35), (130, 70)])
def test_prefilter_bits(flow2d, ctx, w, h):
    """5 x 3, 1 x 7 and 7 x 1 reflect more than once inside the halo; no tile size divides 67 x 35 and 130 x 70 (2 x 2 and 3 x 3
    workgroups)."""
    a = plane_of(w, h, 100 * w + h)
    got, want = run_prefilter(ctx, a), bits(S.bspline_prefilter_reference(a))
    print("%d x %d: %d of %d words differ" % (w, h, (got != want).sum(), want.size))
    assert np.array_equal(got, want)


def test_prefilter_of_a_nan_and_an_inf_pixel(flow2d, ctx):
    """Each is non-finite in exactly its 33 x 33 footprint (across a tile border: the pixels lie in different tiles), and every
    finite word is the restatement's."""
    a = plane_of(130, 70, 5)
    a[30, 60], a[50, 100] = np.nan, np.inf
    got = run_prefilter(ctx, a).view(F32)
    want = np.zeros(a.shape, bool)
    for y, x in ((30, 60), (50, 100)):
        want[max(y - 16, 0):y + 17, max(x - 16, 0):x + 17] = True
    assert np.array_equal(~np.isfinite(got), want)
    ref = S.bspline_prefilter_reference(a)
    assert np.array_equal(bits(got)[~want], bits(ref)[~want]) and np.array_equal(np.isnan(got), np.isnan(ref))


@pytest.mark.parametrize("kind", ["rows", "bytes"])
def test_prefilter_lock_step_batch_of_three(flow2d, ctx, kind):
    w, h, cw, ch, count = 67, 35, 72, 38, 3
    stride = stride_of(kind, pitch_of(cw), ch)
    planes = [plane_of(w, h, 40 + b) for b in range(count)]
    src, dst = Tall(ctx, cw, ch, count, stride).fill(planes), Tall(ctx, cw, ch, count, stride)
    with ctx.set_batch(count, stride):
        ctx.bspline_prefilter(src, w, h, out=dst)
    ctx.synchronize()
    dst.check([S.bspline_prefilter_reference(p) for p in planes], "coefficients (%s)" % kind)
    src.check(None, "the source")
    lib = flow2d.hip_lib()
    with ctx.set_batch(count, stride):  # a destination that meets a later instance of the source
        assert lib.flow2d_bspline_prefilter_2d(ctx.handle, src.ptr, src.ptr + 2 * stride, w, h, src.pitch) == 1
    release(ctx, [src.plane, dst.plane])


def test_prefilter_graph_replayed_twice(flow2d, ctx):
    a = plane_of(130, 70, 6)
    want = bits(S.bspline_prefilter_reference(a))
    src, dst = padded(ctx, a), ctx.plane(135, 73).fill_bytes(0x7F)
    with captured(flow2d, ctx, lambda: ctx.bspline_prefilter(src, 130, 70, out=dst)) as launch:
        for fill in (0x7F, 0x11):
            dst.fill_bytes(fill)
            assert launch() == 0
            ctx.synchronize()
            got = dst.download().view(U32)
            assert np.array_equal(got[:70, :130], want) and (got[70:] == U32(fill * 0x01010101)).all() and (got[:, 130:] == U32(fill * 0x01010101)).all()
    release(ctx, [src, dst])


def test_prefilter_refusals_write_nothing(flow2d, ctx):
    lib = flow2d.hip_lib()
    w, h = 67, 35
    src, dst = ctx.plane(w, h, plane_of(w, h, 1)), ctx.plane(w, h).fill_bytes(0x7F)
    bad = [(None, dst.ptr, w, h, src.pitch), (src.ptr, None, w, h, src.pitch), (src.ptr, dst.ptr, 0, h, src.pitch), (src.ptr, dst.ptr, w, 0, src.pitch),
           (src.ptr, dst.ptr, w, h, src.pitch + 8), (src.ptr, dst.ptr, w, h, 256), (src.ptr + 4, dst.ptr, w, h, src.pitch),
           (src.ptr, src.ptr, w, h, src.pitch), (dst.ptr + 16 * dst.pitch, dst.ptr, w, h - 16, src.pitch)]
    for args in bad:
        assert lib.flow2d_bspline_prefilter_2d(ctx.handle, *args) == 1, args
    assert lib.flow2d_bspline_prefilter_2d(None, src.ptr, dst.ptr, w, h, src.pitch) == 1
    ctx.synchronize()
    assert (dst.download().view(U32) == POISON).all()
    release(ctx, [src, dst])


def test_prefilter_on_planes_of_4_gib(flow2d, ctx):
    """100 x 4200 at a pitch of 1 MiB (bspline_prefilter_kernel<size_t>): the bytes of the run at a pitch of 512 bytes and the
    restatement's; the rows from 4096 on differ from the rows a 32-bit offset would wrap them onto.  Two tall planes.  A third run
    on planes just below 4 GiB (bspline_prefilter_kernel<unsigned> with byte offsets of 2^31 and more from row 2101 on): the same
    bytes, and the rows from 2101 on differ from rows 0 .. ."""
    f1 = tall_speckle_case()[1]
    want = shared("tall coefficients", lambda: S.bspline_prefilter_reference(tall_speckle_case()[1]))
    wrapped_rows_differ(f1, want)
    assert np.isfinite(want[LINE:]).all() and np.unique(want[LINE:]).size > 1000
    assert np.isfinite(want[HIGH_LINE:]).all() and np.unique(want[HIGH_LINE:LINE]).size > 1000

    def run(rig):
        src, dst = rig.load(f1), rig.out()
        ctx.bspline_prefilter(src, TALL_W, TALL_H, out=dst)
        ctx.synchronize()
        return dict(coefficients=dst.download(TALL_W, TALL_H).view(U32))

    got = on_both(ctx, 2, run)
    assert np.array_equal(got["coefficients"], bits(want))


# ---- the first-order refinement -----------------------------------------------------------------------------------------------------
def run_spline(ctx, f0, c1, start, mask, min_pixels, r, s, R, K=20, epsilon=1e-3, max_shift=4.0, max_gradient=0.5):
    """(the eight planes' bits, record bytes) of one flow2d_subset_refine_spline_2d call into poisoned outputs, which must stay
    poisoned beyond the grid; every plane lies in a container larger than its data, NaN beyond it.  start = (u0, v0) or the six."""
    h, w = f0.shape
    nh, nw = start[0].shape
    frames = [padded(ctx, f0), padded(ctx, c1)] + ([padded(ctx, mask)] if mask is not None else [])
    held = [padded(ctx, q) for q in start]
    outs = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(8)]
    rec = ctx.subset_records().fill_bytes(0x7F)
    ctx.subset_refine_spline(frames[0], frames[1], w, h, held[0], held[1], held[2:] if len(held) == 6 else None, nw, nh, r, s, R,
                             frames[2] if mask is not None else None, min_pixels, K, epsilon, max_shift, max_gradient, outs[0], outs[1], outs[2:6],
                             outs[6], outs[7], rec)
    ctx.synchronize()
    got = node_bits(outs, nw, nh)
    raw = rec.download(16, 1).tobytes()
    release(ctx, frames + held + outs + [rec])
    return got, raw


def spline_reference(f0, c1, start, mask, min_pixels, r, s, R, **kw):
    """(the restatement in the device's order, the spread of the three orders); mask None: the list is k itself."""
    with S.spline_sampler():
        if mask is None:
            mask, min_pixels = np.zeros(f0.shape, F32), (2 * R + 1) ** 2
        return all_orders_masked(f0, c1, start[0], start[1], start[2:] if len(start) == 6 else None, mask, min_pixels, r, s, R, **kw)


def check_spline(ctx, f0, f1, start, mask, min_pixels, r, s, R, what, **kw):
    c1 = S.bspline_prefilter_reference(f1)
    want, spread = spline_reference(f0, c1, start, mask, min_pixels, r, s, R, **kw)
    compare(run_spline(ctx, f0, c1, start, mask, min_pixels, r, s, R, **kw), want, spread, what)
    return want


def wide_case():
    """96 x 80 speckle with the grid (7, s 8), 99 nodes, and the starts flow2d_correlate_2d's restatement finds."""
    return shared("96x80", lambda: speckle_case(96, 80, 7, 8))


def start_gradients(shape, seed=11):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-0.01, 0.01, shape).astype(F32) for _ in range(4)]


def test_the_small_case(flow2d, ctx):
    f0, f1, u0, v0, r, s = small_case()
    want = check_spline(ctx, f0, f1, (u0, v0), None, 0, r, s, 3, "50x41, R = 3", max_shift=2.0)
    assert (want.state >= 1).sum() >= 20


@pytest.mark.parametrize("R", [1, 7, 11, 13, 15])
def test_the_radii(flow2d, ctx, R):
    """Four waves per workgroup up to R = 10, three at 11, two from 13; beyond R = 7 the border nodes' subsets leave frame 0."""
    f0, f1, u0, v0 = wide_case()
    want = check_spline(ctx, f0, f1, (u0, v0), None, 0, 7, 8, R, "96x80, R = %d" % R, max_shift=2.0)
    assert (want.state >= 1).sum() >= 40 and (int(want.record["strayed"][0]) >= 30) == (R > 7)


def test_start_gradients(flow2d, ctx):
    f0, f1, u0, v0 = wide_case()
    u0 = u0.copy()
    u0[3, 3], u0[4, 4] = np.nan, 1e30  # no input, strayed
    want = check_spline(ctx, f0, f1, [u0, v0] + start_gradients(u0.shape), None, 0, 7, 8, 7, "96x80 with start gradients")
    assert want.state[3, 3] == -1 and want.state[4, 4] == -3 and (want.state >= 1).sum() >= 60


def clamped_sample(coeff, x, y):
    """bspline_sample with the taps clamped to the frame, which is NOT the header's: what a clamped tap would give."""
    h, w = coeff.shape
    fx, fy = np.floor(x), np.floor(y)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    wx, wy = S.bspline_weights(x - fx), S.bspline_weights(y - fy)
    cols = [np.clip(ix - 1 + i, 0, w - 1) for i in range(4)]
    rows = []
    for j in range(4):
        row = np.clip(iy - 1 + j, 0, h - 1)
        a = [coeff[row, c] for c in cols]
        rows.append(((wx[0] * a[0] + wx[1] * a[1]) + wx[2] * a[2]) + wx[3] * a[3])
    return ((wy[0] * rows[0] + wy[1] * rows[1]) + wy[2] * rows[2]) + wy[3] * rows[3]


def edge_case():
    """95 x 79 with the grid (7, s 8): the first and the last subsets touch columns 0 and 94, rows 0 and 78.  Frame 1 is frame 0 and
    noise and the start is zero, so iteration 1 samples at X = 0 and X = width - 1 exactly: the taps -1 and `width` carry weight 1."""
    f0, f1 = random_frames(95, 79, seed=23, shift=(0, 0), noise=2.0)
    nw, nh = (95 - 15) // 8 + 1, (79 - 15) // 8 + 1
    assert 7 + (nw - 1) * 8 + 7 == 94 and 7 + (nh - 1) * 8 + 7 == 78
    zero = np.zeros((nh, nw), F32)
    return f0, f1, zero, zero


def test_subset_pixels_on_the_first_and_last_column_read_reflected_taps(flow2d, ctx):
    f0, f1, u0, v0 = edge_case()
    want = check_spline(ctx, f0, f1, (u0, v0), None, 0, 7, 8, 7, "95x79, subsets to the frame's edge", max_shift=2.0)
    # ... and a clamped tap would show: the restatement with clamped taps gives other words at refined border nodes of both sides
    c1 = S.bspline_prefilter_reference(f1)
    kept = [m.cubic_sample for m in S.RESTATEMENTS]
    try:
        for m in S.RESTATEMENTS:
            m.cubic_sample = clamped_sample
        clamped = all_orders_masked(f0, c1, u0, v0, None, np.zeros(f0.shape, F32), 225, 7, 8, 7, max_shift=2.0)[0]
    finally:
        for m, f in zip(S.RESTATEMENTS, kept):
            m.cubic_sample = f
    for column in (0, -1):
        live = want.state[:, column] >= 1
        assert live.any() and ((bits(want.u)[:, column] != bits(clamped.u)[:, column]) | (want.state[:, column] != clamped.state[:, column]))[live].all()
    inner = np.s_[1:-1, 1:-1]
    assert np.array_equal(bits(want.u)[inner], bits(clamped.u)[inner])


def test_a_random_mask(flow2d, ctx):
    f0, f1, u0, v0 = wide_case()
    mask = random_mask(f0.shape, 0.3, seed=5)
    want = check_spline(ctx, f0, f1, [u0, v0] + start_gradients(u0.shape), mask, 6, 7, 8, 7, "96x80, random mask")
    assert int(want.record["reserved"][0]) >= 20 and (want.state >= 1).sum() >= 5


def test_no_mask_and_a_zero_mask_give_the_same_bytes(flow2d, ctx):
    """mask = NULL runs the instantiation without the compaction, an all-zero mask the one with it."""
    f0, f1, u0, v0 = wide_case()
    c1 = S.bspline_prefilter_reference(f1)
    for R in (2, 7):
        none = run_spline(ctx, f0, c1, (u0, v0), None, -3, 7, 8, R)  # (min_pixels is not looked at)
        zero = run_spline(ctx, f0, c1, (u0, v0), np.zeros(f0.shape, F32), (2 * R + 1) ** 2, 7, 8, R)
        for name, a, b in zip(NAMES8, none[0], zero[0]):
            assert np.array_equal(a, b), name
        assert none[1] == zero[1] and int(np.frombuffer(none[1], SUBSET_DTYPE)["converged"][0]) >= 60


def test_the_raw_frame_in_place_of_the_coefficients_does_not_pass(flow2d, ctx):
    """The negative control: the comparison can fail."""
    f0, f1, u0, v0, r, s = small_case()
    want, spread = spline_reference(f0, S.bspline_prefilter_reference(f1), (u0, v0), None, 0, r, s, 3, max_shift=2.0)
    got = run_spline(ctx, f0, f1, (u0, v0), None, 0, r, s, 3, max_shift=2.0)
    with pytest.raises(AssertionError):
        compare(got, want, spread, "frame 1 itself")


def test_lock_step_batch_of_three(flow2d, ctx):
    """Three instances with the same frames, three masks and three starts: the bytes of each instance alone."""
    w, h, cw, ch, count, r, s, R = 96, 80, 104, 84, 3, 7, 8, 7
    stride = stride_of("rows", pitch_of(cw), ch)
    f0, f1, u0, v0 = wide_case()
    c1 = S.bspline_prefilter_reference(f1)
    zero = np.zeros_like(u0)
    masks = [random_mask(f0.shape, 0.3, seed=9), np.zeros(f0.shape, F32), random_mask(f0.shape, 0.1, seed=10)]
    starts = [[u0, v0, zero, zero, zero, zero], [u0, v0] + start_gradients(u0.shape), [u0.copy(), v0, zero, zero, zero, zero]]
    starts[2][0][2, 3] = np.nan
    nh, nw = u0.shape
    new = lambda: Tall(ctx, cw, ch, count, stride)  # noqa: E731
    t0, t1, tm = new().fill([f0]), new().fill([c1]), new().fill(masks)
    tin = [new().fill([st[k] for st in starts]) for k in range(6)]
    outs = [new() for _ in range(8)]
    rec = ctx.subset_records(count).fill_bytes(0x7F)
    with ctx.set_batch(count, stride):
        ctx.subset_refine_spline(t0, t1, w, h, tin[0], tin[1], tin[2:], nw, nh, r, s, R, tm, 20, out_u=outs[0], out_v=outs[1],
                                 out_gradients=outs[2:6], out_score=outs[6], out_state=outs[7], record=rec, instances=count)
    ctx.synchronize()
    alone = [run_spline(ctx, f0, c1, starts[b], masks[b], 20, r, s, R) for b in range(count)]
    for k, tall in enumerate(outs):
        tall.check([a[0][k].view(F32) for a in alone], NAMES8[k])
    for tall in [t0, t1, tm] + tin:
        tall.check(None, "inputs")
    raw = rec.download(16 * count, 1).tobytes()
    for b in range(count):
        assert raw[64 * b:64 * b + 64] == alone[b][1], "record of instance %d" % b
    # one instance against the restatement; a written range must not meet a later instance of the coefficients
    want, spread = spline_reference(f0, c1, starts[1], masks[1], 20, r, s, R)
    compare(alone[1], want, spread, "instance 1 alone")
    lib = flow2d.hip_lib()
    with ctx.set_batch(count, stride):
        assert lib.flow2d_subset_refine_spline_2d(ctx.handle, t0.ptr, t1.ptr, w, h, t0.pitch, tin[0].ptr, tin[1].ptr, None, None, None, None, nw, nh,
                                                  tin[0].pitch, r, s, R, 20, 1e-3, 4.0, 0.5, None, 0, t1.ptr + 2 * stride, outs[1].ptr, None, None,
                                                  None, None, None, None, None) == 1
    ctx.synchronize()
    release(ctx, [t.plane for t in [t0, t1, tm] + tin + outs] + [rec])


def test_a_graph_replayed_twice_gives_the_direct_calls_bytes(flow2d, ctx):
    """Prefilter and refinement captured together: the chain a host step queues."""
    f0, f1, u0, v0 = wide_case()
    h, w = f0.shape
    nh, nw = u0.shape
    p0, p1, pc = padded(ctx, f0), padded(ctx, f1), ctx.plane(w + 5, h + 3).fill_bytes(0x7F)
    held = [padded(ctx, u0), padded(ctx, v0)]
    outs = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(8)]
    rec = ctx.subset_records().fill_bytes(0x7F)

    def call():
        ctx.bspline_prefilter(p1, w, h, out=pc)
        ctx.subset_refine_spline(p0, pc, w, h, held[0], held[1], None, nw, nh, 7, 8, 7, out_u=outs[0], out_v=outs[1], out_gradients=outs[2:6],
                                 out_score=outs[6], out_state=outs[7], record=rec)

    def snapshot():
        ctx.synchronize()
        return [q.download().view(U32)[:nh, :nw].copy() for q in outs] + [rec.download(16, 1).tobytes()]

    call()
    direct = snapshot()
    want, spread = spline_reference(f0, S.bspline_prefilter_reference(f1), (u0, v0), None, 0, 7, 8, 7)
    compare((direct[:8], direct[8]), want, spread, "direct chain")
    with captured(flow2d, ctx, call) as launch:
        for fill in (0x7F, 0x11):
            for q in outs + [rec, pc]:
                q.fill_bytes(fill)
            assert launch() == 0
            for a, b in zip(snapshot(), direct):
                assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
            assert (outs[0].download().view(U32)[nh:] == U32(fill * 0x01010101)).all()
    release(ctx, [p0, p1, pc] + held + outs + [rec])


def test_refusals_on_a_real_context_write_nothing(flow2d, ctx):
    f0, f1, u0, v0 = wide_case()
    h, w = f0.shape
    nh, nw = u0.shape
    lib = flow2d.hip_lib()
    p0, pc, pm = ctx.plane(w, h, f0), ctx.plane(w, h, S.bspline_prefilter_reference(f1)), ctx.plane(w, h, np.zeros(f0.shape, F32))
    pin = [ctx.plane(nw, nh, q) for q in (u0, v0)]
    outs = [ctx.plane(nw, nh).fill_bytes(0x7F) for _ in range(8)]
    rec = ctx.subset_records().fill_bytes(0x7F)
    base = dict(c1=pc.ptr, mask=pm.ptr, min_pixels=57, record=rec.ptr, **{n: q.ptr for n, q in zip(NAMES8, outs)})

    def call(**kw):
        a = dict(base, **kw)
        return lib.flow2d_subset_refine_spline_2d(ctx.handle, p0.ptr, a["c1"], w, h, p0.pitch, pin[0].ptr, pin[1].ptr, None, None, None, None, nw, nh,
                                                  pin[0].pitch, 7, 8, 7, 20, 1e-3, 4.0, 0.5, a["mask"], a["min_pixels"], *[a[n] for n in NAMES8],
                                                  a["record"])

    bad = [dict(c1=None), dict(c1=pc.ptr + 4), dict(c1=outs[0].ptr), dict(record=pc.ptr), dict(min_pixels=5), dict(min_pixels=226), dict(ux=None),
           dict(v=outs[0].ptr), dict(mask=outs[3].ptr), dict(mask=None, c1=outs[2].ptr), dict(mask=None, vy=None)]
    if pc.pitch == pin[0].pitch:
        bad += [dict(u=pc.ptr + 16 * pc.pitch), dict(mask=None, state=pc.ptr)]
    for kw in bad:
        assert call(**kw) == 1, kw
    ctx.synchronize()
    for q in outs:
        assert (q.download().view(U32) == POISON).all()
    assert set(rec.download(16, 1).tobytes()) == {0x7F}
    assert call() == 0 and call(mask=None, min_pixels=-1) == 0  # ... and the same planes are accepted
    ctx.synchronize()
    release(ctx, [p0, pc, pm] + pin + outs + [rec])


def test_first_order_on_planes_of_4_gib(flow2d, ctx):
    """subset_refine_masked_kernel<size_t, BSpline, false> at R = 15: frame 0 and the coefficients in tall planes (two of them), and
    the <unsigned, BSpline, false> kernel on planes just below 4 GiB, where the subsets of the node rows 130 and 131 lie across the
    first row whose byte offset has bit 31 set."""
    R = 15
    f0, f1, u0, v0 = tall_speckle_case()
    nh, nw = u0.shape
    c1 = shared("tall coefficients", lambda: S.bspline_prefilter_reference(tall_speckle_case()[1]))
    want, spread = spline_reference(f0, c1, (u0, v0), None, 0, GRID_R, GRID_S, R)
    below = spline_reference(f0[:LINE], S.bspline_prefilter_reference(f1[:LINE]), (below_the_line(u0), below_the_line(v0)), None, 0, GRID_R, GRID_S, R)[0]
    subsets_show_a_wrap(want, R, f0, c1, below)

    def run(rig):
        p0, pc = rig.load(f0), rig.load(c1)
        start = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F).upload(a) for a in (u0, v0)]
        outs, rec = subset_outputs(ctx, nw, nh, 8)
        ctx.subset_refine_spline(p0, pc, TALL_W, TALL_H, start[0], start[1], None, nw, nh, GRID_R, GRID_S, R, None, None, 20, 1e-3, 4.0, 0.5, outs[0],
                                 outs[1], outs[2:6], outs[6], outs[7], rec)
        ctx.synchronize()
        got = dict(zip(NAMES8, node_bits(outs, nw, nh)), record=record_bytes(rec, 64))
        release(ctx, start + outs + [rec])
        return got

    got = on_both(ctx, 2, run)
    compare(([got[n] for n in NAMES8], got["record"]), want, spread, "100x4200 spline, R = 15, 4 GiB planes")


# ---- order 2 ------------------------------------------------------------------------------------------------------------------------
def run_spline2(ctx, f0, c1, u0, v0, r, s, R):
    h, w = f0.shape
    nh, nw = u0.shape
    frames = [padded(ctx, f0), padded(ctx, c1)]
    start = [padded(ctx, u0), padded(ctx, v0)]
    outs = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(14)]
    rec = ctx.subset_records().fill_bytes(0x7F)
    ctx.subset_refine2_spline(frames[0], frames[1], w, h, start[0], start[1], nw, nh, r, s, R, out_u=outs[0], out_v=outs[1], out_gradients=outs[2:6],
                              out_curvatures=outs[6:12], out_score=outs[12], out_state=outs[13], record=rec)
    ctx.synchronize()
    got = dict(zip(OUT_NAMES, node_bits(outs, nw, nh)))
    raw = rec.download(16, 1).tobytes()
    release(ctx, frames + start + outs + [rec])
    return got, raw


def bending_case():
    """The 4 x 3 corner of the grid (7, s 8) of the 96 x 80 "bend" scene, starts from flow2d_correlate_2d's restatement at d = 6."""
    def make():
        scene = scenes_module().make_speckle_bending("bend")
        lo, scale = frame_range(scene.frame_0, scene.frame_1)
        u0, v0, _, _, _ = correlate_reference(scene.frame_0, scene.frame_1, lo, scale, 7, 6, 8)
        return scene.frame_0, scene.frame_1, np.ascontiguousarray(u0[:3, :4]), np.ascontiguousarray(v0[:3, :4])
    return shared("bend", make)


@pytest.mark.parametrize("R", [2, 7, 15])
def test_order_2_on_the_bending_scene(flow2d, ctx, R):
    """Four waves per workgroup at R = 2 and 7, two at 15, where the nodes of the first row and column stray (R > r)."""
    f0, f1, u0, v0 = bending_case()
    c1 = S.bspline_prefilter_reference(f1)
    want, spread = S.all_orders2_spline(f0, c1, u0, v0, 7, 8, R)
    compare2(run_spline2(ctx, f0, c1, u0, v0, 7, 8, R), want, spread, "bend, 4 x 3 nodes, R = %d" % R)
    # (twenty-five pixels carry twelve unknowns badly: at R = 2 one node converges and the others stray after a few iterations)
    assert int(want.record["converged"][0]) >= {2: 1, 7: 8, 15: 3}[R] and int(want.record["iterations"][0]) >= 20
    if R == 7:
        assert want.state[2, 3] >= 1 and abs(float(want.uxy[2, 3]) - 0.004) < 0.002
        catmull = ctx.subset_refine2(*[padded(ctx, q) for q in (f0, f1)], 96, 80, padded(ctx, u0), padded(ctx, v0), 4, 3, 7, 8, R)
        assert not np.array_equal(bits(catmull[0]), bits(want.u))  # (the Catmull-Rom entry on the frame gives other words)


def test_order_2_lock_step_batch_of_three(flow2d, ctx):
    w, h, cw, ch, count, r, s, R = 130, 37, 140, 40, 3, 5, 6, 5
    stride = stride_of("rows", pitch_of(cw), ch)
    cases = [speckle_case(w, h, r, s, motion=m, seed=b) for b, m in enumerate(("affine", "translation", "affine"))]
    cases[1][2][1, 3] = np.nan  # a node without input in one instance only
    coeffs = [S.bspline_prefilter_reference(c[1]) for c in cases]
    nh, nw = cases[0][2].shape
    new = lambda: Tall(ctx, cw, ch, count, stride)  # noqa: E731
    t0, t1 = new().fill([c[0] for c in cases]), new().fill(coeffs)
    tu, tv = new().fill([c[2] for c in cases]), new().fill([c[3] for c in cases])
    outs = [new() for _ in range(14)]
    rec = ctx.subset_records(count).fill_bytes(0x7F)
    with ctx.set_batch(count, stride):
        ctx.subset_refine2_spline(t0, t1, w, h, tu, tv, nw, nh, r, s, R, out_u=outs[0], out_v=outs[1], out_gradients=outs[2:6],
                                  out_curvatures=outs[6:12], out_score=outs[12], out_state=outs[13], record=rec, instances=count)
    ctx.synchronize()
    alone = [run_spline2(ctx, c[0], k, c[2], c[3], r, s, R) for c, k in zip(cases, coeffs)]
    for name, tall in zip(OUT_NAMES, outs):
        tall.check([a[0][name].view(F32) for a in alone], name)
    for tall in (t0, t1, tu, tv):
        tall.check(None, "inputs")
    raw = rec.download(16 * count, 1).tobytes()
    for b in range(count):
        assert raw[64 * b:64 * b + 64] == alone[b][1], "record of instance %d" % b
    assert np.frombuffer(raw, SUBSET_DTYPE)["no_input"].tolist() == [0, 1, 0]
    want, spread = S.all_orders2_spline(cases[0][0], coeffs[0], cases[0][2], cases[0][3], r, s, R)
    compare2(alone[0], want, spread, "instance 0 alone")
    release(ctx, [t.plane for t in [t0, t1, tu, tv] + outs] + [rec])


def test_order_2_on_planes_of_4_gib(flow2d, ctx):
    """subset_refine2_kernel<size_t, BSpline>, R = 15.  Two tall planes; subset_refine2_kernel<unsigned, BSpline> on planes just below
    4 GiB."""
    R = 15
    f0, f1, u0, v0 = tall_speckle_case()
    nh, nw = u0.shape
    c1 = shared("tall coefficients", lambda: S.bspline_prefilter_reference(tall_speckle_case()[1]))
    want, spread = S.all_orders2_spline(f0, c1, u0, v0, GRID_R, GRID_S, R)
    below = S.all_orders2_spline(f0[:LINE], S.bspline_prefilter_reference(f1[:LINE]), below_the_line(u0), below_the_line(v0), GRID_R, GRID_S, R)[0]
    subsets_show_a_wrap(want, R, f0, c1, below)

    def run(rig):
        p0, pc = rig.load(f0), rig.load(c1)
        start = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F).upload(a) for a in (u0, v0)]
        outs, rec = subset_outputs(ctx, nw, nh, 14)
        ctx.subset_refine2_spline(p0, pc, TALL_W, TALL_H, start[0], start[1], nw, nh, GRID_R, GRID_S, R, out_u=outs[0], out_v=outs[1],
                                  out_gradients=outs[2:6], out_curvatures=outs[6:12], out_score=outs[12], out_state=outs[13], record=rec)
        ctx.synchronize()
        got = dict(zip(OUT_NAMES, node_bits(outs, nw, nh)), record=record_bytes(rec, 64))
        release(ctx, start + outs + [rec])
        return got

    got = on_both(ctx, 2, run)
    compare2(({n: got[n] for n in OUT_NAMES}, got["record"]), want, spread, "100x4200 spline second order, R = 15, 4 GiB planes")
