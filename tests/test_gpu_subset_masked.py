"""flow2d_subset_refine_masked_2d on the device against its numpy restatement (tests/test_subset_masked_cpu.py) in the device's
summation order ("butterfly" on the compacted list): every output plane, the state plane and the record byte for byte; each case
prints how many words differ before it asserts.  The layers above the entry are in tests/test_gpu_subset_masked_host.py.
96 x 80 frames with the grid (7, s 8), 99 nodes, for R = 1, 2, 7; a 40 x 36 frame with the grid (3, s 4) for the radii either side
of every change of the waves per workgroup (four up to R = 10, three at 11 and 12, two from 13) and R = 15.  Masks: none and all
zero (the bytes of flow2d_subset_refine_from_2d, from its kernel and from the new one), the specimen's, a seeded random one with 30
% excluded, blocks that leave fewer than 64 usable pixels, Nv at min_pixels and one below, everything excluded, NaN and Inf
entries.  Every plane lies in a container larger than its data, the mask's padding NaN."""
import ctypes

import numpy as np
import pytest

from test_correlate_cpu import F32, U32, bits, grid, scenes_module
from test_gpu_batch_kernels import Tall, pitch_of, stride_of
from test_gpu_multipass import POISON, padded, release
from test_gpu_subset_sequence import run_from
from test_subset_cpu import SUBSET_DTYPE, Refined
from test_subset_masked_cpu import (MASKED, block_mask, default_min_pixels, random_mask, specimen_case,
                                    subset_refine_masked_reference, usable_counts)
from test_subset_sequence_cpu import PLANES, predict_passes

pytestmark = pytest.mark.gpu


# ---- the call ---------------------------------------------------------------------------------------------------------------------------
def run_masked(ctx, f0, f1, start, mask, min_pixels, r, s, R, K=20, epsilon=1e-3, max_shift=4.0, max_gradient=0.5, gradients=True, record=True,
               score=True, state=True):
    """(the eight planes' bits -- None where absent --, record bytes) of one flow2d_subset_refine_masked_2d call into poisoned
    outputs, which must stay poisoned beyond the grid; start = (u0, v0, ux0, uy0, vx0, vy0) or (u0, v0); mask an array or None."""
    h, w = f0.shape
    nh, nw = start[0].shape
    frames = [padded(ctx, f0), padded(ctx, f1)] + ([padded(ctx, mask)] if mask is not None else [])
    held = [padded(ctx, q) for q in start]
    outs = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(8)]
    rec = ctx.subset_records().fill_bytes(0x7F)
    present = [True, True] + [gradients] * 4 + [score, state]
    ctx.subset_refine_masked(frames[0], frames[1], w, h, held[0], held[1], held[2:] if len(held) == 6 else None, nw, nh, r, s, R,
                             frames[2] if mask is not None else None, min_pixels, K, epsilon, max_shift, max_gradient, outs[0], outs[1],
                             outs[2:6] if gradients else None, outs[6] if score else None, outs[7] if state else None, rec if record else None)
    ctx.synchronize()
    got = [q.download().view(U32) for q in outs]
    for g, there in zip(got, present):
        if there:
            assert (g[nh:] == POISON).all() and (g[:, nw:] == POISON).all(), "written beyond the grid"
        else:
            assert (g == POISON).all(), "an absent plane was written"
    raw = rec.download(16, 1).tobytes()
    assert record or set(raw) == {0x7F}
    result = [g[:nh, :nw] if there else None for g, there in zip(got, present)], (raw if record else None)
    release(ctx, frames + held + outs + [rec])
    return result


def same_bytes(got, want, what):
    """The device's planes (bits) and record against the restatement `want` (a Refined), byte for byte."""
    planes, raw = got
    differ = {}
    for g, w_plane, name in zip(planes, want.planes(), Refined.NAMES):
        if g is not None:
            differ[name] = int((g != bits(w_plane)).sum())
    print("%s: words that differ %s; record %s" % (what, differ, np.frombuffer(raw, SUBSET_DTYPE).tolist() if raw else None))
    if planes[7] is not None:
        assert np.array_equal(planes[7], bits(want.state)), "%s: states %s, want %s" % (what, planes[7].view(F32), want.state)
    if raw is not None:
        assert raw == want.record.tobytes(), "%s: record %s, want %s" % (what, np.frombuffer(raw, SUBSET_DTYPE), want.record)
    assert not any(differ.values()), "%s: %s" % (what, differ)


def check_masked(ctx, f0, f1, start, mask, min_pixels, r, s, R, what, **kw):
    ref = {k: v for k, v in kw.items() if k in ("K", "epsilon", "max_shift", "max_gradient")}
    want = subset_refine_masked_reference(f0, f1, start[0], start[1], start[2:] if len(start) == 6 else None, mask, min_pixels, r, s, R, **ref)
    same_bytes(run_masked(ctx, f0, f1, start, mask, min_pixels, r, s, R, **kw), want, what)
    return want


def masked_count(want):
    return int(want.record["reserved"][0])


# ---- inputs, made once ------------------------------------------------------------------------------------------------------------------
_cases = {}


def wide():
    """96 x 80, grid (7, s 8): the stretched specimen, its mask and the restated chain's start (tests/test_subset_masked_cpu.py)."""
    scene, mask, u0, v0 = specimen_case("stretch")
    return scene.frame_0, scene.frame_1, mask, u0, v0


def small():
    """40 x 36, grid (3, s 4), 9 x 8 nodes: the specimen at that size, the start the truth rounded to whole pixels."""
    if "small" not in _cases:
        scene, mask = scenes_module().make_speckle_specimen("stretch", 40, 36, seed=0)
        nw, nh = grid(40, 36, 3, 4)
        cy, cx = 3 + np.arange(nh) * 4, 3 + np.arange(nw) * 4
        _cases["small"] = (scene.frame_0, scene.frame_1, mask, np.rint(scene.gt_u[np.ix_(cy, cx)]).astype(F32),
                           np.rint(scene.gt_v[np.ix_(cy, cx)]).astype(F32))
    return _cases["small"]


def second_step(R=7):
    """The six start planes of a second step on the wide case: the masked first step restated, through the prediction."""
    if ("second", R) not in _cases:
        f0, f1, mask, u0, v0 = wide()
        first = subset_refine_masked_reference(f0, f1, u0, v0, None, mask, default_min_pixels(R), 7, 8, R, max_shift=2.0)
        _cases["second", R] = predict_passes([getattr(first, n) for n in PLANES], first.state, 8)[0]
    return _cases["second", R]


# ---- the equivalences ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [2, 7])
def test_no_mask_and_a_zero_mask_give_the_plain_entrys_bytes(flow2d, ctx, R):
    """mask = NULL is forwarded; an all-zero mask runs the new kernel, whose list is then k itself: both give every byte of
    flow2d_subset_refine_from_2d on the same device, with and without start gradients, and those of the restatement."""
    f0, f1, _, u0, v0 = wide()
    u0 = u0.copy()
    u0[3, 3], u0[4, 4] = np.nan, 1e30  # no input, strayed
    for start in ((u0, v0), [u0, v0] + [q.copy() for q in second_step()[2:]]):
        plain = run_from(ctx, f0, f1, start, 7, 8, R)
        none = run_masked(ctx, f0, f1, start, None, -3, 7, 8, R)  # (min_pixels is not looked at)
        zero = run_masked(ctx, f0, f1, start, np.zeros(f0.shape, F32), (2 * R + 1) ** 2, 7, 8, R)
        for got in (none, zero):
            for name, a, b in zip(Refined.NAMES, got[0], plain[0]):
                assert np.array_equal(a, b), name
            assert got[1] == plain[1]
        want = subset_refine_masked_reference(f0, f1, start[0], start[1], start[2:] if len(start) == 6 else None, np.zeros(f0.shape, F32),
                                              (2 * R + 1) ** 2, 7, 8, R)
        same_bytes(zero, want, "all-zero mask, R = %d, %d start planes" % (R, len(start)))
        assert masked_count(want) == 0 and int(want.record["converged"][0]) >= 1


# ---- masks at 96 x 80 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 7])
def test_the_specimens_mask(flow2d, ctx, R):
    f0, f1, mask, u0, v0 = wide()
    want = check_masked(ctx, f0, f1, (u0, v0), mask, default_min_pixels(R), 7, 8, R, "specimen, R = %d" % R, max_shift=2.0)
    assert masked_count(want) >= 55 and (want.state >= 0).sum() >= 10


@pytest.mark.parametrize("R", [2, 7])
def test_a_random_mask_with_nan_and_inf_entries(flow2d, ctx, R):
    """30 % excluded at random (about a sixth of the pixels stays usable), some of them by NaN and +Inf; a start with gradients."""
    f0, f1, _, u0, v0 = wide()
    mask = random_mask(f0.shape, 0.3, seed=5)
    ones = np.argwhere(mask == 1)
    for k, (y, x) in enumerate(ones[::7]):
        mask[y, x] = (np.nan, np.inf, 0.5, 7.0)[k % 4]
    mask[mask == 0] = np.resize(np.array([0.0, -0.0, 0.49999997, -np.inf, 0.25], F32), int((mask == 0).sum()))
    start = second_step()
    want = check_masked(ctx, f0, f1, start, mask, 6, 7, 8, R, "random mask, R = %d" % R)
    nv = usable_counts(mask, 11, 9, 7, 8, R)
    assert masked_count(want) >= 20 and (want.state != MASKED).sum() >= 5 and (nv[want.state != MASKED] >= 6).all()


def test_blocks_with_fewer_than_64_pixels_and_nv_around_min_pixels(flow2d, ctx):
    """Everything excluded but a 9 x 9 block around node (4, 5) -- 49 usable pixels: fifteen lanes idle -- and an 8 x 10 block
    around node (2, 2), 48 usable ones.  min_pixels 48: both run; 49: Nv == min_pixels runs, one below is masked; 50: none runs."""
    f0, f1, _, u0, v0 = wide()
    mask = np.minimum(block_mask(f0.shape, 7 + 5 * 8, 7 + 4 * 8, 9, 9), block_mask(f0.shape, 7 + 2 * 8, 7 + 2 * 8, 8, 10))
    nv = usable_counts(mask, 11, 9, 7, 8, 7)
    assert nv[4, 5] == 49 and nv[2, 2] == 48
    for min_pixels, running in ((48, 2), (49, 1), (50, 0)):
        want = check_masked(ctx, f0, f1, (u0, v0), mask, min_pixels, 7, 8, 7, "blocks, min_pixels %d" % min_pixels, max_shift=2.0)
        assert masked_count(want) == 99 - running and (want.state[4, 5] != MASKED) == (running >= 1) and (want.state[2, 2] != MASKED) == (running == 2)
        assert (int(want.record["iterations"][0]) > 0) == (running > 0)


def test_everything_excluded(flow2d, ctx):
    f0, f1, _, u0, v0 = wide()
    u0 = u0.copy()
    u0[1, 1] = np.nan  # masked comes before no input
    want = check_masked(ctx, f0, f1, (u0, v0), np.ones(f0.shape, F32), 6, 7, 8, 7, "everything excluded")
    assert want.record.tolist() == [(99, 0, 0, 0, 0, 0, 0, 99)]


def test_optional_planes_absent(flow2d, ctx):
    f0, f1, mask, u0, v0 = wide()
    full = check_masked(ctx, f0, f1, (u0, v0), mask, 57, 7, 8, 7, "all planes", max_shift=2.0)
    for kw in (dict(gradients=False), dict(record=False, score=False), dict(gradients=False, record=False, score=False, state=False)):
        got = run_masked(ctx, f0, f1, (u0, v0), mask, 57, 7, 8, 7, max_shift=2.0, **kw)
        same_bytes(got, full, "absent: %s" % sorted(kw))


# ---- the radii around every change of the waves per workgroup -----------------------------------------------------------------------
@pytest.mark.parametrize("R", [10, 11, 12, 13, 15])
def test_the_large_radii(flow2d, ctx, R):
    """40 x 36: only the inner nodes' subsets lie inside frame 0, the others stray or are masked; the specimen's mask and a
    random one with 10 % excluded, so that a subset keeps a few hundred pixels."""
    f0, f1, mask, u0, v0 = small()
    want = check_masked(ctx, f0, f1, (u0, v0), mask, default_min_pixels(R), 3, 4, R, "40x36 specimen, R = %d" % R)
    assert (want.state >= 0).sum() >= 1 and masked_count(want) >= 6
    want = check_masked(ctx, f0, f1, (u0, v0), random_mask(f0.shape, 0.1, seed=R), 6, 3, 4, R, "40x36 random, R = %d" % R)
    assert (want.state >= 0).sum() >= 1 and int(want.record["strayed"][0]) >= 20


# ---- the same bytes: a lock-step batch, a replayed graph ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["contiguous", "rows"])
def test_lock_step_batch_of_three_with_three_masks(flow2d, ctx, kind):
    """Three instances `stride` apart with the same frames and three different masks and starts: planes and records of instance b
    are the bytes of that instance alone, and every other word of the allocations is what it was."""
    w, h, cw, ch, count, r, s, R = 96, 80, 104, 84, 3, 7, 8, 7
    stride = stride_of(kind, pitch_of(cw), ch)
    f0, f1, mask, u0, v0 = wide()
    zero = np.zeros_like(u0)
    masks = [mask, random_mask(f0.shape, 0.3, seed=9), np.zeros(f0.shape, F32)]
    starts = [[u0, v0, zero, zero, zero, zero], second_step(), [u0.copy(), v0, zero, zero, zero, zero]]
    starts[2][0][2, 3] = np.nan  # a node without input in one instance only
    nh, nw = u0.shape
    new = lambda: Tall(ctx, cw, ch, count, stride)  # noqa: E731
    t0, t1, tm = new().fill([f0]), new().fill([f1]), new().fill(masks)
    tin = [new().fill([st[k] for st in starts]) for k in range(6)]
    outs = [new() for _ in range(8)]
    rec = ctx.subset_records(count).fill_bytes(0x7F)
    with ctx.set_batch(count, stride):
        ctx.subset_refine_masked(t0, t1, w, h, tin[0], tin[1], tin[2:], nw, nh, r, s, R, tm, 20, out_u=outs[0], out_v=outs[1],
                                 out_gradients=outs[2:6], out_score=outs[6], out_state=outs[7], record=rec, instances=count)
    ctx.synchronize()
    alone = [run_masked(ctx, f0, f1, starts[b], masks[b], 20, r, s, R) for b in range(count)]
    for k, tall in enumerate(outs):
        tall.check([a[0][k].view(F32) for a in alone], "%s (%s)" % (Refined.NAMES[k], kind))
    for tall in [t0, t1, tm] + tin:
        tall.check(None, "inputs")
    raw = rec.download(16 * count, 1).tobytes()
    for b in range(count):
        assert raw[64 * b:64 * b + 64] == alone[b][1], "record of instance %d" % b
    records = np.frombuffer(raw, SUBSET_DTYPE)
    assert records["reserved"][0] == 55 and records["reserved"][1] >= 20 and records["reserved"][2] == 0
    assert records["no_input"][0] == 0 and records["no_input"][2] == 1
    # a written range must not meet a later instance of the mask
    lib = flow2d.hip_lib()
    with ctx.set_batch(count, stride):
        assert lib.flow2d_subset_refine_masked_2d(ctx.handle, t0.ptr, t1.ptr, w, h, t0.pitch, tin[0].ptr, tin[1].ptr, tin[2].ptr, tin[3].ptr,
                                                  tin[4].ptr, tin[5].ptr, nw, nh, tin[0].pitch, r, s, R, 20, 1e-3, 4.0, 0.5, tm.ptr, 20,
                                                  tm.ptr + 2 * stride, outs[1].ptr, None, None, None, None, None, None, None) == 1
    ctx.synchronize()
    for k, tall in enumerate(outs):
        tall.check([a[0][k].view(F32) for a in alone], "after the refusal")


def test_a_graph_replayed_twice_gives_the_direct_calls_bytes(flow2d, ctx):
    w, h, r, s, R = 96, 80, 7, 8, 7
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    f0, f1, mask, _, _ = wide()
    start = second_step()
    nh, nw = start[0].shape
    frames = [padded(ctx, f0), padded(ctx, f1), padded(ctx, mask)]
    held = [padded(ctx, q) for q in start]
    outs = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(8)]
    rec = ctx.subset_records().fill_bytes(0x7F)

    def call():
        ctx.subset_refine_masked(frames[0], frames[1], w, h, held[0], held[1], held[2:], nw, nh, r, s, R, frames[2], 57, out_u=outs[0],
                                 out_v=outs[1], out_gradients=outs[2:6], out_score=outs[6], out_state=outs[7], record=rec)

    def snapshot():
        ctx.synchronize()
        return [q.download().view(U32)[:nh, :nw].copy() for q in outs] + [rec.download(16, 1).tobytes()]

    call()
    direct = snapshot()
    want = subset_refine_masked_reference(f0, f1, start[0], start[1], start[2:], mask, 57, r, s, R)
    same_bytes((direct[:8], direct[8]), want, "direct call")
    assert masked_count(want) == 55
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    try:
        call()
    finally:
        graph = vp()
        assert lib.flow2d_capture_end(ctx.handle, ctypes.byref(graph)) == 0
    try:
        for fill in (0x7F, 0x11):
            for q in outs + [rec]:
                q.fill_bytes(fill)
            assert lib.flow2d_graph_launch(ctx.handle, graph) == 0
            for a, b in zip(snapshot(), direct):
                assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
            assert (outs[0].download().view(U32)[nh:] == U32(fill * 0x01010101)).all()
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)
    release(ctx, frames + held + outs + [rec])


# ---- refusals on a real context -----------------------------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing(flow2d, ctx):
    w, h, r, s, R = 96, 80, 7, 8, 7
    lib = flow2d.hip_lib()
    f0, f1, mask, _, _ = wide()
    start = second_step()
    nh, nw = start[0].shape
    p0, p1, pm = ctx.plane(w, h, f0), ctx.plane(w, h, f1), ctx.plane(w, h, mask)
    pin = [ctx.plane(nw, nh, q) for q in start]
    outs = [ctx.plane(nw, nh).fill_bytes(0x7F) for _ in range(8)]
    rec = ctx.subset_records().fill_bytes(0x7F)
    ins = ("u0", "v0", "ux0", "uy0", "vx0", "vy0")
    names = ("u", "v", "ux", "uy", "vx", "vy", "score", "state")
    base = dict(record=rec.ptr, mask=pm.ptr, min_pixels=57, **{n: q.ptr for n, q in zip(ins, pin)}, **{n: q.ptr for n, q in zip(names, outs)})

    def call(**kw):
        a = dict(base, **kw)
        return lib.flow2d_subset_refine_masked_2d(ctx.handle, p0.ptr, p1.ptr, w, h, p0.pitch, *[a[n] for n in ins], nw, nh, pin[0].pitch, r, s, R,
                                                  20, 1e-3, 4.0, 0.5, a["mask"], a["min_pixels"], *[a[n] for n in names], a["record"])

    inside_mask = pm.ptr + 16 * pm.pitch  # 16 rows into the mask: 16-byte aligned, and the node planes' rows still end inside it
    bad = [dict(min_pixels=5), dict(min_pixels=226), dict(min_pixels=0), dict(mask=pm.ptr + 4), dict(record=pm.ptr), dict(record=inside_mask),
           dict(mask=outs[0].ptr), dict(mask=p0.ptr, u=p0.ptr), dict(ux0=None), dict(u=pin[0].ptr), dict(v=outs[0].ptr), dict(ux=None)]
    if pm.pitch == pin[0].pitch:
        bad += [dict(u=inside_mask), dict(state=pm.ptr), dict(vy=inside_mask)]
    for kw in bad:
        assert call(**kw) == 1, kw
    ctx.synchronize()
    for q in outs:
        assert (q.download().view(U32) == POISON).all()
    assert set(rec.download(16, 1).tobytes()) == {0x7F}
    assert np.array_equal(pm.download(w, h).view(U32), bits(mask))
    assert call() == 0  # ... and the same planes are accepted
    ctx.synchronize()
    want = subset_refine_masked_reference(f0, f1, start[0], start[1], start[2:], mask, 57, r, s, R)
    same_bytes(([q.download(nw, nh).view(U32) for q in outs], rec.download(16, 1).tobytes()), want, "accepted")
