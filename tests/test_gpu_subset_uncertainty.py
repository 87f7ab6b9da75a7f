"""flow2d_subset_uncertainty_2d on the device against its numpy restatement (tests/test_subset_uncertainty_cpu.py) in the device's
summation order ("butterfly"): every output plane and the record byte for byte; each case prints how many words differ before it
asserts.  The layers above the entry are in tests/test_gpu_subset_uncertainty_host.py.
96 x 80 frames with the grid (7, s 8), 99 nodes, for R = 1, 2, 7; a 40 x 36 frame with the grid (3, s 4) for the radii either side
of every change of the waves per workgroup (four up to R = 12, three at 13, two from 14) and R = 15, where most nodes are outside.
The input field is the restated refinement of the stretched specimen, masked or plain, with one node each forced to NaN, to the
state -3 and to a huge u.  Masks: none and all zero (the same bytes), the specimen's, a seeded random one with 30 % excluded and
NaN and Inf entries, Nv at 8 and at 9, everything excluded.  Every plane lies in a container larger than its data, the mask's
padding NaN."""
import ctypes

import numpy as np
import pytest

from test_correlate_cpu import F32, U32, bits, grid, scenes_module
from test_gpu_batch_kernels import Tall, pitch_of, stride_of
from test_gpu_multipass import POISON, padded, release
from test_subset_masked_cpu import default_min_pixels, random_mask, specimen_case, subset_refine_masked_reference, usable_counts
from test_subset_spline_cpu import bspline_prefilter_reference
from test_subset_uncertainty_cpu import EVALUATED, MASKED, OUTSIDE, PLANES, SKIPPED, THIN, UNCERTAINTY_DTYPE, subset_uncertainty_reference, thin_mask

pytestmark = pytest.mark.gpu

ALL = (True,) * 8


# ---- the call ---------------------------------------------------------------------------------------------------------------------------
def run_uncertainty(ctx, f0, f1, nodes, state, mask, min_pixels, r, s, R, min_state=1, interpolation=0, present=ALL, record=True):
    """(the eight planes' bits -- None where absent --, record bytes) of one flow2d_subset_uncertainty_2d call into poisoned
    outputs, which must stay poisoned beyond the grid; f1 is frame 1 or, with interpolation = 1, its coefficients."""
    h, w = f0.shape
    nh, nw = state.shape
    frames = [padded(ctx, f0), padded(ctx, f1)] + ([padded(ctx, mask)] if mask is not None else [])
    held = [padded(ctx, q) for q in list(nodes) + [state]]
    outs = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(8)]
    rec = ctx.uncertainty_records().fill_bytes(0x7F)
    ctx.subset_uncertainty(frames[0], frames[1], w, h, held[:6], held[6], nw, nh, r, s, R, min_state, interpolation,
                           frames[2] if mask is not None else None, min_pixels, [q if there else None for q, there in zip(outs, present)],
                           rec if record else None)
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
    """The device's planes (bits) and record against the restatement `want`, byte for byte."""
    planes, raw = got
    differ = {name: int((g != bits(w_plane)).sum()) for g, w_plane, name in zip(planes, want.planes(), PLANES) if g is not None}
    print("%s: words that differ %s; record %s" % (what, differ, np.frombuffer(raw, UNCERTAINTY_DTYPE).tolist() if raw else None))
    if raw is not None:
        assert raw == want.record.tobytes(), "%s: record %s, want %s" % (what, np.frombuffer(raw, UNCERTAINTY_DTYPE), want.record)
    assert not any(differ.values()), "%s: %s" % (what, differ)


def check(ctx, f0, f1, nodes, state, mask, min_pixels, r, s, R, what, min_state=1, interpolation=0, **kw):
    want = subset_uncertainty_reference(f0, f1, nodes, state, r, s, R, min_state, mask, min_pixels, interpolation)
    same_bytes(run_uncertainty(ctx, f0, f1, nodes, state, mask, min_pixels, r, s, R, min_state, interpolation, **kw), want, what)
    return want


def count(want, name):
    return int(want.record[name][0])


# ---- inputs, made once ------------------------------------------------------------------------------------------------------------------
_cases = {}


def wide(masked):
    """96 x 80, grid (7, s 8): the stretched specimen, frame 1's coefficients, its mask, and the restated refinement at R = 7 (under
    the mask, or plain) with node (3, 3) forced to NaN, node (4, 4) to the state -3, node (5, 5) to a huge u, node (2, 6) to the
    state 0 and nodes (2, 7), (2, 8) to the states 65 and 66."""
    if ("wide", masked) not in _cases:
        scene, mask, u0, v0 = specimen_case("stretch")
        got = subset_refine_masked_reference(scene.frame_0, scene.frame_1, u0, v0, None, mask if masked else None, 57, 7, 8, 7, max_shift=2.0)
        nodes, state = [q.copy() for q in (got.u, got.v, got.ux, got.uy, got.vx, got.vy)], got.state.copy()
        nodes[4][3, 3], state[4, 4], nodes[0][5, 5] = np.nan, -3, 1e30
        state[2, 6], state[2, 7], state[2, 8] = 0, 65, 66
        if "coeff" not in _cases:
            _cases["coeff"] = bspline_prefilter_reference(scene.frame_1)
        _cases["wide", masked] = (scene.frame_0, scene.frame_1, _cases["coeff"], mask, nodes, state)
    return _cases["wide", masked]


def small():
    """40 x 36, grid (3, s 4), 9 x 8 nodes: the specimen at that size, its mask, frame 1's coefficients, and as the field the
    truth rounded to whole pixels with gradients of a hundredth, every state 1."""
    if "small" not in _cases:
        scene, mask = scenes_module().make_speckle_specimen("stretch", 40, 36, seed=0)
        nw, nh = grid(40, 36, 3, 4)
        cy, cx = 3 + np.arange(nh) * 4, 3 + np.arange(nw) * 4
        rng = np.random.default_rng(3)
        nodes = [np.rint(scene.gt_u[np.ix_(cy, cx)]).astype(F32), np.rint(scene.gt_v[np.ix_(cy, cx)]).astype(F32)]
        nodes += [rng.uniform(-0.01, 0.01, (nh, nw)).astype(F32) for _ in range(4)]
        _cases["small"] = (scene.frame_0, scene.frame_1, bspline_prefilter_reference(scene.frame_1), mask, nodes, np.ones((nh, nw), F32))
    return _cases["small"]


# ---- the fields at 96 x 80 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 7])
def test_the_specimens_fields(flow2d, ctx, R):
    """The plain field without a mask and the masked field under the specimen's mask, both samplers, both min_state."""
    for masked in (False, True):
        f0, f1, coeff, mask, nodes, state = wide(masked)
        for interpolation in (0, 1):
            for min_state in ((1, 0) if interpolation == 0 else (1,)):
                want = check(ctx, f0, coeff if interpolation else f1, nodes, state, mask if masked else None, default_min_pixels(R), 7, 8, R,
                             "specimen, R = %d, mask %s, interpolation %d, min_state %d" % (R, masked, interpolation, min_state), min_state,
                             interpolation)
                assert count(want, "evaluated") >= 10 and count(want, "skipped") >= 1
                # (nodes (4, 4) and (5, 5) lie in the specimen's hole: masked comes before skipped and outside)
                assert want.fate[3, 3] == SKIPPED and want.fate[4, 4] == (MASKED if masked else SKIPPED)
                assert want.fate[5, 5] == (MASKED if masked else OUTSIDE)
                if R == 7:
                    assert want.fate[2, 7] == want.fate[2, 8] == EVALUATED and want.fate[2, 6] == (SKIPPED if min_state else EVALUATED)
                if masked:
                    assert count(want, "masked") >= 40


def test_an_all_zero_mask_gives_the_bytes_of_no_mask(flow2d, ctx):
    f0, f1, coeff, _, nodes, state = wide(False)
    for interpolation, second in ((0, f1), (1, coeff)):
        none = run_uncertainty(ctx, f0, second, nodes, state, None, -3, 7, 8, 7, interpolation=interpolation)  # (min_pixels is not looked at)
        zero = run_uncertainty(ctx, f0, second, nodes, state, np.zeros(f0.shape, F32), 225, 7, 8, 7, interpolation=interpolation)
        for name, a, b in zip(PLANES, none[0], zero[0]):
            assert np.array_equal(a, b), name
        assert none[1] == zero[1]
        same_bytes(zero, subset_uncertainty_reference(f0, second, nodes, state, 7, 8, 7, interpolation=interpolation), "all-zero mask")


@pytest.mark.parametrize("R", [2, 7])
def test_a_random_mask_with_nan_and_inf_entries(flow2d, ctx, R):
    """30 % excluded at random (about a sixth of the pixels stays usable), some of them by NaN and +Inf."""
    f0, f1, coeff, _, nodes, state = wide(False)
    mask = random_mask(f0.shape, 0.3, seed=5)
    ones = np.argwhere(mask == 1)
    for k, (y, x) in enumerate(ones[::7]):
        mask[y, x] = (np.nan, np.inf, 0.5, 7.0)[k % 4]
    mask[mask == 0] = np.resize(np.array([0.0, -0.0, 0.49999997, -np.inf, 0.25], F32), int((mask == 0).sum()))
    for interpolation, second in ((0, f1), (1, coeff)):
        want = check(ctx, f0, second, nodes, state, mask, 6, 7, 8, R, "random mask, R = %d, interpolation %d" % (R, interpolation),
                     interpolation=interpolation)
        assert count(want, "masked") >= 20 and count(want, "evaluated") + count(want, "thin") >= 5


def test_eight_usable_pixels_are_thin_and_nine_are_evaluated(flow2d, ctx):
    f0, f1, _, _, nodes, state = wide(False)
    cx, cy = 7 + 5 * 8, 7 + 2 * 8  # node (2, 5)
    for usable, fate in ((8, THIN), (9, EVALUATED)):
        mask = thin_mask(f0.shape, cx, cy, usable)
        assert usable_counts(mask, 11, 9, 7, 8, 7)[2, 5] == usable
        want = check(ctx, f0, f1, nodes, state, mask, 6, 7, 8, 7, "Nv = %d" % usable)
        assert want.fate[2, 5] == fate and count(want, "masked") == 98 and count(want, "thin") == (usable == 8)


def test_everything_excluded(flow2d, ctx):
    f0, f1, _, _, nodes, state = wide(False)
    want = check(ctx, f0, f1, nodes, state, np.ones(f0.shape, F32), 6, 7, 8, 7, "everything excluded")
    assert want.record.tolist() == [(99, 0, 0, 99, 0, 0, 0, 0)]  # (masked comes before skipped)


def test_each_optional_plane_absent_in_turn(flow2d, ctx):
    f0, f1, _, mask, nodes, state = wide(True)
    full = check(ctx, f0, f1, nodes, state, mask, 57, 7, 8, 7, "all planes")
    no_rho, no_gradients, no_noise = (1, 1, 0, 1, 1, 1, 1, 1), (1, 1, 1, 0, 0, 0, 0, 1), (1, 1, 1, 1, 1, 1, 1, 0)
    for present, record in ((no_rho, True), (no_gradients, True), (no_noise, True), (ALL, False), ((1, 1, 0, 0, 0, 0, 0, 0), False)):
        got = run_uncertainty(ctx, f0, f1, nodes, state, mask, 57, 7, 8, 7, present=[bool(q) for q in present], record=record)
        same_bytes(got, full, "present %s, record %s" % (present, record))


# ---- the radii around every change of the waves per workgroup -----------------------------------------------------------------------
@pytest.mark.parametrize("R", [12, 13, 14, 15])
def test_the_large_radii(flow2d, ctx, R):
    """40 x 36: only the inner nodes' subsets lie inside frame 0, the others are outside; without a mask, under the specimen's
    and under a random one with 10 % excluded, so that a subset keeps a few hundred pixels."""
    f0, f1, coeff, mask, nodes, state = small()
    want = check(ctx, f0, f1, nodes, state, None, 0, 3, 4, R, "40x36, R = %d" % R)
    assert count(want, "evaluated") >= 1 and count(want, "outside") >= 60
    want = check(ctx, f0, coeff, nodes, state, mask, default_min_pixels(R), 3, 4, R, "40x36 specimen, B-spline, R = %d" % R, interpolation=1)
    assert count(want, "masked") >= 6 and count(want, "outside") >= 10
    want = check(ctx, f0, f1, nodes, state, random_mask(f0.shape, 0.1, seed=R), 6, 3, 4, R, "40x36 random, R = %d" % R)
    assert count(want, "evaluated") >= 1


# ---- the exact properties on the device -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [2, 11])
def test_both_frames_times_two_scales_nothing_but_the_noise(flow2d, ctx, R):
    f0, f1, _, _, nodes, state = wide(False)
    one = run_uncertainty(ctx, f0, f1, nodes, state, None, 0, 7, 8, R)
    two = run_uncertainty(ctx, f0 * F32(2), f1 * F32(2), nodes, state, None, 0, 7, 8, R)
    assert one[1] == two[1] and np.frombuffer(one[1], UNCERTAINTY_DTYPE)["evaluated"][0] >= 50
    for name, a, b in zip(PLANES[:7], one[0], two[0]):
        assert np.array_equal(a, b), name
    live = np.isfinite(one[0][7].view(F32))
    assert np.array_equal(two[0][7].view(F32)[live], one[0][7].view(F32)[live] * F32(2)) and (one[0][7].view(F32)[live] > 0).sum() >= 50


def test_a_pair_that_matches_exactly_has_sigma_zero(flow2d, ctx):
    f0 = wide(False)[0]
    f1 = np.roll(f0, (2, -3), axis=(0, 1))
    nw, nh = grid(96, 80, 7, 8)
    zero = np.zeros((nh, nw), F32)
    nodes = [np.full((nh, nw), -3, F32), np.full((nh, nw), 2, F32), zero, zero, zero, zero]
    state = np.ones((nh, nw), F32)
    got = run_uncertainty(ctx, f0, f1, nodes, state, None, 0, 7, 8, 3)
    same_bytes(got, subset_uncertainty_reference(f0, f1, nodes, state, 7, 8, 3), "an exact match")
    live = np.isfinite(got[0][2].view(F32))
    assert live.sum() >= 63
    for k in (0, 1, 3, 4, 5, 6, 7):
        assert (got[0][k][live] == 0).all(), PLANES[k]  # +0.0


# ---- the same bytes: a lock-step batch, a replayed graph ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["contiguous", "rows"])
def test_lock_step_batch_of_three(flow2d, ctx, kind):
    """Three instances `stride` apart with the same frames and three different masks and fields: planes and records of instance b
    are the bytes of that instance alone, and every other word of the allocations is what it was."""
    w, h, cw, ch, instances, r, s, R = 96, 80, 104, 84, 3, 7, 8, 7
    stride = stride_of(kind, pitch_of(cw), ch)
    f0, f1, _, mask, plain_nodes, plain_state = wide(False)
    _, _, _, _, masked_nodes, masked_state = wide(True)
    masks = [mask, random_mask(f0.shape, 0.3, seed=9), np.zeros(f0.shape, F32)]
    fields = [masked_nodes + [masked_state], plain_nodes + [plain_state], [q.copy() for q in plain_nodes] + [plain_state]]
    fields[2][1][1, 2] = np.nan  # a skipped node in one instance only
    nh, nw = plain_state.shape
    new = lambda: Tall(ctx, cw, ch, instances, stride)  # noqa: E731
    t0, t1, tm = new().fill([f0]), new().fill([f1]), new().fill(masks)
    tin = [new().fill([field[k] for field in fields]) for k in range(7)]
    outs = [new() for _ in range(8)]
    rec = ctx.uncertainty_records(instances).fill_bytes(0x7F)
    with ctx.set_batch(instances, stride):
        ctx.subset_uncertainty(t0, t1, w, h, tin[:6], tin[6], nw, nh, r, s, R, 1, 0, tm, 20, outs, rec, instances)
    ctx.synchronize()
    alone = [run_uncertainty(ctx, f0, f1, fields[b][:6], fields[b][6], masks[b], 20, r, s, R) for b in range(instances)]
    for k, tall in enumerate(outs):
        tall.check([a[0][k].view(F32) for a in alone], "%s (%s)" % (PLANES[k], kind))
    for tall in [t0, t1, tm] + tin:
        tall.check(None, "inputs")
    raw = rec.download(16 * instances, 1).tobytes()
    for b in range(instances):
        assert raw[64 * b:64 * b + 64] == alone[b][1], "record of instance %d" % b
    records = np.frombuffer(raw, UNCERTAINTY_DTYPE)
    assert records["masked"][0] >= 40 and records["masked"][1] >= 20 and records["masked"][2] == 0
    assert records["skipped"][2] >= 1 and records["evaluated"][2] > records["evaluated"][1] >= 1
    # a written range must not meet a later instance of the mask
    lib = flow2d.hip_lib()
    with ctx.set_batch(instances, stride):
        assert lib.flow2d_subset_uncertainty_2d(ctx.handle, t0.ptr, t1.ptr, 0, w, h, t0.pitch, *[q.ptr for q in tin], nw, nh, tin[0].pitch, r, s, R,
                                                1, tm.ptr, 20, tm.ptr + 2 * stride, outs[1].ptr, None, None, None, None, None, None, None) == 1
    ctx.synchronize()
    for k, tall in enumerate(outs):
        tall.check([a[0][k].view(F32) for a in alone], "after the refusal")
    release(ctx, [rec])


def test_a_graph_replayed_twice_gives_the_direct_calls_bytes(flow2d, ctx):
    w, h, r, s, R = 96, 80, 7, 8, 7
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    f0, f1, _, mask, nodes, state = wide(True)
    nh, nw = state.shape
    frames = [padded(ctx, f0), padded(ctx, f1), padded(ctx, mask)]
    held = [padded(ctx, q) for q in nodes + [state]]
    outs = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(8)]
    rec = ctx.uncertainty_records().fill_bytes(0x7F)

    def call():
        ctx.subset_uncertainty(frames[0], frames[1], w, h, held[:6], held[6], nw, nh, r, s, R, 1, 0, frames[2], 57, outs, rec)

    def snapshot():
        ctx.synchronize()
        return [q.download().view(U32)[:nh, :nw].copy() for q in outs] + [rec.download(16, 1).tobytes()]

    call()
    direct = snapshot()
    same_bytes((direct[:8], direct[8]), subset_uncertainty_reference(f0, f1, nodes, state, r, s, R, 1, mask, 57), "direct call")
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


# ---- planes of 4 GiB and just under -----------------------------------------------------------------------------------------------------
def test_planes_that_span_4_gib_and_just_under(flow2d, ctx):
    """The masked kernel with 64-bit offsets (planes of 4 GiB) and with 32-bit offsets whose bit 31 is set (just under), R = 15, on
    the field tests/test_gpu_wide_planes.py::test_subset_refine_masked restates: the same bytes as on ordinary planes, and those of
    the restatement.  Three tall planes."""
    from test_gpu_wide_planes import (GRID_R, GRID_S, H, HIGH_LINE, LINE, W, below_the_line, node_bits, node_poison, on_both, record_bytes,
                                      speckle_case, wrapped_rows_differ)
    R = 15
    f0, f1, u0, v0 = speckle_case()
    nh, nw = u0.shape
    mask = random_mask(f0.shape, 0.1, seed=55)
    field = subset_refine_masked_reference(f0, f1, u0, v0, None, mask, default_min_pixels(R), GRID_R, GRID_S, R)
    nodes = [field.u, field.v, field.ux, field.uy, field.vx, field.vy]
    want = subset_uncertainty_reference(f0, f1, nodes, field.state, GRID_R, GRID_S, R, 1, mask, default_min_pixels(R))
    below = subset_uncertainty_reference(f0[:LINE], f1[:LINE], [below_the_line(q) for q in nodes], below_the_line(field.state), GRID_R, GRID_S,
                                         R, 1, mask[:LINE], default_min_pixels(R))
    for j in (130, 131, 132, 255, 256, 257, 258):  # the node rows on either side of both lines, and wholly beyond them
        assert (want.fate[j] == EVALUATED).any(), "no node of row %d was evaluated" % j
    assert not np.array_equal(want.sigma_u[256:259], want.sigma_u[0:3]) and not np.array_equal(want.sigma_u[131:133], want.sigma_u[0:2])
    assert below.record.tobytes() != want.record.tobytes()
    wrapped_rows_differ(f0, f1, mask)
    assert HIGH_LINE < LINE < H

    def run(rig):
        p0, p1, pm = rig.load(f0), rig.load(f1), rig.load(mask)
        held = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F).upload(a) for a in nodes + [field.state]]
        outs, rec = node_poison(ctx, nw, nh, 8), ctx.uncertainty_records().fill_bytes(0x7F)
        ctx.subset_uncertainty(p0, p1, W, H, held[:6], held[6], nw, nh, GRID_R, GRID_S, R, 1, 0, pm, default_min_pixels(R), outs, rec)
        ctx.synchronize()
        got = dict(zip(PLANES, node_bits(outs, nw, nh)), record=record_bytes(rec, 64))
        release(ctx, held + outs + [rec])
        return got

    got = on_both(ctx, 3, run)
    same_bytes(([got[n] for n in PLANES], got["record"]), want, "100x4200 masked, R = 15, 4 GiB planes")


# ---- refusals on a real context -----------------------------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing(flow2d, ctx):
    w, h, r, s, R = 96, 80, 7, 8, 7
    lib = flow2d.hip_lib()
    f0, f1, _, mask, nodes, state = wide(True)
    nh, nw = state.shape
    p0, p1, pm = ctx.plane(w, h, f0), ctx.plane(w, h, f1), ctx.plane(w, h, mask)
    ins = ("u", "v", "ux", "uy", "vx", "vy", "state")
    names = ("su", "sv", "rho", "sux", "suy", "svx", "svy", "noise")
    pin = [ctx.plane(nw, nh, q) for q in nodes + [state]]
    outs = [ctx.plane(nw, nh).fill_bytes(0x7F) for _ in range(8)]
    rec = ctx.uncertainty_records().fill_bytes(0x7F)
    base = dict(record=rec.ptr, mask=pm.ptr, min_pixels=57, interpolation=0, min_state=1, **{n: q.ptr for n, q in zip(ins, pin)},
                **{n: q.ptr for n, q in zip(names, outs)})

    def call(**kw):
        a = dict(base, **kw)
        return lib.flow2d_subset_uncertainty_2d(ctx.handle, p0.ptr, p1.ptr, a["interpolation"], w, h, p0.pitch, *[a[n] for n in ins], nw, nh,
                                                pin[0].pitch, r, s, R, a["min_state"], a["mask"], a["min_pixels"], *[a[n] for n in names],
                                                a["record"])

    bad = [dict(interpolation=2), dict(min_state=2), dict(min_state=-1), dict(min_pixels=5), dict(min_pixels=226), dict(mask=pm.ptr + 4),
           dict(record=pm.ptr), dict(mask=outs[0].ptr), dict(state=None), dict(ux=None), dict(su=None), dict(sux=None), dict(su=pin[0].ptr),
           dict(sv=outs[0].ptr), dict(noise=pin[6].ptr), dict(rho=outs[7].ptr), dict(record=rec.ptr + 4)]
    for kw in bad:
        assert call(**kw) == 1, kw
    ctx.synchronize()
    for q in outs:
        assert (q.download().view(U32) == POISON).all()
    assert set(rec.download(16, 1).tobytes()) == {0x7F}
    assert call() == 0  # ... and the same planes are accepted
    ctx.synchronize()
    want = subset_uncertainty_reference(f0, f1, nodes, state, r, s, R, 1, mask, 57)
    same_bytes(([q.download(nw, nh).view(U32) for q in outs], rec.download(16, 1).tobytes()), want, "accepted")
    release(ctx, [p0, p1, pm] + pin + outs + [rec])
