"""flow2d_compose_nodes_2d on the device against its numpy restatement (compose_reference of tests/test_subset_reference_cpu.py):
every byte of every plane, of the state, of the score and of the record.  Grids of 2 x 2 (every clamp active), 11 x 9 (the fields
of the rotation sequence: the base from step 3, the increment a real refinement), 70 x 5 (across the 64-lane row, the block not
full); containers larger than the data with poisoned outputs; synthetic fields with holes, outside nodes and a partly lost cell;
the score and the state absent; a lock-step batch of two; a replayed graph; the refusals, which write nothing."""
import ctypes

import numpy as np
import pytest

from test_correlate_cpu import F32, U32, bits
from test_gpu_batch_kernels import Tall, pitch_of, stride_of
from test_gpu_multipass import POISON, padded, release
from test_subset_reference_cpu import (COMPOSE_DTYPE, COMPOSED, ROTATION, affine_field, compose_reference, first5, holes_case, rotation_rows,
                                       rotation_scenes, seven)
from test_subset_sequence_cpu import PLANES, predict_passes

pytestmark = pytest.mark.gpu


def run_compose(ctx, base, increment, r, s, min_state=1, score=None, with_state=True, record=True):
    """([six planes' bits, the state's, the score's -- None where absent], record bytes or None) of one call into poisoned outputs in
    containers with a padded node pitch, which must stay poisoned beyond the grid; the inputs' padding is NaN."""
    nh, nw = base[6].shape
    held = [padded(ctx, q) for q in list(base) + list(increment)]
    sc = padded(ctx, score) if score is not None else None
    outs = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(8)]
    rec = ctx.compose_records().fill_bytes(0x7F)
    ctx.compose_nodes(held[:7], held[7:], nw, nh, r, s, min_state, sc, outs[:6], outs[6] if with_state else None,
                      outs[7] if score is not None else None, rec if record else None)
    ctx.synchronize()
    got = [q.download().view(U32) for q in outs]
    present = [True] * 6 + [with_state, score is not None]
    for g, there in zip(got, present):
        if there:
            assert (g[nh:] == POISON).all() and (g[:, nw:] == POISON).all(), "written beyond the grid"
        else:
            assert (g == POISON).all(), "an absent plane was written"
    raw = rec.download(16, 1).tobytes()
    assert record or set(raw) == {0x7F}
    result = [g[:nh, :nw] if there else None for g, there in zip(got, present)], (raw if record else None)
    release(ctx, held + ([sc] if sc is not None else []) + outs + [rec])
    return result


def check_compose(ctx, base, increment, r, s, what, min_state=1, score=None, **kw):
    planes, state, out_score, record = compose_reference(base, increment, r, s, min_state, score)
    got, raw = run_compose(ctx, base, increment, r, s, min_state, score, **kw)
    for name, g, want in zip(PLANES, got, planes):
        assert np.array_equal(g, bits(want)), "%s: %s" % (what, name)
    if got[6] is not None:
        assert np.array_equal(got[6], bits(state)), "%s: state %s, want %s" % (what, got[6].view(F32), state)
    if score is not None:
        assert np.array_equal(got[7], bits(out_score)), "%s: score" % what
    if raw is not None:
        assert raw == record.tobytes(), "%s: record %s, want %s" % (what, np.frombuffer(raw, COMPOSE_DTYPE), record)
    return planes, state, out_score, record


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def rotation_fields():
    """The 11 x 9 fields of the rotation sequence with a new reference every 3 steps, restated once (lru-cached there): the base
    of reference 3 -- two prediction passes over step 3's field -- and the increment of step 5, a refinement from step 4's."""
    c = ROTATION
    from test_subset_reference_cpu import chained_with_reference
    if "fields" not in _cache:
        scenes = rotation_scenes()[:5]
        delivered, records, increments = chained_with_reference(scenes, c["r"], c["s"], c["R"], 3, c["d"])
        nodes, state, _ = predict_passes(seven(delivered[2])[:6], delivered[2].state, c["s"], 2)
        _cache["fields"] = (list(nodes) + [state], increments[4], delivered[4], records[4])
    return _cache["fields"]


_cache = {}


def wide_case(nh=5, nw=70, r=3, s=4, seed=5):
    """70 x 5 nodes: a smooth made-up base that carries the nodes up to a cell and a half, an increment with holes."""
    rng = np.random.default_rng(seed)
    A = [(rng.standard_normal((nh, nw)) * a).astype(F32) for a in (3.0, 3.0, 0.05, 0.05, 0.05, 0.05)]
    A.append(np.where(rng.random((nh, nw)) < 0.1, -3, 5).astype(F32))
    B = [(rng.standard_normal((nh, nw)) * a).astype(F32) for a in (1.0, 1.0, 0.05, 0.05, 0.05, 0.05)]
    B.append(np.where(rng.random((nh, nw)) < 0.3, -3, 2).astype(F32))
    B[6][1:4, 10:14] = -2           # a hole wider than a cell: nodes with no increment
    B[0][2, 30], B[3][3, 40] = np.nan, np.inf
    B[6][2, 50], A[6][2, 51] = 0, 0
    A[6][4, 69] = np.nan
    return A, B, rng.random((nh, nw)).astype(F32), r, s


# ---- the bytes ------------------------------------------------------------------------------------------------------------------------
def test_the_minimum_grid(flow2d, ctx):
    """2 x 2: one cell, every node's cell clamped; a node carried exactly half a cell out (inside) and one a little further."""
    r, s = 2, 3
    A = [np.array(q, F32) for q in ([[-1.5, 1.4], [0.5, -0.5]], [[-1.5, -1.4], [1.4, 0.25]], [[0.01, 0], [0, 0]], [[0, 0.02], [0, 0]],
                                    [[0, 0], [0.03, 0]], [[0, 0], [0, -0.01]], [[1, 1], [1, 1]])]
    B = affine_field(2, 2, r, s, np.array([[1.02, 0.01], [0.0, 0.99]]), np.array([0.3, -0.2]))
    sc = np.array([[0.9, 0.8], [0.7, 0.6]], F32)
    _, state, _, record = check_compose(ctx, A, B, r, s, "2x2", score=sc)
    assert first5(record) == [4, 4, 0, 0, 0]
    A[0][0, 0] = np.nextafter(F32(-1.5), F32(-2))
    A[1][1, 0] = 1.6
    B[6][1, 1] = -3
    _, state, _, record = check_compose(ctx, A, B, r, s, "2x2, two outside, a lost corner", score=sc)
    assert first5(record) == [4, 2, 0, 2, 0] and state[0, 0] == -1 and state[1, 0] == -1


@pytest.mark.parametrize("min_state", [0, 1])
def test_the_rotation_sequences_fields(flow2d, ctx, min_state):
    base, inc, delivered, record = rotation_fields()
    planes, state, score, got = check_compose(ctx, base, seven(inc), ROTATION["r"], ROTATION["s"], "11x9 rotation", min_state, inc.score)
    assert state.shape == (9, 11) and first5(got)[1] >= 60 and first5(got)[3] >= 5
    if min_state == 1:  # ... which is the sequence's delivered step 5
        assert got.tobytes() == record.tobytes() and np.array_equal(bits(planes[0]), bits(delivered.u))


@pytest.mark.parametrize("min_state", [0, 1])
def test_holes_outside_nodes_and_a_partly_lost_cell(flow2d, ctx, min_state):
    A, B, sc, kind, r, s = holes_case()
    _, state, _, record = check_compose(ctx, A, B, r, s, "holes, min_state %d" % min_state, min_state, sc)
    assert min(first5(record)[1:]) >= 2 and state[3, 4] == COMPOSED and (state[1, 3] == COMPOSED) == (min_state == 0)


def test_across_the_wave_row(flow2d, ctx):
    A, B, sc, r, s = wide_case()
    _, state, _, record = check_compose(ctx, A, B, r, s, "70x5", 1, sc)
    print(first5(record))
    assert min(first5(record)[1:]) >= 3 and (state[:, 64:] == COMPOSED).any() and (state[4] == COMPOSED).any()
    check_compose(ctx, A, B, r, s, "70x5, min_state 0", 0, sc)


def test_the_optional_planes(flow2d, ctx):
    A, B, sc, r, s = wide_case(seed=6)
    check_compose(ctx, A, B, r, s, "no score")
    check_compose(ctx, A, B, r, s, "no state", with_state=False)
    check_compose(ctx, A, B, r, s, "no state, no record, a score", score=sc, with_state=False, record=False)


# ---- the same bytes: a lock-step batch, a replayed graph ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["contiguous", "rows"])
def test_lock_step_batch_of_two(flow2d, ctx, kind):
    count, cw, ch = 2, 76, 7
    cases = [wide_case(seed=7), wide_case(seed=8)]
    r, s = cases[0][3], cases[0][4]
    nh, nw = cases[0][0][6].shape
    stride = stride_of(kind, pitch_of(cw), ch)
    new = lambda: Tall(ctx, cw, ch, count, stride)  # noqa: E731
    tin = [new().fill([c[0][k] for c in cases]) for k in range(7)] + [new().fill([c[1][k] for c in cases]) for k in range(7)]
    tsc = new().fill([c[2] for c in cases])
    outs = [new() for _ in range(8)]
    rec = ctx.compose_records(count).fill_bytes(0x7F)
    with ctx.set_batch(count, stride):
        ctx.compose_nodes(tin[:7], tin[7:], nw, nh, r, s, 1, tsc, outs[:6], outs[6], outs[7], rec, instances=count)
    ctx.synchronize()
    alone = [run_compose(ctx, c[0], c[1], r, s, 1, c[2]) for c in cases]
    for k, tall in enumerate(outs):
        tall.check([a[0][k].view(F32) for a in alone], "plane %d (%s)" % (k, kind))
    for tall in tin + [tsc]:
        tall.check(None, "inputs")
    raw = rec.download(16 * count, 1).tobytes()
    for b in range(count):
        assert raw[64 * b:64 * b + 64] == alone[b][1], "record of instance %d" % b
    assert alone[0][1] != alone[1][1]
    # a written range must not meet the second instance of an input
    lib = flow2d.hip_lib()
    arr = lambda planes: (ctypes.c_void_p * len(planes))(*planes)  # noqa: E731
    with ctx.set_batch(count, stride):
        assert lib.flow2d_compose_nodes_2d(ctx.handle, arr([q.ptr for q in tin[:7]]), arr([q.ptr for q in tin[7:]]), None, nw, nh, tin[0].pitch, r, s,
                                           1, arr([q.ptr for q in outs[:5]] + [tin[9].ptr + stride]), None, None, None) == 1
    ctx.synchronize()


def test_a_replayed_graph_gives_the_direct_calls_bytes(flow2d, ctx):
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    A, B, sc, r, s = wide_case(seed=9)
    nh, nw = A[6].shape
    held = [padded(ctx, q) for q in A + B + [sc]]
    outs = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(8)]
    rec = ctx.compose_records().fill_bytes(0x7F)

    def call():
        ctx.compose_nodes(held[:7], held[7:14], nw, nh, r, s, 1, held[14], outs[:6], outs[6], outs[7], rec)

    def snapshot():
        ctx.synchronize()
        return [q.download().view(U32)[:nh, :nw].copy() for q in outs] + [rec.download(16, 1).tobytes()]

    call()
    direct = snapshot()
    planes, state, score, record = compose_reference(A, B, r, s, 1, sc)
    assert direct[-1] == record.tobytes() and np.array_equal(direct[0], bits(planes[0]))
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
    release(ctx, held + outs + [rec])


# ---- refusals on a real context -----------------------------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing(flow2d, ctx):
    lib = flow2d.hip_lib()
    A, B, sc, r, s = wide_case(seed=10)
    nh, nw = A[6].shape
    pa, pb, psc = [ctx.plane(nw, nh, q) for q in A], [ctx.plane(nw, nh, q) for q in B], ctx.plane(nw, nh, sc)
    outs = [ctx.plane(nw, nh).fill_bytes(0x7F) for _ in range(8)]
    rec = ctx.compose_records().fill_bytes(0x7F)
    arr = lambda planes: (ctypes.c_void_p * len(planes))(*planes)  # noqa: E731

    def call(a=None, b=None, o=None, score=psc.ptr, out_state=outs[6].ptr, out_score=outs[7].ptr, record=rec.ptr, nw_=nw, nh_=nh, r_=r, s_=s,
             low=1):
        a, b, o = a or [q.ptr for q in pa], b or [q.ptr for q in pb], o or [q.ptr for q in outs[:6]]
        return lib.flow2d_compose_nodes_2d(ctx.handle, arr(a), arr(b), score, nw_, nh_, pa[0].pitch, r_, s_, low, arr(o), out_state, out_score,
                                           record)

    def swapped(planes, k, value):
        ptrs = [q.ptr for q in planes]
        ptrs[k] = value
        return ptrs

    bad = [dict(a=swapped(pa, 6, None)), dict(b=swapped(pb, 0, None)), dict(o=swapped(outs[:6], 3, None)),
           dict(o=[q.ptr for q in pa[:6]]), dict(o=swapped(outs[:6], 2, pb[4].ptr)), dict(o=swapped(outs[:6], 3, outs[2].ptr)),
           dict(out_state=pb[6].ptr), dict(out_state=outs[0].ptr), dict(out_score=psc.ptr), dict(out_score=outs[6].ptr),
           dict(score=None), dict(out_score=None), dict(record=rec.ptr + 4), dict(record=pa[0].ptr), dict(nw_=1), dict(nh_=1), dict(nw_=0),
           dict(r_=0), dict(r_=16), dict(s_=0), dict(s_=65), dict(low=2), dict(low=-1), dict(a=swapped(pa, 1, pa[1].ptr + 4))]
    for kw in bad:
        assert call(**kw) == 1, kw
    ctx.synchronize()
    for q in outs:
        assert (q.download().view(U32) == POISON).all()
    assert set(rec.download(16, 1).tobytes()) == {0x7F}
    assert call() == 0  # ... and the same planes are accepted
    ctx.synchronize()
    planes, state, score, record = compose_reference(A, B, r, s, 1, sc)
    for q, want in zip(outs, planes + [state, score]):
        assert np.array_equal(q.download(nw, nh).view(U32), bits(want))
    assert rec.download(16, 1).tobytes() == record.tobytes()
    # the wrapper's own checks and its allocating form
    with pytest.raises(ValueError):
        ctx.compose_nodes(pa[:6], pb, nw, nh, r, s)
    with pytest.raises(ValueError):
        ctx.compose_nodes(pa, pb, nw, nh, r, s, out=outs[:5])
    got, got_state, got_score, got_record = ctx.compose_nodes(pa, pb, nw, nh, r, s, score=psc)
    assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, planes)) and np.array_equal(bits(got_state), bits(state))
    assert np.array_equal(bits(got_score), bits(score)) and bytes(got_record) == record.tobytes()
    assert ctx.compose_nodes(pa, pb, nw, nh, r, s, record=False)[2:] == (None, None)
