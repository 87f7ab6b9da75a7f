"""The strip solver and the streaming kernels under the launch plans of other CU counts, bit for bit against the oracle.

The bytes a launch writes do not depend on its plan; the plan depends on the CU count, and a device has one.  With
flow2d_context_set_planning_cus a test runs, on whatever device it finds, the plans of one compute unit, of a partitioned chip and of
a larger chip: strips of hundreds of rows (the ring-unrolled row loop over many turns), block columns of two strips that both touch a
border, border-aware plans whose side blocks are not dealt over the launch order's runs, lock-step groups launched instance by
instance, more blocks than the device's own plan has, and tall strips of the streaming medians and the Gaussian with a ragged last
strip.  Every case sets its count explicitly and asserts, through the context's own diagnostic, that the plan is the one it is named
for (the classes: tests/test_planning_cus_cpu.py) before it compares."""
import ctypes

import numpy as np
import pytest

from conftest import in_container, level_fields
from test_gpu_batch_kernels import Tall, check_level, fields, pitch_of, stride_of
from test_planning_cus_cpu import (CASES, CHUNKED, GROUPS, PACKED, STREAM_CUS, STREAM_SIGMAS, STREAM_SIZES, check_plan_class)

pytestmark = pytest.mark.gpu

U32 = np.uint32
POISON = U32(0x7F7F7F7F)
GREY, GRADIENT, UNTILED, LOG = 0, 1, 2, 3
FUSED = 2
OUTER = 2
ALPHA = 3.5
BY_NAME = {c.name: c for c in CASES}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(U32)


def plan_for(flow2d, ctx, case, instances=1, split=False):
    """Sets the case's count and asserts, on the context, that launches of the case's level take the plan the case is named for."""
    ctx.set_planning_cus(case.cus)
    assert ctx.planning_cus() == case.cus
    plan = check_plan_class(flow2d, case, instances, split)
    per_launch = 1 if split else instances
    order = ctx.fused_block_order(case.w, case.h, case.inner, per_launch)
    assert np.array_equal(order, flow2d.fused_block_order_for_cus(case.cus, case.w, case.h, case.inner, per_launch)), case.name
    other = flow2d.fused_block_order_for_cus(case.differs, case.w, case.h, case.inner, per_launch)
    assert order.shape != other.shape or not np.array_equal(order, other), case.name
    assert int((order[:, 0] >= 0).sum()) == plan.blocks
    return plan


_inputs, _wanted = {}, {}


def inputs(oracle, w, h, seed=31):
    if (w, h, seed) not in _inputs:
        _inputs[(w, h, seed)] = level_fields(oracle, w, h, seed)[:4]
    return _inputs[(w, h, seed)]


def wanted(ctx, oracle, case, inner, constancy, omega=0.0):
    """The oracle's level, computed once per (level, sweeps, data term) and shared by the tests that need it."""
    key = (case.w, case.h, case.cw, case.ch, inner, constancy, omega)
    if key not in _wanted:
        f0, f1, u, v = inputs(oracle, case.w, case.h)
        hx, hy = np.float32(case.cw / case.w), np.float32(case.ch / case.h)
        if omega:
            _wanted[key] = oracle.solve_level_sor(f0, f1, u, v, case.w, case.h, hx, hy, ALPHA, 0.001, 0.001, OUTER, inner, omega, constancy)[:2]
        elif constancy == LOG:  # the oracle is handed the device's logarithms (tests/test_gpu_log_derivatives.py)
            with oracle.device_logs(ctx):
                _wanted[key] = oracle.solve_level(f0, f1, u, v, case.w, case.h, hx, hy, ALPHA, 0.001, 0.001, OUTER, inner, constancy)[:2]
        else:
            _wanted[key] = oracle.solve_level(f0, f1, u, v, case.w, case.h, hx, hy, ALPHA, 0.001, 0.001, OUTER, inner, constancy)[:2]
    return _wanted[key]


def assert_level(plane, want, w, h, what):
    """The level rectangle is the oracle's, word for word; the rest of the container is the poison it was filled with (the rows
    below the level, over the level's width, may have been zeroed: include/flow2d_c_abi.h, flow2d_solve_level)."""
    got = bits(plane.download())
    bad = np.argwhere(got[:h, :w] != bits(want))
    assert not len(bad), "%s: %d words differ, the first at row %d, column %d" % (what, len(bad), bad[0][0], bad[0][1])
    assert (got[:, w:] == POISON).all(), what + ": written right of the level"
    below = got[h:, :w]
    assert (below == POISON).all() or not below.any(), what + ": written below the level"


def run_level(ctx, oracle, case, inner, constancy, omega=0.0):
    w, h, cw, ch = case.w, case.h, case.cw, case.ch
    d = [ctx.plane(cw, ch, in_container(a, cw, ch)) for a in inputs(oracle, w, h)]
    scratch = [ctx.plane(cw, ch).fill_bytes(0x7F) for _ in range(6)]
    hx, hy = np.float32(cw / w), np.float32(ch / h)
    rdu, rdv = ctx.solve_level(*d, *scratch, w, h, hx, hy, ALPHA, 0.001, 0.001, OUTER, inner, constancy, FUSED, sor_omega=omega)
    odu, odv = wanted(ctx, oracle, case, inner, constancy, omega)
    what = "%s, %d CUs, inner %d, data term %d, omega %g" % (case.name, case.cus, inner, constancy, omega)
    assert_level(rdu, odu, w, h, what + ": du")
    assert_level(rdv, odv, w, h, what + ": dv")
    for plane, a in zip(d, inputs(oracle, w, h)):
        assert np.array_equal(bits(plane.download()), bits(in_container(a, cw, ch))), what + ": an input was written"


# ---- the strip solver, one pair -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("constancy", [GREY, GRADIENT], ids=["grey", "gradient"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_single_pair(flow2d, ctx, oracle, case, constancy):
    plan_for(flow2d, ctx, case)
    run_level(ctx, oracle, case, case.inner, constancy)


@pytest.mark.parametrize("constancy", [GREY, GRADIENT], ids=["grey", "gradient"])
def test_chunked_sweeps_continue_under_long_strips(flow2d, ctx, oracle, constancy):
    """inner 8 is two launches of four sweeps per outer iteration; the second continues the first one's sweeps from its result
    (the kernels of continued sweeps), here down eight 113-row strips per block column."""
    plan_for(flow2d, ctx, CHUNKED)
    run_level(ctx, oracle, CHUNKED, 8, constancy)


@pytest.mark.parametrize("name,constancy", [("sides_not_dealt", UNTILED), ("dealt_sides_139_112", UNTILED),
                                            ("uniform_180_rows", LOG), ("dealt_sides_81_65", LOG)])
def test_other_data_terms(flow2d, ctx, oracle, name, constancy):
    case = BY_NAME[name]
    plan_for(flow2d, ctx, case)
    run_level(ctx, oracle, case, case.inner, constancy)


@pytest.mark.parametrize("case,iterations", [(BY_NAME["two_border_strips"], 1), (CHUNKED, 2)], ids=["2_stages", "4_stages"])
def test_red_black_sor(flow2d, ctx, oracle, case, iterations):
    """A launch of red-black SOR holds two half-sweep stages per iteration and is planned by its stages: the cases' inner counts."""
    assert case.inner == 2 * iterations
    plan_for(flow2d, ctx, case)
    run_level(ctx, oracle, case, iterations, GREY, omega=1.4)


# ---- lock-step groups -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("constancy", [GREY, GRADIENT], ids=["grey", "gradient"])
@pytest.mark.parametrize("case,count,split", GROUPS, ids=[g[0].name for g in GROUPS])
def test_groups(flow2d, ctx, oracle, case, count, split, constancy):
    """Instances `stride` bytes apart with padding rows between them (no multiple of the level): every instance is the oracle's level
    of its own inputs and what the instance gives alone, the inputs and every word outside the levels are what they were.  split:
    the instances are launched one by one, every plane pointer stepped by the stride."""
    w, h, cw, ch, inner = case.w, case.h, case.cw, case.ch, case.inner
    plan_for(flow2d, ctx, case, count, split)
    stride = stride_of("rows", pitch_of(cw), ch)
    assert stride > pitch_of(cw) * ch
    f0, f1, u, v, _, _ = fields(oracle, w, h, count, 29)
    d = [Tall(ctx, cw, ch, count, stride).fill(x) for x in (f0, f1, u, v)]
    written = [Tall(ctx, cw, ch, count, stride) for _ in range(6)]  # du, dv, phi, ksi, tdu, tdv: poison
    hx, hy = np.float32(cw / w), np.float32(ch / h)
    what = "%s x %d, data term %d" % (case.name, count, constancy)
    with ctx.set_batch(count, stride):
        pair = ctx.solve_level(*d, *written, w, h, hx, hy, ALPHA, 0.001, 0.001, OUTER, inner, constancy, FUSED, container_height=ch)
    ctx.synchronize()
    want = [oracle.solve_level(a, b, c, e, w, h, hx, hy, ALPHA, 0.001, 0.001, OUTER, inner, constancy)[:2] for a, b, c, e in zip(f0, f1, u, v)]
    du, dv, phi, ksi, tdu, tdv = written
    assert pair in ((du, dv), (tdu, tdv))
    other = (tdu, tdv) if pair[0] is du else (du, dv)
    check_level(pair, other, (phi, ksi), [[q[0] for q in want], [q[1] for q in want]], w, h, ch, what)
    for t in d:
        t.check(None, what + ": an input")
    group = [t.rects(t.download())[:, :h, :w].copy() for t in pair]
    for b in range(count):  # the instance alone, under the same planning count
        lone = [ctx.plane(cw, ch, in_container(x[b], cw, ch)) for x in (f0, f1, u, v)]
        scratch = [ctx.plane(cw, ch).fill_bytes(0x7F) for _ in range(6)]
        rdu, rdv = ctx.solve_level(*lone, *scratch, w, h, hx, hy, ALPHA, 0.001, 0.001, OUTER, inner, constancy, FUSED)
        assert np.array_equal(bits(rdu.download(w, h)), group[0][b]) and np.array_equal(bits(rdv.download(w, h)), group[1][b]), (what, b)


# ---- the packed build -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("constancy", [GREY, GRADIENT], ids=["grey", "gradient"])
def test_packed_build_serves_a_larger_plan(flow2d, ctx, oracle, constancy):
    """A lone context takes the packed build for launches of at most one workgroup per planning CU: with 512 of them that is
    2048 x 1536 at inner 5, more blocks than the packed build has run on any device (test_gpu_fused_packed.py leaves this level to
    the pipeline's build).  flow2d_fused_packed_launches rises by the outer iterations; the bits are the oracle's."""
    ctx.set_lone(True)
    plan = plan_for(flow2d, ctx, PACKED)
    assert 256 < plan.blocks <= 512
    before = flow2d.fused_packed_launches()
    run_level(ctx, oracle, PACKED, PACKED.inner, constancy)
    assert flow2d.fused_packed_launches() - before == OUTER
    ctx.set_planning_cus(256)  # the same level on the device's usual plan: 488 blocks, the pipeline's build
    before = flow2d.fused_packed_launches()
    run_level(ctx, oracle, PACKED, PACKED.inner, constancy)
    assert flow2d.fused_packed_launches() == before


# ---- the streaming kernels ---------------------------------------------------------------------------------------------------------
_stream = {}


def stream_reference(flow2d, oracle, w, h):
    """Inputs and the oracle's medians and blurs of a size, once for the four planning counts."""
    if (w, h) not in _stream:
        _, _, u, v, du, dv = level_fields(oracle, w, h, 3 + w)
        u[::3, ::5] = 0.0  # ties
        ref = {"in": (u, v, du, dv)}
        for window in (3, 5, 7):
            ref[window] = (oracle.median(u, w, h, window), oracle.median(v, w, h, window),
                           oracle.median(oracle.add(u, du, w, h), w, h, window), oracle.median(oracle.add(v, dv, w, h), w, h, window))
        for sigma in STREAM_SIGMAS:
            ref[sigma] = oracle.convolution(u, w, h, sigma)
        _stream[(w, h)] = ref
    return _stream[(w, h)]


def assert_plane(plane, want, w, h, what):
    got = bits(plane.download())
    bad = np.argwhere(got[:h, :w] != bits(want))
    assert not len(bad), "%s: %d words differ, the first at row %d, column %d" % (what, len(bad), bad[0][0], bad[0][1])
    outside = np.ones(got.shape, bool)
    outside[:h, :w] = False
    assert (got[outside] == POISON).all(), what + ": written outside the level"


@pytest.mark.parametrize("cus", STREAM_CUS)
@pytest.mark.parametrize("w,h,cw,ch", STREAM_SIZES)
def test_streaming_kernels(flow2d, ctx, oracle, w, h, cw, ch, cus):
    """Median 3 / 5 / 7 (one plane, the pair launch, the add-median form with two plane sets) and the Gaussian at three radii, in
    containers whose remainder is poison on the input side too: strips of every height the planners know, the last one ragged."""
    ref = stream_reference(flow2d, oracle, w, h)
    ctx.set_planning_cus(cus)
    assert ctx.planning_cus() == cus
    rows = flow2d.stream_rows_for_cus(cus, flow2d.STREAM_MEDIAN, w, h, 2)
    assert rows in (8, 16, 32, 64)  # (which sizes and counts give which: test_planning_cus_cpu.py::test_streaming_cases_reach_every_row_count)
    tu, tv, tdu, tdv = (ctx.plane(cw, ch).fill_bytes(0x7F).upload(a) for a in ref["in"])
    for window in (3, 5, 7):
        med_u, med_v, sum_u, sum_v = ref[window]
        what = "median %d, %d x %d, %d CUs (%d rows per strip)" % (window, w, h, cus, rows)
        ou, ov = (ctx.plane(cw, ch).fill_bytes(0x7F) for _ in range(2))
        ctx.median(tu, w, h, window, ou)
        assert_plane(ou, med_u, w, h, what)
        ou.fill_bytes(0x7F)
        ctx.median_pair(tu, tv, w, h, window, ou, ov)
        assert_plane(ou, med_u, w, h, what + ", pair")
        assert_plane(ov, med_v, w, h, what + ", pair, second plane")
        ou.fill_bytes(0x7F), ov.fill_bytes(0x7F)
        ctx.add_median(tu, tdu, w, h, window, ou, tv, tdv, ov)
        assert_plane(ou, sum_u, w, h, what + ", add")
        assert_plane(ov, sum_v, w, h, what + ", add, second plane")
    for sigma in STREAM_SIGMAS:
        taps, radius = flow2d.gaussian_kernel(sigma)
        rows = flow2d.stream_rows_for_cus(cus, flow2d.STREAM_GAUSSIAN, w, h, radius)
        assert rows in (16, 32, 64, 128)
        dst = ctx.plane(cw, ch).fill_bytes(0x7F)
        ctx.gaussian_blur(dst, tu, w, h, taps, radius)
        assert_plane(dst, ref[sigma], w, h, "gaussian radius %d, %d x %d, %d CUs (%d rows per strip)" % (radius, w, h, cus, rows))
    for plane, a in zip((tu, tv, tdu, tdv), ref["in"]):
        assert_plane(plane, a, w, h, "an input")


# ---- a recorded graph keeps its plan ------------------------------------------------------------------------------------------------
def test_captured_graph_keeps_the_plan_it_was_recorded_with(flow2d, ctx, oracle):
    """A plan is fixed when a launch is queued: a level recorded at 8 CUs (five 180-row strips per column) and replayed after the
    count went back to the device's gives the bytes of the eager run and of the oracle, twice."""
    case = BY_NAME["uniform_180_rows"]
    w, h, cw, ch = case.w, case.h, case.cw, case.ch
    lib, vp = flow2d.hip_lib(), ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    device_cus = ctx.planning_cus()
    plan_for(flow2d, ctx, case)
    d = [ctx.plane(cw, ch, in_container(a, cw, ch)) for a in inputs(oracle, w, h)]
    scratch = [ctx.plane(cw, ch).fill_bytes(0x7F) for _ in range(6)]
    hx, hy = np.float32(cw / w), np.float32(ch / h)
    odu, odv = wanted(ctx, oracle, case, case.inner, GREY)
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    try:
        rdu, rdv = ctx.solve_level(*d, *scratch, w, h, hx, hy, ALPHA, 0.001, 0.001, OUTER, case.inner, GREY, FUSED)
    finally:
        graph = vp()
        assert lib.flow2d_capture_end(ctx.handle, ctypes.byref(graph)) == 0
    try:
        ctx.synchronize()
        assert (bits(rdu.download()) == POISON).all()  # recorded, not run
        ctx.set_planning_cus(0)
        assert ctx.planning_cus() == device_cus
        for _ in range(2):
            for q in scratch:
                q.fill_bytes(0x7F)
            assert lib.flow2d_graph_launch(ctx.handle, graph) == 0
            ctx.synchronize()
            assert_level(rdu, odu, w, h, "replayed: du")
            assert_level(rdv, odv, w, h, "replayed: dv")
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)


# ---- the whole pipeline -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("constancy", [GREY, GRADIENT], ids=["grey", "gradient"])
def test_whole_pipeline_under_two_counts(flow2d, ctx, oracle, constancy):
    """700 x 650, three levels at scale 0.5, 2 x 5 sweeps, median 5, sigma 1.5: the finest level is the strips' (four 163-row strips per
    column at 8 CUs, 14 / 10 rows at 304), the blur and the medians stream under the same count; both runs are the oracle's flow."""
    w, h = 700, 650
    f0, f1 = oracle.synthetic_pair(w, h, 1.5, -0.75, seed=7, noise=True)
    ou, ov, _ = oracle.compute_flow(f0, f1, 3, 0.5, 2, 5, 35.0, 0.001, 0.001, 5, 1.5, constancy)
    flow = flow2d.OpticalFlow(w, h, constancy, ctx=ctx, lone=False)
    try:
        for cus, uniform in ((8, True), (304, False)):
            ctx.set_planning_cus(cus)
            order = ctx.fused_block_order(w, h, 5)
            assert np.array_equal(order, flow2d.fused_block_order_for_cus(cus, w, h, 5))
            assert flow2d.fused_plan_for_cus(cus, w, h, 5).uniform == uniform
            u, v, _ = flow.compute_flow(f0, f1, flow.params(3, 0.5, 2, 5, 35.0, 0.001, 0.001, 5, 1.5))
            assert np.array_equal(bits(u), bits(ou)) and np.array_equal(bits(v), bits(ov)), cus
    finally:
        flow.close()


# ---- the setter on a real context ----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_count_as_it_was(flow2d, ctx):
    device_cus = ctx.planning_cus()
    assert device_cus >= 1
    ctx.set_planning_cus(8)
    for bad in (-1, 4097, 1 << 30):
        with pytest.raises(flow2d.Flow2DError) as e:
            ctx.set_planning_cus(bad)
        assert e.value.status == 1 and ctx.planning_cus() == 8
    ctx.set_planning_cus(0)
    assert ctx.planning_cus() == device_cus
    assert np.array_equal(ctx.fused_block_order(640, 520, 5), flow2d.fused_block_order_for_cus(device_cus, 640, 520, 5))
