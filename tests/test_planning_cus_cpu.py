"""The launch planners under other CU counts than the one the suite's device has, on the host alone (no device).

Three planners read the context's CU count: the strip plan of the fused solver (csrc/solve_fused.hip), the rows per strip of the
streaming Gaussian (csrc/pyramid_ops.hip) and of the streaming medians (csrc/median.hip).  flow2d_context_set_planning_cus sets
the count they plan for; flow2d_fused_block_order_for_cus, flow2d_fused_plan_for_cus and flow2d_stream_rows_for_cus answer, without
a context, which plan a count gives.  Here:

  * a fixed-seed sweep of the strip planner and its launch order over geometries and CU counts: every block named once, every
    block column's strips a partition of the rows, no empty strip, border strips longer than the kernel's border band, dealt side
    blocks spread evenly;
  * the cases tests/test_gpu_planning_cus.py runs on the device, each in the class of plan it is named for (CASES, GROUPS);
  * the plans at 256 CUs of the levels bench.py's configurations solve with strips, against tests/golden/strip_plans_256.json
    (recorded by tests/golden/make_strip_plans_256.py before the planning count existed): the hot path plans as it did;
  * the setter and the getter on a zeroed stand-in for a context."""
import collections
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CU_COUNTS = (1, 4, 8, 16, 32, 36, 64, 80, 104, 128, 256, 304)
GROUP_SIZES = (1, 2, 3, 8)

# The strip-solver cases of the device tests.  expect: what the plan must be -- uniform or not, (rows_interior, rows_edge), strips per
# interior block column, block columns, blocks, whether the side blocks are dealt --; differs: the CU count whose plan this one is
# meant not to be.  Figures as csrc/solve_fused.hip plans them.
Case = collections.namedtuple("Case", "name w h cw ch inner cus expect differs")
Expect = collections.namedtuple("Expect", "uniform rows strips blocks_x blocks dealt")
CASES = [
    Case("uniform_180_rows", 417, 900, 448, 900, 5, 8, Expect(True, (180, 180), 5, 3, 15, False), 256),
    Case("sides_not_dealt", 417, 900, 417, 900, 5, 32, Expect(False, (55, 43), 17, 3, 59, False), 256),
    Case("dealt_sides_139_112", 1111, 777, 1120, 780, 1, 8, Expect(False, (139, 112), 6, 5, 32, True), 256),
    Case("dealt_sides_81_65", 1111, 777, 1120, 780, 5, 32, Expect(False, (81, 65), 10, 6, 64, True), 256),
    Case("two_border_strips", 1300, 64, 1312, 64, 2, 8, Expect(True, (32, 32), 2, 6, 12, False), 256),
    Case("one_block_column", 200, 300, 200, 300, 5, 1, Expect(True, (150, 150), 2, 1, 2, False), 256),
    Case("two_260_row_strips", 640, 520, 640, 520, 5, 4, Expect(True, (260, 260), 2, 4, 8, False), 256),
    Case("more_blocks_than_256_cus", 640, 1000, 640, 1000, 2, 304, Expect(True, (10, 10), 100, 3, 300, False), 256),
]
# inner 8 on the first case: two launches of four sweeps per outer iteration, the second continuing the first's
CHUNKED = Case("uniform_113_rows_chunks", 417, 900, 448, 900, 4, 8, Expect(True, (113, 113), 8, 2, 16, False), 256)
# Lock-step groups: (case, instances, split).  split: a single pair's plan has interior strips of 128 rows and more, so the group is
# launched instance by instance with THAT plan (expect describes it); otherwise expect is the plan of the shared launch.
GROUPS = [
    (Case("group_split", 417, 900, 448, 900, 5, 8, Expect(True, (180, 180), 5, 3, 15, False), 256), 3, True),
    (Case("group_shared_75_60", 417, 420, 448, 420, 5, 4, Expect(False, (75, 60), 6, 3, 20, False), 256), 3, False),
    (Case("group_sides_not_dealt_2", 509, 270, 512, 272, 5, 256, Expect(False, (14, 10), 20, 3, 74, False), 8), 2, False),
    (Case("group_sides_not_dealt_4", 645, 266, 704, 266, 3, 256, Expect(False, (19, 14), 15, 3, 53, False), 8), 4, False),
]
# the packed build's case: a lone context planning for 512 CUs takes a launch of 2048 x 1536 at inner 5 (at most one block per CU)
PACKED = Case("packed_508_blocks", 2048, 1536, 2048, 1536, 5, 512, Expect(False, (33, 25), 48, 10, 508, True), 256)
SPLIT_ROWS = 128  # launch_fused_outer: a group is launched instance by instance from this many interior rows on

# the streaming kernels' cases: (w, h, container w, container h), the planning counts they run under
STREAM_SIZES = [(700, 133, 704, 140), (257, 333, 300, 340), (61, 200, 64, 200)]
STREAM_CUS = (1, 2, 16, 1024)
STREAM_SIGMAS = (0.45, 1.5, 2.2)  # radii 1, 4, 6


def check_plan_class(flow2d, case, instances=1, split=False):
    """The plan the library gives `case` under its CU count is the one the case is named for, and not the plan of case.differs."""
    plan = flow2d.fused_plan_for_cus(case.cus, case.w, case.h, case.inner, 1 if split else instances)
    e = case.expect
    assert plan.uniform == e.uniform, (case.name, plan)
    assert (plan.rows_interior, plan.rows_edge) == e.rows, (case.name, plan)
    assert (plan.strips_interior, plan.blocks_x, plan.blocks) == (e.strips, e.blocks_x, e.blocks), (case.name, plan)
    assert (plan.side_blocks > 0) == e.dealt, (case.name, plan)
    if not e.uniform and not e.dealt:  # the branch of fused_block_of that finds a side block behind the interior ones
        assert plan.side_blocks == 0 and plan.blocks > (plan.blocks_x - 2) * plan.strips_interior
    lone = flow2d.fused_plan_for_cus(case.cus, case.w, case.h, case.inner, 1)
    assert (lone.rows_interior >= SPLIT_ROWS) == split or instances == 1, (case.name, lone)
    assert plan != flow2d.fused_plan_for_cus(case.differs, case.w, case.h, case.inner, 1 if split else instances), case.name
    return plan


class Orders:
    """flow2d_fused_block_order_for_cus into one buffer (the sweep asks thousands of times)."""

    def __init__(self, flow2d):
        self.lib = flow2d.hip_lib()
        self.cap = 1 << 19
        self.buf = (ctypes.c_int * (4 * self.cap))()

    def __call__(self, cus, w, h, inner, instances):
        grid = ctypes.c_size_t(0)
        rc = self.lib.flow2d_fused_block_order_for_cus(cus, w, h, inner, instances, self.buf, self.cap, ctypes.byref(grid))
        assert rc == 0, (rc, cus, w, h, inner, instances)
        return np.frombuffer(self.buf, np.int32, 4 * grid.value).reshape(-1, 4).copy()


def check_geometry(flow2d, orders, cus, w, h, inner, instances):
    what = (cus, w, h, inner, instances)
    plan = flow2d.fused_plan_for_cus(cus, w, h, inner, instances)
    order = orders(cus, w, h, inner, instances)
    assert len(order) % 8 == 0 and len(order) >= plan.blocks, what
    live = order[order[:, 0] >= 0]
    assert (order[order[:, 0] < 0] == -1).all(), what
    valid = 64 - 2 * (inner + 1)
    assert plan.blocks_x == (-(-w // valid) + 3) // 4, what
    # every block of the plan, once
    side_strips = -(-h // plan.rows_edge)
    if plan.uniform:
        want = {(bx, by) for bx in range(plan.blocks_x) for by in range(plan.strips_interior)}
    else:
        assert plan.blocks_x >= 3 and plan.strips_interior >= 3 and plan.rows_interior > plan.rows_edge, (what, plan)
        assert plan.rows_edge > inner + 4, (what, plan)  # the kernel's border band: a border strip's neighbour is an interior wave
        want = {(bx, by) for bx in range(1, plan.blocks_x - 1) for by in range(plan.strips_interior)}
        want |= {(bx, by) for bx in (0, plan.blocks_x - 1) for by in range(side_strips)}
    named = list(map(tuple, live[:, :2].tolist()))
    assert len(named) == plan.blocks == len(want) and set(named) == want, (what, plan, len(named))
    # every block column: no empty strip, and the strips tile [0, h)
    assert (live[:, 3] > live[:, 2]).all(), (what, plan, "an empty strip")
    for bx in range(plan.blocks_x):
        col = live[live[:, 0] == bx]
        col = col[np.argsort(col[:, 1])]
        assert col[0, 2] == 0 and col[-1, 3] == h and (col[1:, 2] == col[:-1, 3]).all(), (what, plan, bx)
    # dealt side blocks: the eight runs (launch ids k, k + 8, ...) carry them within one of each other
    if plan.side_blocks:
        assert plan.side_blocks == 2 * side_strips, (what, plan)
        per_run = [int(((order[k::8, 0] == 0) | (order[k::8, 0] == plan.blocks_x - 1)).sum()) for k in range(8)]
        assert sum(per_run) == plan.side_blocks and max(per_run) - min(per_run) <= 1, (what, plan, per_run)
    return plan


def named_shapes():
    shapes = {(c.w, c.h) for c in CASES + [CHUNKED, PACKED]} | {(g[0].w, g[0].h) for g in GROUPS}
    return sorted(shapes | {(4096, 4096), (8192, 8192), (1920, 1080), (584, 388), (700, 650)})


def test_sweep_of_plans_and_launch_orders(flow2d):
    orders = Orders(flow2d)
    rng = np.random.default_rng(20261020)
    seen = collections.Counter()
    for _ in range(3000):
        w, h = int(rng.integers(2, 3001)), int(rng.integers(2, 1501))
        inner, instances, cus = int(rng.integers(1, 6)), int(rng.choice(GROUP_SIZES)), int(rng.choice(CU_COUNTS))
        plan = check_geometry(flow2d, orders, cus, w, h, inner, instances)
        seen["uniform" if plan.uniform else "dealt" if plan.side_blocks else "not dealt"] += 1
    assert min(seen["uniform"], seen["dealt"], seen["not dealt"]) >= 100, seen  # the sweep reaches every kind of plan
    for w, h in named_shapes():
        for cus in CU_COUNTS:
            for inner in (1, 2, 3, 4, 5):
                for instances in GROUP_SIZES:
                    check_geometry(flow2d, orders, cus, w, h, inner, instances)


@pytest.mark.parametrize("case", CASES + [CHUNKED, PACKED], ids=lambda c: c.name)
def test_single_pair_cases_land_in_their_class(flow2d, case):
    plan = check_plan_class(flow2d, case)
    check_geometry(flow2d, Orders(flow2d), case.cus, case.w, case.h, case.inner, 1)
    if case is PACKED:  # one workgroup per planning CU at the most, which the device's own count (256) does not allow
        assert plan.blocks <= case.cus and flow2d.fused_plan_for_cus(256, case.w, case.h, case.inner).blocks > 256


@pytest.mark.parametrize("case,instances,split", GROUPS, ids=lambda g: getattr(g, "name", None))
def test_group_cases_land_in_their_class(flow2d, case, instances, split):
    check_plan_class(flow2d, case, instances, split)
    check_geometry(flow2d, Orders(flow2d), case.cus, case.w, case.h, case.inner, 1 if split else instances)


def test_whole_pipeline_case_is_strip_solved_under_two_plans(flow2d):
    """700 x 650 (tests/test_gpu_planning_cus.py's pyramid): above the tiles' 600 x 600, and four 163-row strips per column at 8 CUs
    where 304 CUs plan 14 / 10."""
    FUSED = 2
    assert flow2d.hip_lib().flow2d_solver_algorithm_for(0, 700, 650, flow2d.hip_lib().flow2d_plane_pitch_bytes(700), 2, 5, 0) == FUSED
    small, large = flow2d.fused_plan_for_cus(8, 700, 650, 5), flow2d.fused_plan_for_cus(304, 700, 650, 5)
    assert small.uniform and small.rows_interior == 163 and (large.rows_interior, large.rows_edge) == (14, 10) and large.side_blocks


def test_streaming_cases_reach_every_row_count(flow2d):
    """The sizes and planning counts of the device test give the medians strips of 8, 16, 32 and 64 rows and the Gaussian strips of 16,
    32, 64 and 128, among them tall strips (32 rows and more) whose last strip is ragged."""
    G, M = flow2d.STREAM_GAUSSIAN, flow2d.STREAM_MEDIAN
    median = {(w, h, cus): flow2d.stream_rows_for_cus(cus, M, w, h, 2) for w, h, _, _ in STREAM_SIZES for cus in STREAM_CUS}
    assert set(median.values()) == {8, 16, 32, 64}, median
    assert any(rows >= 32 and h % rows for (_, h, _), rows in median.items())
    for radius in (1, 3):  # the three windows take the same strips
        assert all(flow2d.stream_rows_for_cus(cus, M, w, h, radius) == rows for (w, h, cus), rows in median.items())
    gauss = {}
    for sigma in STREAM_SIGMAS:
        radius = flow2d.gaussian_kernel(sigma)[1]
        gauss.update({(w, h, cus, radius): flow2d.stream_rows_for_cus(cus, G, w, h, radius) for w, h, _, _ in STREAM_SIZES for cus in STREAM_CUS})
    assert {k[3] for k in gauss} == {1, 4, 6} and set(gauss.values()) == {16, 32, 64, 128}, gauss
    assert any(rows >= 64 and h % rows for (_, h, _, _), rows in gauss.items())
    # the rule itself, restated: halve from the tallest strip until there are 16 waves per CU, or the shortest strip is reached
    for (w, h, cus, radius), rows in gauss.items():
        strips = -(-w // (64 - 2 * radius))
        assert rows == 16 or strips * -(-h // rows) >= 16 * cus, (w, h, cus, radius, rows)
        assert rows == 128 or strips * -(-h // (2 * rows)) < 16 * cus, (w, h, cus, radius, rows)
    for (w, h, cus), rows in median.items():
        strips = -(-w // 60)
        assert rows == 8 or strips * -(-h // rows) >= 16 * cus, (w, h, cus, rows)
        assert rows == 64 or strips * -(-h // (2 * rows)) < 16 * cus, (w, h, cus, rows)
    # a lock-step group's instances count as waves; arguments outside the streaming kernels' ranges are refused
    assert flow2d.stream_rows_for_cus(2, M, 61, 200, 2, instances=4) == 64 and flow2d.stream_rows_for_cus(2, M, 61, 200, 2) == 8
    raw = flow2d.hip_lib().flow2d_stream_rows_for_cus
    for bad in ((0, M, 64, 64, 2, 1), (4097, M, 64, 64, 2, 1), (8, 2, 64, 64, 2, 1), (8, M, 64, 64, 4, 1), (8, G, 64, 64, 7, 1),
                (8, G, 64, 64, 0, 1), (8, G, 0, 64, 1, 1), (8, G, 64, 0, 1, 1), (8, G, 64, 64, 1, 0)):
        assert raw(*bad) == -1, bad


def test_plans_at_256_cus_are_the_recorded_ones(flow2d):
    """tests/golden/strip_plans_256.json: every pyramid level of bench.py's configurations, inner 1 ... 5 (5, the 4 + 4 of a chunked
    level, SOR's 2 and 4 stages), a single pair and the group sizes -- plan, grid and launch order as they were before the planning
    count existed.  The order is compared through a context without a count (what the fixture was recorded through), through a
    context set to 256 and through the host-only entry."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_strip_plans_256", os.path.join(ROOT, "tests", "golden", "make_strip_plans_256.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "strip_plans_256.json")))
    assert len(recorded) == len(maker.level_sizes()) * len(maker.INNER) * len(maker.INSTANCES) >= 900
    for size in ((4096, 4096), (2048, 2048), (1024, 1024), (1920, 1080), (960, 540), (8192, 8192), (584, 388), (526, 350)):
        assert size in maker.level_sizes(), size
    lib = flow2d.hip_lib()
    orders = Orders(flow2d)
    fake = ctypes.create_string_buffer(4096)
    assert lib.flow2d_context_set_planning_cus(ctypes.addressof(fake), 256) == 0
    sha = lambda order: hashlib.sha1(np.ascontiguousarray(order, "<i4").tobytes()).hexdigest()
    assert maker.records(lib) == recorded  # a context without a count
    for w, h, inner, instances, ri, re, strips, blocks_x, blocks, grid, digest in recorded:
        plan = flow2d.fused_plan_for_cus(256, w, h, inner, instances)
        assert tuple(plan)[:5] == (ri, re, strips, blocks_x, blocks), (w, h, inner, instances, plan)
        order = orders(256, w, h, inner, instances)
        assert len(order) == grid and sha(order) == digest, (w, h, inner, instances)
        assert maker.plan_of_order(order) == (ri, re, strips, blocks_x, blocks)
    for w, h, inner, instances, *_, digest in recorded[::7]:  # the context entry, on a context set to 256
        buf, grid = (ctypes.c_int * (4 * 4096))(), ctypes.c_size_t(0)
        rc = lib.flow2d_fused_block_order(ctypes.addressof(fake), w, h, inner, instances, buf, 4096, ctypes.byref(grid))
        if rc == 0:
            assert sha(np.frombuffer(buf, np.int32, 4 * grid.value).reshape(-1, 4)) == digest, (w, h, inner, instances)
        else:
            assert rc == 1 and grid.value > 4096  # (too small a buffer is refused with the grid reported)


def test_setter_and_getter_on_a_stand_in_context(flow2d):
    """flow2d_context_set_planning_cus / flow2d_context_planning_cus on a zeroed stand-in for a context (host logic only): the
    refusals leave the count as it was, a value is stored and plans follow it, and 0 goes back to the device's count -- which a
    zeroed context does not have, so the planners take 256."""
    lib = flow2d.hip_lib()
    fake = ctypes.create_string_buffer(4096)
    ctx = ctypes.addressof(fake)
    got = ctypes.c_int(-7)

    def count():
        assert lib.flow2d_context_planning_cus(ctx, ctypes.byref(got)) == 0
        return got.value

    def order(w, h, inner, instances=1):
        buf, grid = (ctypes.c_int * (4 * 4096))(), ctypes.c_size_t(0)
        assert lib.flow2d_fused_block_order(ctx, w, h, inner, instances, buf, 4096, ctypes.byref(grid)) == 0
        return np.frombuffer(buf, np.int32, 4 * grid.value).reshape(-1, 4).copy()

    assert count() == 256
    assert lib.flow2d_context_set_planning_cus(ctx, 8) == 0 and count() == 8
    assert np.array_equal(order(417, 900, 5), flow2d.fused_block_order_for_cus(8, 417, 900, 5))
    for bad in (-1, 4097, 1 << 20, -(1 << 31)):
        assert lib.flow2d_context_set_planning_cus(ctx, bad) == 1 and count() == 8, bad
    assert lib.flow2d_context_set_planning_cus(None, 8) == 1 and lib.flow2d_context_planning_cus(None, ctypes.byref(got)) == 1
    assert lib.flow2d_context_planning_cus(ctx, None) == 1
    for cus in (1, 304, 4096):
        assert lib.flow2d_context_set_planning_cus(ctx, cus) == 0 and count() == cus
        assert np.array_equal(order(640, 520, 5, 2), flow2d.fused_block_order_for_cus(cus, 640, 520, 5, 2)), cus
    assert lib.flow2d_context_set_planning_cus(ctx, 0) == 0 and count() == 256
    assert np.array_equal(order(417, 900, 5), flow2d.fused_block_order_for_cus(256, 417, 900, 5))
    # the host-only entries refuse what they cannot plan for
    plan, grid = (ctypes.c_int * 5)(), ctypes.c_size_t(0)
    buf = (ctypes.c_int * 64)()
    for cus, w, h, inner, instances in ((0, 64, 64, 5, 1), (4097, 64, 64, 5, 1), (8, 0, 64, 5, 1), (8, 64, 0, 5, 1), (8, 64, 64, 0, 1),
                                        (8, 64, 64, 6, 1), (8, 64, 64, 5, 0)):
        assert lib.flow2d_fused_plan_for_cus(cus, w, h, inner, instances, plan, None) == 1
        assert lib.flow2d_fused_block_order_for_cus(cus, w, h, inner, instances, buf, 16, ctypes.byref(grid)) == 1
    assert lib.flow2d_fused_plan_for_cus(8, 64, 64, 5, 1, None, None) == 1
    assert lib.flow2d_fused_block_order_for_cus(8, 417, 900, 5, 1, buf, 8, ctypes.byref(grid)) == 1 and grid.value == 16  # too small
    assert flow2d.Context.set_planning_cus.__doc__ and flow2d.Context.planning_cus.__doc__


def test_the_strips_end_where_their_32_bit_offsets_do(flow2d):
    """flow2d_solver_algorithm_for at the line height * pitch_bytes = 2^32 (fused_addressable, csrc/solve_fused.hip): a plane one
    row, or one pitch step, short of 4 GiB is the strips', a plane of exactly 4 GiB or more is the per-sweep kernels' under AUTO and
    refused where the strips are asked for.  tests/test_gpu_high_offsets.py runs the planes of the first two lines on the device."""
    AUTO, PER_SWEEP, FUSED = flow2d.SOLVER_AUTO, flow2d.SOLVER_PER_SWEEP, flow2d.SOLVER_FUSED
    pick = flow2d.hip_lib().flow2d_solver_algorithm_for
    MIB = 1 << 20
    # (width, height, pitch in bytes, the plane's bytes against 2^32)
    below = [(100, 4095, MIB, -MIB), (100, 4095, MIB + 256, -256), (200, 2048, 2 * MIB - 256, -2048 * 256), (100, 4096, MIB - 4, -4 * 4096)]
    beyond = [(100, 4096, MIB, 0), (100, 4095, MIB + 512, 4095 * 512 - MIB), (200, 2048, 2 * MIB, 0), (100, 4097, MIB - 4, MIB - 4 * 4097),
              (100, 4200, MIB, 104 * MIB)]
    for w, h, pitch, distance in below + beyond:
        assert h * pitch - (1 << 32) == distance, (h, pitch)
        assert w * h > 600 * 600  # (above the tiles' crossover: AUTO chooses between the strips and the per-sweep kernels)
    for constancy in (flow2d.GREY, flow2d.GRADIENT, flow2d.LOG_DERIVATIVES):
        for w, h, pitch, _ in below:
            for inner in (2, 5):
                assert pick(AUTO, w, h, pitch, 3, inner, constancy) == FUSED, (w, h, pitch, inner, constancy)
                assert pick(FUSED, w, h, pitch, 3, inner, constancy) == FUSED, (w, h, pitch, inner, constancy)
            assert pick(AUTO, w, h, pitch, 3, 1, constancy) == PER_SWEEP  # (a single sweep leaves nothing to fuse)
        for w, h, pitch, _ in beyond:
            for inner in (2, 5):
                assert pick(AUTO, w, h, pitch, 3, inner, constancy) == PER_SWEEP, (w, h, pitch, inner, constancy)
                assert pick(FUSED, w, h, pitch, 3, inner, constancy) == -1, (w, h, pitch, inner, constancy)
            assert pick(PER_SWEEP, w, h, pitch, 3, 5, constancy) == PER_SWEEP
    # the frame of the device test at inner 5 and 2: at most one workgroup per CU, the launch the packed build takes on a lone context
    for inner in (2, 5):
        assert flow2d.fused_plan_for_cus(256, 100, 4095, inner).blocks <= 256
