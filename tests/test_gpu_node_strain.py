"""flow2d_node_strain_2d on the device against the numpy restatement of tests/test_node_strain_cpu.py: every plane byte for
byte, the record's counts, reasons, min and max exactly and its double sums within the summation-order bound that
tests/test_gpu_deformation.py derives; the smallest grids, grids that cross a workgroup with the window reaching over the seam,
every window, order, measure and spacing, lost nodes of every kind, planes requested alone, containers larger than the data,
a lock-step batch, a replayed graph and the refusals."""
import ctypes

import numpy as np
import pytest

from test_deformation_cpu import F32, GREEN, PLANES, SMALL, STAT_NAMES, STATS_DTYPE, U32, bits
from test_gpu_batch_kernels import Tall, pitch_of, stride_of
from test_gpu_multipass import POISON, padded
from test_node_strain_cpu import node_case, node_strain_reference

pytestmark = pytest.mark.gpu
# the smallest grids, a grid that crosses a 64-wide workgroup (and three 4-row ones) and one of three by six workgroups
GRIDS = [(1, 1), (2, 2), (3, 3), (5, 1), (1, 6), (67, 9), (130, 21)]
WINDOWS = [0, 1, 2, 7]
# (order, measure, spacing, min_state, min_nodes or None for k + 1): both orders and measures, the three spacings
FORMS = [(1, SMALL, 8, 1, None), (2, GREEN, 1, 0, None), (1, GREEN, 64, 0, 3), (2, SMALL, 8, 1, 6)]


def poisoned_record(ctx, instances=1):
    return ctx.deformation_records(instances).fill_bytes(0x7F)


def record_of(ctx, record, instances=1):
    return np.frombuffer(record.download(instances * 64, 1).tobytes(), STATS_DTYPE)


def check_record(got, ref, what):
    """Counts, reasons, min and max exact; the double sums within n * 2^-52 * sum|term| of the restatement's: the worst case of
    any two orders of n additions of exactly representable terms (tests/test_gpu_deformation.py).  Derived, not measured."""
    want = ref["stats"][0]
    n = int(want["valid"])
    assert got["valid"] == n and got["invalid"] == want["invalid"], what
    assert np.array_equal(got["reserved"], want["reserved"]), (what, got["reserved"][:3], want["reserved"][:3])
    for name in STAT_NAMES:
        assert got[name]["min"] == want[name]["min"] and got[name]["max"] == want[name]["max"], (what, name)
        for field, total in (("sum", ref["abs_sum"][name]), ("sum_sq", ref["abs_sum_sq"][name])):
            bound = n * 2.0 ** -52 * total
            print("%s %s.%s: |difference| %.3g, bound %.3g" % (what, name, field, abs(got[name][field] - want[name][field]), bound))
            assert abs(got[name][field] - want[name][field]) <= bound, (what, name, field)


class Field:
    """A node field in containers 5 columns wider and 3 rows taller than the grid, the padding NaN."""

    def __init__(self, ctx, u, v, state=None, grads=None):
        self.ctx = ctx
        self.nh, self.nw = u.shape
        self.host = (u, v, state, grads)
        self.u, self.v = padded(ctx, u), padded(ctx, v)
        self.state = None if state is None else padded(ctx, state)
        self.grads = None if grads is None else [padded(ctx, g) for g in grads]

    def outputs(self, names=PLANES):
        return {name: self.ctx.plane(self.nw + 5, self.nh + 3).fill_bytes(0x7F) for name in names}

    def run(self, planes, record, s, m, order, measure, min_state=1, min_nodes=None, state=True, grads=True):
        self.ctx.node_strain(self.u, self.v, self.nw, self.nh, s, m, order, min_nodes or 0, min_state, measure,
                             state=self.state if state else None, gradients=self.grads if grads else None, planes=planes,
                             stats=record)

    def reference(self, s, m, order, measure, min_state=1, min_nodes=None, state=True):
        u, v, st, grads = self.host
        return node_strain_reference(u, v, st if state else None, grads, s, m, order, min_nodes, min_state, measure)

    def check(self, planes, ref, what):
        for name, plane in planes.items():
            got = plane.download().view(U32)
            assert np.array_equal(got[:self.nh, :self.nw], bits(ref[name])), "%s: %s" % (what, name)
            assert (got[self.nh:] == POISON).all() and (got[:, self.nw:] == POISON).all(), "%s: %s beyond the grid" % (what, name)


@pytest.mark.parametrize("m", WINDOWS)
@pytest.mark.parametrize("nw,nh", GRIDS)
def test_planes_and_record_match_the_definition(flow2d, ctx, nw, nh, m):
    """Seeded holes of every state, a NaN and an infinity at a usable state, a NaN state, predicted (65) and unconverged (0)
    nodes, with and without the state plane."""
    u, v, state, grads = node_case(nw, nh, seed=m)
    field = Field(ctx, u, v, state, grads)
    for order, measure, s, min_state, min_nodes in FORMS:
        if min_nodes is not None and min_nodes > (2 * m + 1) ** 2:
            min_nodes = None
        if m >= 1 and (3, 6)[order - 1] + (min_nodes is None) > (2 * m + 1) ** 2:
            continue
        for with_state in (True, False):
            planes, record = field.outputs(), poisoned_record(ctx)
            field.run(planes, record, s, m, order, measure, min_state, min_nodes, state=with_state)
            ref = field.reference(s, m, order, measure, min_state, min_nodes, state=with_state)
            what = "%dx%d m %d order %d measure %d s %d min_state %d state %s" % (nw, nh, m, order, measure, s, min_state, with_state)
            field.check(planes, ref, what)
            check_record(record_of(ctx, record)[0], ref, what)


def test_min_state_and_full_grid(flow2d, ctx):
    """min_state 0 against 1 with state-0 and state-65 nodes present, and a full grid where every window away from the border
    is whole."""
    nw, nh = 67, 9
    u, v, state, grads = node_case(nw, nh, seed=11)
    assert (state == 0).any() and (state == 65).any()
    field = Field(ctx, u, v, state, grads)
    valid = []
    for min_state in (0, 1):
        planes, record = field.outputs(("exx",)), poisoned_record(ctx)
        field.run(planes, record, 8, 2, 1, SMALL, min_state)
        ref = field.reference(8, 2, 1, SMALL, min_state)
        field.check(planes, ref, "min_state %d" % min_state)
        check_record(record_of(ctx, record)[0], ref, "min_state %d" % min_state)
        valid.append(ref["valid"])
        assert ref["valid"][state == 65].any()
    assert valid[0][state == 0].any() and not valid[1][state == 0].any()
    full_u, full_v, _, _ = node_case(nw, nh, seed=12, holes=0.0)
    full_u, full_v = np.nan_to_num(full_u, nan=0.5, posinf=0.25), np.nan_to_num(full_v, nan=0.5, posinf=0.25)
    full = Field(ctx, full_u, full_v)
    for m, order in ((2, 1), (7, 2), (3, 2)):
        planes, record = full.outputs(), poisoned_record(ctx)
        full.run(planes, record, 8, m, order, GREEN)
        ref = full.reference(8, m, order, GREEN)
        assert ref["valid"].all()
        full.check(planes, ref, "full grid m %d order %d" % (m, order))
        check_record(record_of(ctx, record)[0], ref, "full grid m %d order %d" % (m, order))


def test_subsets_cost_no_other_plane(flow2d, ctx):
    """Each plane alone and the record alone: the requested plane is the full run's, the others keep their poison, and the
    record is the same bytes whatever planes go with it."""
    nw, nh, s, m = 67, 9, 8, 2
    u, v, state, grads = node_case(nw, nh, seed=5)
    field = Field(ctx, u, v, state, grads)
    ref = field.reference(s, m, 2, GREEN)
    full, full_record = field.outputs(), poisoned_record(ctx)
    field.run(full, full_record, s, m, 2, GREEN)
    field.check(full, ref, "all planes")
    want_record = record_of(ctx, full_record).tobytes()
    for names, with_record in [((name,), k % 2 == 0) for k, name in enumerate(PLANES)] + [((), True), (("exx", "e2"), False)]:
        planes, record = field.outputs(), poisoned_record(ctx)
        field.run({name: planes[name] for name in names}, record if with_record else None, s, m, 2, GREEN)
        field.check({name: planes[name] for name in names}, ref, "subset %s" % (names,))
        for name in PLANES:
            if name not in names:
                assert (planes[name].download().view(U32) == POISON).all(), (names, name)
        got = record_of(ctx, record).tobytes()
        assert got == (want_record if with_record else bytes([0x7F]) * 256), names
    # the direct form reads the gradient planes; the window form does not need them
    planes = field.outputs(("vorticity",))
    field.run(planes, None, s, m, 1, SMALL, grads=False)
    field.check(planes, field.reference(s, m, 1, SMALL), "without gradient planes")
    # the convenience form: planes by name, the record read back
    got, stats = ctx.node_strain(field.u, field.v, nw, nh, s, m, 2, measure=GREEN, state=field.state, planes=("e1", "vorticity"))
    assert set(got) == {"e1", "vorticity"} and bytes(stats) == want_record
    for name in got:
        assert np.array_equal(bits(got[name]), bits(ref[name])), name
    assert list(stats.reserved[:3]) == [int(x) for x in ref["stats"]["reserved"][0][:3]]
    assert flow2d.Context.node_strain_workspace_bytes(nw, nh) == flow2d.hip_lib().flow2d_node_strain_workspace_bytes(nw, nh, 1) > 0
    assert flow2d.Context.node_strain_workspace_bytes(0, nh) == 0


def test_repeated_calls_and_a_replayed_graph_give_the_same_bytes(flow2d, ctx):
    nw, nh, s, m = 130, 21, 8, 2
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    u, v, state, grads = node_case(nw, nh, seed=6)
    field = Field(ctx, u, v, state, grads)
    outs = [(field.outputs(), poisoned_record(ctx)) for _ in range(3)]

    def snapshot(k):
        return [outs[k][0][name].download().tobytes() for name in PLANES] + [record_of(ctx, outs[k][1]).tobytes()]

    field.run(*outs[0], s, m, 2, GREEN)  # (also allocates the context's workspace)
    field.run(*outs[1], s, m, 2, GREEN)
    eager = snapshot(0)
    assert snapshot(1) == eager
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    try:
        field.run(*outs[2], s, m, 2, GREEN)
    finally:
        graph = vp()
        assert lib.flow2d_capture_end(ctx.handle, ctypes.byref(graph)) == 0
    try:
        ctx.synchronize()
        assert all(set(x) == {0x7F} for x in snapshot(2))  # captured, not run
        for _ in range(2):
            for q in list(outs[2][0].values()) + [outs[2][1]]:
                q.fill_bytes(0x3C)
            assert lib.flow2d_graph_launch(ctx.handle, graph) == 0
            ctx.synchronize()
            got = snapshot(2)
            # (the words beyond the grid hold the other poison now: compare the grid and the record)
            for name, a, b in zip(PLANES, got, eager):
                a, b = (np.frombuffer(q, U32).reshape(nh + 3, -1)[:nh, :nw] for q in (a, b))
                assert np.array_equal(a, b), name
            assert got[-1] == eager[-1]
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)
    field.check(outs[0][0], field.reference(s, m, 2, GREEN), "130x21")


def test_lock_step_batch(flow2d, ctx):
    """Three instances a padded stride apart: planes and record of instance b are the bytes of the same input analysed alone
    and the restatement's planes, and every other word of the output allocations is what it was."""
    nw, nh, cw, ch, count, s, m = 67, 9, 80, 12, 3, 8, 2
    stride = stride_of("rows", pitch_of(cw), ch)
    cases = [node_case(nw, nh, seed=20 + b) for b in range(count)]
    fill = lambda arrays: Tall(ctx, cw, ch, count, stride).fill(arrays)  # noqa: E731
    tu, tv, ts = (fill([c[k] for c in cases]) for k in range(3))
    outs = {name: Tall(ctx, cw, ch, count, stride) for name in PLANES}
    records = poisoned_record(ctx, count)
    with ctx.set_batch(count, stride):
        ctx.node_strain(tu, tv, nw, nh, s, m, 2, measure=GREEN, state=ts, planes=outs, stats=records, instances=count)
    ctx.synchronize()
    refs = [node_strain_reference(c[0], c[1], c[2], None, s, m, 2, measure=GREEN) for c in cases]
    for name in PLANES:
        outs[name].check([r[name] for r in refs], name)
    got = record_of(ctx, records, count)
    for b, (c, ref) in enumerate(zip(cases, refs)):
        planes = {name: ctx.plane(cw, ch).fill_bytes(0x7F) for name in PLANES}
        record = poisoned_record(ctx)
        ctx.node_strain(ctx.plane(cw, ch, c[0]), ctx.plane(cw, ch, c[1]), nw, nh, s, m, 2, measure=GREEN, state=ctx.plane(cw, ch, c[2]),
                        planes=planes, stats=record)
        assert record_of(ctx, record).tobytes() == got[b:b + 1].tobytes(), "record of instance %d" % b
        for name in PLANES:
            assert np.array_equal(planes[name].download(nw, nh).view(U32), bits(ref[name])), (b, name)
        check_record(got[b], ref, "instance %d" % b)
    assert len({got[b:b + 1].tobytes() for b in range(count)}) == count
    for t in (tu, tv, ts):
        t.check(None, "an input")
    # a written range must not meet a later instance of an input or of another output, and one slice is no workspace for three
    lib = flow2d.hip_lib()
    need, ws = ctx._node_strain_workspace

    def call(planes, record=records.ptr, ws_bytes=need):
        out = flow2d.DeformationPlanes(**planes)
        return lib.flow2d_node_strain_2d(ctx.handle, tu.ptr, tv.ptr, ts.ptr, None, None, None, None, nw, nh, tu.pitch, s, m, 2, 7, 1,
                                         GREEN, ctypes.byref(out), record, ws.ptr, ws_bytes)

    with ctx.set_batch(count, stride):
        assert call({"e1": tv.ptr + 2 * stride}) == 1
        assert call({"e1": outs["e1"].ptr, "e2": outs["e1"].ptr + stride}) == 1
        assert call({"e1": outs["e1"].ptr}, record=ws.ptr + need - 256) == 1
        assert call({"e1": outs["e1"].ptr}, ws_bytes=lib.flow2d_node_strain_workspace_bytes(nw, nh, 1)) == 1
        assert call({"e1": outs["e1"].ptr}) == 0
    ctx.synchronize()


def test_invalid_arguments_write_nothing(flow2d, ctx):
    nw, nh = 40, 30
    lib = flow2d.hip_lib()
    u, v, state, grads = node_case(nw, nh, seed=8)
    pu, pv, ps = (ctx.plane(nw, nh, a) for a in (u, v, state))
    pg = [ctx.plane(nw, nh, g) for g in grads]
    outs = {name: ctx.plane(nw, nh).fill_bytes(0x7F) for name in PLANES}
    record = poisoned_record(ctx)
    need = lib.flow2d_node_strain_workspace_bytes(nw, nh, 1)
    assert need % 16 == 0 and need == lib.flow2d_node_strain_workspace_bytes(nw, nh, 2) // 2
    ws = ctx.plane(need // 4, 1).fill_bytes(0x7F)
    span = pu.pitch * nh
    d = dict(u=pu.ptr, v=pv.ptr, state=ps.ptr, grads=[q.ptr for q in pg], nw=nw, nh=nh, pitch=pu.pitch, s=8, m=2, order=1, min_nodes=4,
             min_state=1, measure=SMALL, stats=record.ptr, ws=ws.ptr, ws_bytes=need, planes={name: q.ptr for name, q in outs.items()},
             out=True)

    def call(**kw):
        a = dict(d, **kw)
        out = flow2d.DeformationPlanes(**a["planes"])
        return lib.flow2d_node_strain_2d(ctx.handle, a["u"], a["v"], a["state"], *a["grads"], a["nw"], a["nh"], a["pitch"], a["s"], a["m"],
                                         a["order"], a["min_nodes"], a["min_state"], a["measure"],
                                         ctypes.byref(out) if a["out"] else None, a["stats"], a["ws"], a["ws_bytes"])

    e1 = outs["e1"].ptr
    none = [None] * 4
    bad = [dict(u=None), dict(v=None), dict(out=False, stats=None), dict(planes={}, stats=None), dict(nw=0), dict(nh=0),
           dict(pitch=pu.pitch + 8), dict(pitch=16), dict(s=0), dict(s=65), dict(m=-1), dict(m=8), dict(order=0), dict(order=3),
           dict(min_nodes=2), dict(min_nodes=26), dict(order=2, min_nodes=5), dict(m=1, min_nodes=10), dict(min_state=-1),
           dict(min_state=2), dict(measure=2), dict(measure=-1), dict(m=0, grads=none), dict(grads=[pg[0].ptr, None, pg[2].ptr, pg[3].ptr]),
           dict(m=0, grads=[None, None, None, pg[3].ptr]), dict(grads=[pg[0].ptr + 4] + [q.ptr for q in pg[1:]]),
           dict(state=ps.ptr + 4), dict(stats=record.ptr + 4), dict(ws=ws.ptr + 8), dict(ws=None), dict(ws_bytes=need - 1),
           dict(planes={"divergence": pu.ptr}), dict(planes={"max_shear": pv.ptr + pu.pitch}), dict(planes={"exx": ps.ptr}),
           dict(planes={"eyy": pg[1].ptr}), dict(planes={"exx": e1, "exy": e1}), dict(planes={"e1": e1, "e2": e1 + span - pu.pitch}),
           dict(stats=pu.ptr + 64), dict(stats=e1), dict(ws=pv.ptr), dict(ws=outs["exy"].ptr), dict(stats=ws.ptr + 16),
           dict(stats=ws.ptr + need - 8)]
    for kw in bad:
        assert call(**kw) == 1, kw
    assert call(nw=1 << 16, nh=1 << 15, pitch=4 << 16) == 5  # 2^31 nodes
    with ctx.set_batch(2, span):
        assert call() == 1  # a workspace for one instance under a batch of two
    ctx.synchronize()
    for name, q in outs.items():
        assert (q.download().view(U32) == POISON).all(), name
    assert set(record.download(64, 1).tobytes()) == {0x7F} and (ws.download().view(U32) == POISON).all()
    # without statistics the workspace takes no part, whatever it is; the direct form looks at neither order nor min_nodes
    assert call(stats=None, ws=None, ws_bytes=0, planes={"vorticity": outs["vorticity"].ptr}) == 0
    assert call(stats=None, ws=pv.ptr, ws_bytes=0, planes={"exx": outs["exx"].ptr}, m=0, order=0, min_nodes=0) == 0
    ctx.synchronize()
    assert set(record.download(64, 1).tobytes()) == {0x7F} and (ws.download().view(U32) == POISON).all()
    assert np.array_equal(outs["exx"].download().view(U32), bits(node_strain_reference(u, v, state, grads, 8, 0)["exx"]))
    assert call(grads=none) == 0
    ref = node_strain_reference(u, v, state, None, 8, 2, 1, 4)
    for name, q in outs.items():
        assert np.array_equal(q.download().view(U32), bits(ref[name])), name
    check_record(record_of(ctx, record)[0], ref, "after the refusals")
