"""flow2d_node_strain_robust_2d on the device against the numpy restatement of tests/test_node_strain_robust_cpu.py, in the manner
of tests/test_gpu_node_strain.py: the nine planes and the three diagnostic planes byte for byte, the record's counts, reasons,
the three robust words, min and max exactly and its double sums within that file's derived bound; the smallest grids and grids
that cross the 64-column and the 4-row seams of the workgroups with outliers planted on either side of them, every window kind,
both orders, no reweighted pass, one and eight, a scale that rejects and one that does not; the plain entry's bytes from pass 0
alone, planes requested alone, containers larger than the data, a lock-step batch, a replayed graph and the refusals."""
import ctypes

import numpy as np
import pytest

from test_deformation_cpu import F32, GREEN, PLANES, SMALL, U32, bits
from test_gpu_batch_kernels import Tall, pitch_of, stride_of
from test_gpu_multipass import POISON
from test_gpu_node_strain import Field, check_record, poisoned_record, record_of
from test_node_strain_cpu import node_case
from test_node_strain_robust_cpu import DIAGNOSTICS, MAX_ITERATIONS, node_strain_robust_reference, robust_words

pytestmark = pytest.mark.gpu
ALL = PLANES + DIAGNOSTICS
GRIDS = [(1, 1), (3, 3), (5, 1), (67, 9), (130, 21)]
WINDOWS = [1, 2, 7]
PASSES = [(0, 1e6), (0, 0.05), (1, 0.05), (1, 1e6), (8, 0.05), (8, 1e6)]  # (K, sigma)


def planted_case(nw, nh, seed, holes=0.2):
    """node_case (noise of 0.01 px, lost nodes of every kind) with outliers of some pixels: on each side of the 64-column seam
    and of a 4-row seam where the grid has them, and one near the first corner."""
    u, v, state, grads = node_case(nw, nh, seed, holes)
    spots = [(1, 1), (3, 63), (4, 64), (7, 62), (8, 66), (11, 127), (12, 128)]
    for k, (j, i) in enumerate(spots):
        if j < nh and i < nw:
            u[j, i] += F32(2.5 + 0.25 * k)
            v[j, i] -= F32(1.5)
            state[j, i] = 9
    return u, v, state


class RobustField(Field):
    """A node field as tests/test_gpu_node_strain.py holds it, run through the robust entry."""

    def outputs(self, names=ALL):
        return super().outputs(names)

    def run(self, outs, record, s, m, order, measure, sigma, passes, min_state=1, min_nodes=None, state=True):
        self.ctx.node_strain_robust(self.u, self.v, self.nw, self.nh, s, m, order, min_nodes or 0, min_state, measure, sigma, passes,
                                    state=self.state if state else None, planes={n: q for n, q in outs.items() if n in PLANES},
                                    diagnostics={n: q for n, q in outs.items() if n in DIAGNOSTICS}, stats=record)

    def reference(self, s, m, order, measure, sigma, passes, min_state=1, min_nodes=None, state=True):
        u, v, st, _ = self.host
        return node_strain_robust_reference(u, v, st if state else None, s, m, order, min_nodes, min_state, measure, sigma, passes)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("m", WINDOWS)
@pytest.mark.parametrize("nw,nh", GRIDS)
def test_planes_diagnostics_and_record_match_the_definition(flow2d, ctx, nw, nh, m, order):
    u, v, state = planted_case(nw, nh, seed=m)
    field = RobustField(ctx, u, v, state)
    measure, s, min_state = (SMALL, 8, 1) if order == 1 else (GREEN, 3, 0)
    rejected = 0
    for passes, sigma in PASSES:
        for with_state in ((True, False) if passes == 8 else (True,)):
            outs, record = field.outputs(), poisoned_record(ctx)
            field.run(outs, record, s, m, order, measure, sigma, passes, min_state, state=with_state)
            ref = field.reference(s, m, order, measure, sigma, passes, min_state, state=with_state)
            what = "%dx%d m %d order %d K %d sigma %g state %s" % (nw, nh, m, order, passes, sigma, with_state)
            field.check(outs, ref, what)
            check_record(record_of(ctx, record)[0], ref, what)
            rejected += robust_words(ref)[1] if sigma < 1 else 0
            assert sigma < 1 or robust_words(ref) == [0, 0, 0], what
    # (the cases do what they are for: on the grids that hold the seams, taps were rejected)
    assert rejected > 0 or nw < 67


def test_pass_0_alone_gives_the_plain_entry_its_bytes(flow2d, ctx):
    """K = 0 with a sigma no residual reaches, against Context.node_strain on the device: planes and record."""
    nw, nh = 130, 21
    u, v, state = planted_case(nw, nh, seed=3)
    field = RobustField(ctx, u, v, state)
    for m, order, measure in ((1, 1, SMALL), (2, 2, GREEN), (7, 2, SMALL)):
        plain, plain_record = Field.outputs(field), poisoned_record(ctx)
        Field.run(field, plain, plain_record, 8, m, order, measure, grads=False)
        outs, record = field.outputs(), poisoned_record(ctx)
        field.run(outs, record, 8, m, order, measure, 1e6, 0)
        for name in PLANES:
            assert outs[name].download().tobytes() == plain[name].download().tobytes(), (m, order, name)
        assert record_of(ctx, record).tobytes() == record_of(ctx, plain_record).tobytes(), (m, order)
        got = outs["rejected"].download(nw, nh)
        valid = np.isfinite(plain["exx"].download(nw, nh))
        assert (got[valid] == 0).all() and np.isnan(got[~valid]).all() and 0 < valid.sum() < nw * nh


def test_subsets_cost_no_other_plane(flow2d, ctx):
    """Each of the twelve planes alone and the record alone: the requested plane is the full run's, the others keep their
    poison, and the record is the same bytes whatever goes with it."""
    nw, nh, s, m = 67, 9, 8, 2
    u, v, state = planted_case(nw, nh, seed=5)
    field = RobustField(ctx, u, v, state)
    ref = field.reference(s, m, 2, GREEN, 0.05, 8)
    full, full_record = field.outputs(), poisoned_record(ctx)
    field.run(full, full_record, s, m, 2, GREEN, 0.05, 8)
    field.check(full, ref, "all planes")
    assert robust_words(ref)[1] > 0
    want_record = record_of(ctx, full_record).tobytes()
    for names, with_record in [((name,), k % 2 == 0) for k, name in enumerate(ALL)] + [((), True), (DIAGNOSTICS, False)]:
        outs, record = field.outputs(), poisoned_record(ctx)
        field.run({name: outs[name] for name in names}, record if with_record else None, s, m, 2, GREEN, 0.05, 8)
        field.check({name: outs[name] for name in names}, ref, "subset %s" % (names,))
        for name in ALL:
            if name not in names:
                assert (outs[name].download().view(U32) == POISON).all(), (names, name)
        assert record_of(ctx, record).tobytes() == (want_record if with_record else bytes([0x7F]) * 256), names
    # the convenience form: planes and diagnostics by name, the record read back
    got, stats = ctx.node_strain_robust(field.u, field.v, nw, nh, s, m, 2, measure=GREEN, sigma=0.05, iterations=8, state=field.state,
                                        planes=("e1",), diagnostics=("rejected", "centre"))
    assert set(got) == {"e1", "rejected", "centre"} and bytes(stats) == want_record
    for name in got:
        assert np.array_equal(bits(got[name]), bits(ref[name])), name
    counts = flow2d.node_strain_robust_counts(stats)
    assert [counts[k] for k in ("touched", "rejected", "suspect")] == robust_words(ref)
    assert flow2d.NODE_STRAIN_DIAGNOSTICS == DIAGNOSTICS and flow2d.NODE_STRAIN_MAX_ITERATIONS == MAX_ITERATIONS
    assert flow2d.Context.node_strain_robust_workspace_bytes(nw, nh) == 224 * 2 * 3


def test_repeated_calls_and_a_replayed_graph_give_the_same_bytes(flow2d, ctx):
    nw, nh, s, m = 130, 21, 8, 2
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    u, v, state = planted_case(nw, nh, seed=6)
    field = RobustField(ctx, u, v, state)
    outs = [(field.outputs(), poisoned_record(ctx)) for _ in range(3)]

    def snapshot(k):
        return [outs[k][0][name].download().tobytes() for name in ALL] + [record_of(ctx, outs[k][1]).tobytes()]

    field.run(*outs[0], s, m, 2, GREEN, 0.05, 8)  # (also allocates the context's workspace)
    field.run(*outs[1], s, m, 2, GREEN, 0.05, 8)
    eager = snapshot(0)
    assert snapshot(1) == eager
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    try:
        field.run(*outs[2], s, m, 2, GREEN, 0.05, 8)
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
            for name, a, b in zip(ALL, got, eager):
                a, b = (np.frombuffer(q, U32).reshape(nh + 3, -1)[:nh, :nw] for q in (a, b))
                assert np.array_equal(a, b), name
            assert got[-1] == eager[-1]
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)
    field.check(outs[0][0], field.reference(s, m, 2, GREEN, 0.05, 8), "130x21")


def test_lock_step_batch(flow2d, ctx):
    """Three instances a padded stride apart, the second all NaN: planes, diagnostics and record of instance b are the bytes of
    the same input analysed alone and the restatement's, and every other word of the output allocations is what it was."""
    nw, nh, cw, ch, count, s, m = 67, 9, 80, 12, 3, 8, 2
    stride = stride_of("rows", pitch_of(cw), ch)
    cases = [planted_case(nw, nh, seed=20 + b) for b in range(count)]
    cases[1] = (np.full((nh, nw), np.nan, F32), np.full((nh, nw), np.nan, F32), cases[1][2])
    fill = lambda arrays: Tall(ctx, cw, ch, count, stride).fill(arrays)  # noqa: E731
    tu, tv, ts = (fill([c[k] for c in cases]) for k in range(3))
    outs = {name: Tall(ctx, cw, ch, count, stride) for name in ALL}
    records = poisoned_record(ctx, count)
    with ctx.set_batch(count, stride):
        ctx.node_strain_robust(tu, tv, nw, nh, s, m, 2, measure=GREEN, sigma=0.05, iterations=8, state=ts,
                               planes={n: outs[n] for n in PLANES}, diagnostics={n: outs[n] for n in DIAGNOSTICS}, stats=records,
                               instances=count)
    ctx.synchronize()
    refs = [node_strain_robust_reference(c[0], c[1], c[2], s, m, 2, measure=GREEN, sigma=0.05, iterations=8) for c in cases]
    assert not refs[1]["valid"].any() and int(refs[1]["stats"]["reserved"][0][0]) == nw * nh
    for name in ALL:
        outs[name].check([r[name] for r in refs], name)
    got = record_of(ctx, records, count)
    for b, (c, ref) in enumerate(zip(cases, refs)):
        alone = {name: ctx.plane(cw, ch).fill_bytes(0x7F) for name in ALL}
        record = poisoned_record(ctx)
        ctx.node_strain_robust(ctx.plane(cw, ch, c[0]), ctx.plane(cw, ch, c[1]), nw, nh, s, m, 2, measure=GREEN, sigma=0.05, iterations=8,
                               state=ctx.plane(cw, ch, c[2]), planes={n: alone[n] for n in PLANES},
                               diagnostics={n: alone[n] for n in DIAGNOSTICS}, stats=record)
        assert record_of(ctx, record).tobytes() == got[b:b + 1].tobytes(), "record of instance %d" % b
        for name in ALL:
            assert np.array_equal(alone[name].download(nw, nh).view(U32), bits(ref[name])), (b, name)
        check_record(got[b], ref, "instance %d" % b)
    for t in (tu, tv, ts):
        t.check(None, "an input")
    # a written range must not meet a later instance of an input or of another output, and one slice is no workspace for three
    lib = flow2d.hip_lib()
    need, ws = ctx._node_strain_robust_workspace

    def call(planes, diag, record=records.ptr, ws_bytes=need):
        out, dg = flow2d.DeformationPlanes(**planes), flow2d.NodeStrainDiagnostics(**diag)
        return lib.flow2d_node_strain_robust_2d(ctx.handle, tu.ptr, tv.ptr, ts.ptr, nw, nh, tu.pitch, s, m, 2, 7, 1, GREEN, 0.05, 8,
                                                ctypes.byref(out), ctypes.byref(dg), record, ws.ptr, ws_bytes)

    e1, res = outs["e1"].ptr, outs["residual"].ptr
    with ctx.set_batch(count, stride):
        assert call({}, {"residual": tv.ptr + 2 * stride}) == 1
        assert call({"e1": e1}, {"centre": e1 + stride}) == 1
        assert call({}, {"residual": res, "rejected": res + 2 * stride}) == 1
        assert call({}, {"residual": res}, record=ws.ptr + need - 256) == 1
        assert call({}, {"residual": res}, ws_bytes=lib.flow2d_node_strain_robust_workspace_bytes(nw, nh, 1)) == 1
        assert call({"e1": e1}, {"residual": res}) == 0
    ctx.synchronize()


def test_invalid_arguments_write_nothing(flow2d, ctx):
    nw, nh = 40, 30
    lib = flow2d.hip_lib()
    u, v, state = planted_case(nw, nh, seed=8)
    pu, pv, ps = (ctx.plane(nw, nh, a) for a in (u, v, state))
    outs = {name: ctx.plane(nw, nh).fill_bytes(0x7F) for name in ALL}
    record = poisoned_record(ctx)
    need = lib.flow2d_node_strain_robust_workspace_bytes(nw, nh, 1)
    assert need % 16 == 0 and need == lib.flow2d_node_strain_robust_workspace_bytes(nw, nh, 2) // 2
    ws = ctx.plane(need // 4, 1).fill_bytes(0x7F)
    span = pu.pitch * nh
    d = dict(u=pu.ptr, v=pv.ptr, state=ps.ptr, nw=nw, nh=nh, pitch=pu.pitch, s=8, m=2, order=1, min_nodes=4, min_state=1, measure=SMALL,
             sigma=0.05, iterations=8, stats=record.ptr, ws=ws.ptr, ws_bytes=need, planes={name: outs[name].ptr for name in PLANES},
             diag={name: outs[name].ptr for name in DIAGNOSTICS}, out=True, diagnostics=True)

    def call(**kw):
        a = dict(d, **kw)
        out, dg = flow2d.DeformationPlanes(**a["planes"]), flow2d.NodeStrainDiagnostics(**a["diag"])
        return lib.flow2d_node_strain_robust_2d(ctx.handle, a["u"], a["v"], a["state"], a["nw"], a["nh"], a["pitch"], a["s"], a["m"],
                                                a["order"], a["min_nodes"], a["min_state"], a["measure"], a["sigma"], a["iterations"],
                                                ctypes.byref(out) if a["out"] else None, ctypes.byref(dg) if a["diagnostics"] else None,
                                                a["stats"], a["ws"], a["ws_bytes"])

    e1, res = outs["e1"].ptr, outs["residual"].ptr
    bad = [dict(u=None), dict(v=None), dict(out=False, diagnostics=False, stats=None), dict(planes={}, diag={}, stats=None), dict(nw=0),
           dict(nh=0), dict(pitch=pu.pitch + 8), dict(pitch=16), dict(s=0), dict(s=65), dict(m=0), dict(m=-1), dict(m=8), dict(order=0),
           dict(order=3), dict(min_nodes=2), dict(min_nodes=26), dict(order=2, min_nodes=5), dict(m=1, min_nodes=10), dict(min_state=-1),
           dict(min_state=2), dict(measure=2), dict(measure=-1), dict(sigma=0.0), dict(sigma=-0.05), dict(sigma=float("nan")),
           dict(sigma=float("inf")), dict(iterations=-1), dict(iterations=MAX_ITERATIONS + 1), dict(state=ps.ptr + 4),
           dict(stats=record.ptr + 4), dict(ws=ws.ptr + 8), dict(ws=None), dict(ws_bytes=need - 1), dict(planes={"divergence": pu.ptr}),
           dict(diag={"residual": pu.ptr}), dict(diag={"rejected": pv.ptr + pu.pitch}), dict(diag={"centre": ps.ptr}),
           dict(diag={"residual": e1}), dict(diag={"residual": res, "centre": res}), dict(diag={"residual": res, "rejected": res + span - pu.pitch}),
           dict(diag={"residual": res + 4}), dict(stats=pu.ptr + 64), dict(stats=res), dict(ws=pv.ptr), dict(ws=outs["centre"].ptr),
           dict(stats=ws.ptr + 16), dict(stats=ws.ptr + need - 8)]
    for kw in bad:
        assert call(**kw) == 1, kw
    assert call(nw=1 << 16, nh=1 << 15, pitch=4 << 16) == 5  # 2^31 nodes
    with ctx.set_batch(2, span):
        assert call() == 1  # a workspace for one instance under a batch of two
    ctx.synchronize()
    for name, q in outs.items():
        assert (q.download().view(U32) == POISON).all(), name
    assert set(record.download(64, 1).tobytes()) == {0x7F} and (ws.download().view(U32) == POISON).all()
    # without statistics the workspace takes no part, whatever it is; a diagnostic plane alone is output enough
    assert call(stats=None, ws=pv.ptr, ws_bytes=0, planes={}, out=False, diag={"rejected": outs["rejected"].ptr}) == 0
    ctx.synchronize()
    assert set(record.download(64, 1).tobytes()) == {0x7F} and (ws.download().view(U32) == POISON).all()
    ref = node_strain_robust_reference(u, v, state, 8, 2, 1, 4, sigma=0.05, iterations=8)
    assert np.array_equal(outs["rejected"].download().view(U32), bits(ref["rejected"]))
    assert call(iterations=MAX_ITERATIONS) == 0 and call() == 0
    for name, q in outs.items():
        assert np.array_equal(q.download().view(U32), bits(ref[name])), name
    check_record(record_of(ctx, record)[0], ref, "after the refusals")
