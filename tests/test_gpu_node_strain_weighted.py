"""flow2d_node_strain_weighted_2d on the device against the numpy restatement of tests/test_node_strain_weighted_cpu.py, in the
manner of tests/test_gpu_node_strain_robust.py: the nine planes, the three diagnostic planes and the nine sigma planes byte for
byte, the record's counts, reasons, the four further words, min and max exactly and its double sums within
tests/test_gpu_node_strain.py's derived bound; a grid that crosses the 64-column and the 4-row seams of the workgroups and the
smallest ones, every window kind, both orders and measures, T = 0 and T = 3 with four passes, lost nodes, sigmas that are NaN or
zero; the two exact properties of the header against the plain entry's device bytes, planes requested alone, a lock-step batch,
a replayed graph and the refusals."""
import ctypes

import numpy as np
import pytest

from test_deformation_cpu import F32, GREEN, PLANES, SMALL, U32, bits
from test_gpu_batch_kernels import Tall, pitch_of, stride_of
from test_gpu_multipass import POISON, padded
from test_gpu_node_strain import Field, check_record, poisoned_record, record_of
from test_gpu_node_strain_robust import planted_case
from test_node_strain_robust_cpu import DIAGNOSTICS, MAX_ITERATIONS
from test_node_strain_weighted_cpu import SIGMAS, node_strain_weighted_reference, sigma_case, weighted_words

pytestmark = pytest.mark.gpu
ALL = PLANES + DIAGNOSTICS + SIGMAS
GRIDS = [(70, 9), (5, 5), (3, 1)]
WINDOWS = [1, 2, 7]
ROBUST = [(0.0, 0), (3.0, 4)]  # (T, K)


def weighted_case(nw, nh, seed, holes=0.2):
    """planted_case -- noise of 0.01 px, 20 % lost nodes of every kind, outliers of some pixels on both sides of the seams -- with
    sigma planes that vary by a decade between neighbours and hold a NaN, a zero and an infinity at usable nodes."""
    u, v, state = planted_case(nw, nh, seed, holes)
    su, sv = sigma_case(nw, nh, seed)
    rng = np.random.default_rng(seed + 31 * nw + nh)
    usable = np.flatnonzero((state >= 1) & np.isfinite(u) & np.isfinite(v))
    spots = rng.permutation(usable)[:4]
    for k, q in enumerate(spots):
        (su if k % 2 else sv).flat[q] = (np.nan, 0.0, 0.0, np.inf)[k]
    return u, v, state, su, sv


class WeightedField(Field):
    """A node field as tests/test_gpu_node_strain.py holds it, with its two sigma planes, run through the weighted entry."""

    def __init__(self, ctx, u, v, state, su, sv):
        super().__init__(ctx, u, v, state)
        self.sigma_host = (su, sv)
        self.su, self.sv = padded(ctx, su), padded(ctx, sv)

    def outputs(self, names=ALL):
        return super().outputs(names)

    def run(self, outs, record, s, m, order, measure, floor, threshold, passes, min_state=1, min_nodes=None, state=True):
        pick = lambda names: {n: q for n, q in outs.items() if n in names}  # noqa: E731
        self.ctx.node_strain_weighted(self.u, self.v, self.su, self.sv, self.nw, self.nh, s, m, order, min_nodes or 0, min_state, measure,
                                      floor, threshold, passes, state=self.state if state else None, planes=pick(PLANES),
                                      diagnostics=pick(DIAGNOSTICS), sigmas=pick(SIGMAS), stats=record)

    def reference(self, s, m, order, measure, floor, threshold, passes, min_state=1, min_nodes=None, state=True):
        u, v, st, _ = self.host
        su, sv = self.sigma_host
        return node_strain_weighted_reference(u, v, su, sv, st if state else None, s, m, order, min_nodes, min_state, measure, floor,
                                              threshold, passes)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("m", WINDOWS)
@pytest.mark.parametrize("nw,nh", GRIDS)
def test_every_plane_and_the_record_match_the_definition(flow2d, ctx, nw, nh, m, order):
    u, v, state, su, sv = weighted_case(nw, nh, seed=m)
    field = WeightedField(ctx, u, v, state, su, sv)
    rejected = unweighable = 0
    for measure, s, min_state in ((SMALL, 8, 1), (GREEN, 3, 0)):
        for threshold, passes in ROBUST:
            # the zero sigmas are unweighable without a floor and weighable with one
            for floor in ((0.0, 0.002) if measure == SMALL else (0.002,)):
                outs, record = field.outputs(), poisoned_record(ctx)
                field.run(outs, record, s, m, order, measure, floor, threshold, passes, min_state)
                ref = field.reference(s, m, order, measure, floor, threshold, passes, min_state)
                what = "%dx%d m %d order %d measure %d floor %g T %g K %d" % (nw, nh, m, order, measure, floor, threshold, passes)
                field.check(outs, ref, what)
                check_record(record_of(ctx, record)[0], ref, what)
                words = weighted_words(ref)
                rejected += words[1]
                unweighable += words[3]
                assert threshold > 0 or words[:3] == [0, 0, 0], what
    # (the cases do what they are for: on the grid that holds the seams taps were rejected, and nodes were not weighable)
    assert (rejected > 0 and unweighable > 0) or nw < 70


def test_property_a_unit_sigmas_give_the_plain_entry_its_bytes(flow2d, ctx):
    """Both sigma planes 1.0f, floor 0, T = 0, against Context.node_strain on the device: the nine planes, and the record but for
    reserved[3 .. 6] (which are 0 here: nothing rejected, every usable node weighable -- so the whole record)."""
    nw, nh = 70, 9
    u, v, state = planted_case(nw, nh, seed=3)
    one = np.ones((nh, nw), F32)
    field = WeightedField(ctx, u, v, state, one, one)
    for m, order, measure in ((1, 1, SMALL), (2, 2, GREEN), (7, 2, SMALL), (7, 1, GREEN)):
        plain, plain_record = Field.outputs(field), poisoned_record(ctx)
        Field.run(field, plain, plain_record, 8, m, order, measure, grads=False)
        outs, record = field.outputs(), poisoned_record(ctx)
        field.run(outs, record, 8, m, order, measure, 0.0, 0.0, 0)
        for name in PLANES:
            assert outs[name].download().tobytes() == plain[name].download().tobytes(), (m, order, name)
        got, want = record_of(ctx, record).copy(), record_of(ctx, plain_record)
        assert (got["reserved"][0][3:7] == 0).all() and got.tobytes() == want.tobytes(), (m, order)
        valid = np.isfinite(plain["exx"].download(nw, nh))
        assert 0 < valid.sum() < nw * nh
        for name in SIGMAS:
            sg = outs[name].download(nw, nh)
            assert np.isfinite(sg[valid]).all() and (sg[valid] > 0).all() and np.isnan(sg[~valid]).all(), name


def test_property_b_doubled_sigmas_double_the_strain_sigmas(flow2d, ctx):
    """T = 0: both sigma planes and the floor times 2 change no byte of `out` or of the record and double every sigma plane
    exactly."""
    nw, nh = 70, 9
    u, v, state, su, sv = weighted_case(nw, nh, seed=4)
    once, twice = WeightedField(ctx, u, v, state, su, sv), WeightedField(ctx, u, v, state, 2 * su, 2 * sv)
    for m, order, measure, floor in ((1, 1, SMALL, 0.0), (2, 2, GREEN, 0.0078125), (7, 2, SMALL, 0.0), (7, 1, GREEN, 0.0078125)):
        a, ra = once.outputs(), poisoned_record(ctx)
        once.run(a, ra, 8, m, order, measure, floor, 0.0, 0)
        b, rb = twice.outputs(), poisoned_record(ctx)
        twice.run(b, rb, 8, m, order, measure, 2 * floor, 0.0, 0)
        for name in PLANES:
            assert a[name].download().tobytes() == b[name].download().tobytes(), (m, order, name)
        assert record_of(ctx, ra).tobytes() == record_of(ctx, rb).tobytes(), (m, order)
        for name in SIGMAS:
            x, y = a[name].download(nw, nh), b[name].download(nw, nh)
            assert np.isfinite(x).any() and np.array_equal(bits((2 * x).astype(F32)), bits(y)), (m, order, name)


def test_subsets_cost_no_other_plane(flow2d, ctx):
    """Each of the twenty-one planes alone and the record alone: the requested plane is the full run's, the others keep their
    poison, and the record is the same bytes whatever goes with it."""
    nw, nh, s, m = 70, 9, 8, 2
    u, v, state, su, sv = weighted_case(nw, nh, seed=5)
    field = WeightedField(ctx, u, v, state, su, sv)
    form = (s, m, 2, GREEN, 0.002, 3.0, 4)
    ref = field.reference(*form)
    full, full_record = field.outputs(), poisoned_record(ctx)
    field.run(full, full_record, *form)
    field.check(full, ref, "all planes")
    assert weighted_words(ref)[1] > 0
    want_record = record_of(ctx, full_record).tobytes()
    for names, with_record in [((name,), k % 2 == 0) for k, name in enumerate(ALL)] + [((), True), (SIGMAS, False)]:
        outs, record = field.outputs(), poisoned_record(ctx)
        field.run({name: outs[name] for name in names}, record if with_record else None, *form)
        field.check({name: outs[name] for name in names}, ref, "subset %s" % (names,))
        for name in ALL:
            if name not in names:
                assert (outs[name].download().view(U32) == POISON).all(), (names, name)
        assert record_of(ctx, record).tobytes() == (want_record if with_record else bytes([0x7F]) * 256), names
    # the convenience form: planes, diagnostics and sigmas by name, the record read back
    got, stats = ctx.node_strain_weighted(field.u, field.v, field.su, field.sv, nw, nh, s, m, 2, measure=GREEN, sigma_floor=0.002,
                                          threshold=3.0, iterations=4, state=field.state, planes=("e1",), diagnostics=("rejected",),
                                          sigmas=("sigma_exx", "sigma_exy"))
    assert set(got) == {"e1", "rejected", "sigma_exx", "sigma_exy"} and bytes(stats) == want_record
    for name in got:
        assert np.array_equal(bits(got[name]), bits(ref[name])), name
    counts = flow2d.node_strain_weighted_counts(stats)
    assert [counts[k] for k in ("touched", "rejected", "suspect", "unweighable")] == weighted_words(ref)
    assert flow2d.STRAIN_SIGMA_PLANES == SIGMAS
    assert flow2d.Context.node_strain_weighted_workspace_bytes(nw, nh) == 224 * 2 * 3


def test_repeated_calls_and_a_replayed_graph_give_the_same_bytes(flow2d, ctx):
    nw, nh, s, m = 70, 9, 8, 2
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    u, v, state, su, sv = weighted_case(nw, nh, seed=6)
    field = WeightedField(ctx, u, v, state, su, sv)
    form = (s, m, 2, GREEN, 0.002, 3.0, 4)
    outs = [(field.outputs(), poisoned_record(ctx)) for _ in range(3)]

    def snapshot(k):
        return [outs[k][0][name].download().tobytes() for name in ALL] + [record_of(ctx, outs[k][1]).tobytes()]

    field.run(*outs[0], *form)  # (also allocates the context's workspace)
    field.run(*outs[1], *form)
    eager = snapshot(0)
    assert snapshot(1) == eager
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    try:
        field.run(*outs[2], *form)
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
    field.check(outs[0][0], field.reference(*form), "70x9")


def test_lock_step_batch(flow2d, ctx):
    """Three instances a padded stride apart, the second all NaN: every plane and the record of instance b are the bytes of the
    same input analysed alone and the restatement's, and every other word of the output allocations is what it was."""
    nw, nh, cw, ch, count, s, m = 70, 9, 80, 12, 3, 8, 2
    stride = stride_of("rows", pitch_of(cw), ch)
    cases = [weighted_case(nw, nh, seed=20 + b) for b in range(count)]
    cases[1] = (np.full((nh, nw), np.nan, F32), np.full((nh, nw), np.nan, F32)) + cases[1][2:]
    fill = lambda arrays: Tall(ctx, cw, ch, count, stride).fill(arrays)  # noqa: E731
    tu, tv, ts, tsu, tsv = (fill([c[k] for c in cases]) for k in range(5))
    outs = {name: Tall(ctx, cw, ch, count, stride) for name in ALL}
    records = poisoned_record(ctx, count)
    form = dict(measure=GREEN, sigma_floor=0.002, threshold=3.0, iterations=4)
    pick = lambda held, names: {n: held[n] for n in names}  # noqa: E731
    with ctx.set_batch(count, stride):
        ctx.node_strain_weighted(tu, tv, tsu, tsv, nw, nh, s, m, 2, state=ts, planes=pick(outs, PLANES), diagnostics=pick(outs, DIAGNOSTICS),
                                 sigmas=pick(outs, SIGMAS), stats=records, instances=count, **form)
    ctx.synchronize()
    refs = [node_strain_weighted_reference(c[0], c[1], c[3], c[4], c[2], s, m, 2, measure=GREEN, floor=0.002, threshold=3.0, iterations=4)
            for c in cases]
    assert not refs[1]["valid"].any() and int(refs[1]["stats"]["reserved"][0][0]) == nw * nh
    for name in ALL:
        outs[name].check([r[name] for r in refs], name)
    got = record_of(ctx, records, count)
    for b, (c, ref) in enumerate(zip(cases, refs)):
        alone = {name: ctx.plane(cw, ch).fill_bytes(0x7F) for name in ALL}
        record = poisoned_record(ctx)
        ctx.node_strain_weighted(ctx.plane(cw, ch, c[0]), ctx.plane(cw, ch, c[1]), ctx.plane(cw, ch, c[3]), ctx.plane(cw, ch, c[4]), nw, nh,
                                 s, m, 2, state=ctx.plane(cw, ch, c[2]), planes=pick(alone, PLANES), diagnostics=pick(alone, DIAGNOSTICS),
                                 sigmas=pick(alone, SIGMAS), stats=record, **form)
        assert record_of(ctx, record).tobytes() == got[b:b + 1].tobytes(), "record of instance %d" % b
        for name in ALL:
            assert np.array_equal(alone[name].download(nw, nh).view(U32), bits(ref[name])), (b, name)
        check_record(got[b], ref, "instance %d" % b)
    for t in (tu, tv, ts, tsu, tsv):
        t.check(None, "an input")
    # a written range must not meet a later instance of an input or of another output, and one slice is no workspace for three
    lib = flow2d.hip_lib()
    need, ws = ctx._node_strain_weighted_workspace

    def call(planes, sig, record=records.ptr, ws_bytes=need):
        out, dg, sg = flow2d.DeformationPlanes(**planes), flow2d.NodeStrainDiagnostics(), flow2d.StrainSigmaPlanes(**sig)
        return lib.flow2d_node_strain_weighted_2d(ctx.handle, tu.ptr, tv.ptr, ts.ptr, tsu.ptr, tsv.ptr, nw, nh, tu.pitch, s, m, 2, 7, 1, GREEN,
                                                  0.002, 3.0, 4, ctypes.byref(out), ctypes.byref(dg), ctypes.byref(sg), record, ws.ptr,
                                                  ws_bytes)

    e1, sx = outs["e1"].ptr, outs["sigma_exx"].ptr
    with ctx.set_batch(count, stride):
        assert call({}, {"sigma_exx": tsv.ptr + 2 * stride}) == 1
        assert call({}, {"sigma_exx": tsu.ptr + stride}) == 1
        assert call({"e1": e1}, {"sigma_exy": e1 + stride}) == 1
        assert call({}, {"sigma_exx": sx, "sigma_eyy": sx + 2 * stride}) == 1
        assert call({}, {"sigma_exx": sx}, record=ws.ptr + need - 256) == 1
        assert call({}, {"sigma_exx": sx}, ws_bytes=lib.flow2d_node_strain_weighted_workspace_bytes(nw, nh, 1)) == 1
        assert call({"e1": e1}, {"sigma_exx": sx}) == 0
    ctx.synchronize()


def test_invalid_arguments_write_nothing(flow2d, ctx):
    nw, nh = 40, 30
    lib = flow2d.hip_lib()
    u, v, state, su, sv = weighted_case(nw, nh, seed=8)
    pu, pv, ps, psu, psv = (ctx.plane(nw, nh, a) for a in (u, v, state, su, sv))
    outs = {name: ctx.plane(nw, nh).fill_bytes(0x7F) for name in ALL}
    record = poisoned_record(ctx)
    need = lib.flow2d_node_strain_weighted_workspace_bytes(nw, nh, 1)
    assert need % 16 == 0 and need == lib.flow2d_node_strain_weighted_workspace_bytes(nw, nh, 2) // 2
    ws = ctx.plane(need // 4, 1).fill_bytes(0x7F)
    span = pu.pitch * nh
    d = dict(u=pu.ptr, v=pv.ptr, state=ps.ptr, su=psu.ptr, sv=psv.ptr, nw=nw, nh=nh, pitch=pu.pitch, s=8, m=2, order=1, min_nodes=4,
             min_state=1, measure=SMALL, floor=0.002, threshold=3.0, iterations=4, stats=record.ptr, ws=ws.ptr, ws_bytes=need,
             planes={name: outs[name].ptr for name in PLANES}, diag={name: outs[name].ptr for name in DIAGNOSTICS},
             sig={name: outs[name].ptr for name in SIGMAS}, out=True, diagnostics=True, sigmas=True)

    def call(**kw):
        a = dict(d, **kw)
        out, dg, sg = flow2d.DeformationPlanes(**a["planes"]), flow2d.NodeStrainDiagnostics(**a["diag"]), flow2d.StrainSigmaPlanes(**a["sig"])
        return lib.flow2d_node_strain_weighted_2d(ctx.handle, a["u"], a["v"], a["state"], a["su"], a["sv"], a["nw"], a["nh"], a["pitch"],
                                                  a["s"], a["m"], a["order"], a["min_nodes"], a["min_state"], a["measure"], a["floor"],
                                                  a["threshold"], a["iterations"], ctypes.byref(out) if a["out"] else None,
                                                  ctypes.byref(dg) if a["diagnostics"] else None, ctypes.byref(sg) if a["sigmas"] else None,
                                                  a["stats"], a["ws"], a["ws_bytes"])

    e1, sx = outs["e1"].ptr, outs["sigma_exx"].ptr
    nan, inf = float("nan"), float("inf")
    none = dict(planes={}, diag={}, sig={})
    bad = [dict(u=None), dict(v=None), dict(su=None), dict(sv=None), dict(su=psu.ptr + 4), dict(out=False, diagnostics=False, sigmas=False, stats=None),
           dict(none, stats=None), dict(nw=0), dict(nh=0), dict(pitch=pu.pitch + 8), dict(pitch=16), dict(s=0), dict(s=65), dict(m=0), dict(m=-1),
           dict(m=8), dict(order=0), dict(order=3), dict(min_nodes=2), dict(min_nodes=26), dict(order=2, min_nodes=5), dict(m=1, min_nodes=10),
           dict(min_state=-1), dict(min_state=2), dict(measure=2), dict(measure=-1), dict(floor=-0.002), dict(floor=nan), dict(floor=inf),
           dict(threshold=-3.0), dict(threshold=nan), dict(threshold=inf), dict(iterations=-1), dict(iterations=MAX_ITERATIONS + 1),
           dict(threshold=0.0, iterations=4), dict(state=ps.ptr + 4), dict(stats=record.ptr + 4), dict(ws=ws.ptr + 8), dict(ws=None),
           dict(ws_bytes=need - 1), dict(planes={"divergence": psu.ptr}), dict(diag={"residual": psv.ptr}),
           dict(sig={"sigma_ux": psu.ptr}), dict(sig={"sigma_uy": psv.ptr + pu.pitch}), dict(sig={"sigma_vx": pu.ptr}),
           dict(sig={"sigma_vy": ps.ptr}), dict(sig={"sigma_exx": e1}), dict(sig={"sigma_exx": sx, "sigma_eyy": sx}),
           dict(sig={"sigma_exx": sx, "sigma_exy": sx + span - pu.pitch}), dict(sig={"sigma_exx": sx + 4}), dict(stats=psu.ptr + 64),
           dict(stats=sx), dict(ws=psv.ptr), dict(ws=outs["sigma_vorticity"].ptr), dict(stats=ws.ptr + 16), dict(stats=ws.ptr + need - 8)]
    for kw in bad:
        assert call(**kw) == 1, kw
    assert call(nw=1 << 16, nh=1 << 15, pitch=4 << 16) == 5  # 2^31 nodes
    with ctx.set_batch(2, span):
        assert call() == 1  # a workspace for one instance under a batch of two
    ctx.synchronize()
    for name, q in outs.items():
        assert (q.download().view(U32) == POISON).all(), name
    assert set(record.download(64, 1).tobytes()) == {0x7F} and (ws.download().view(U32) == POISON).all()
    # without statistics the workspace takes no part, whatever it is; a sigma plane alone is output enough
    assert call(stats=None, ws=pv.ptr, ws_bytes=0, out=False, diagnostics=False, sig={"sigma_exy": outs["sigma_exy"].ptr}) == 0
    ctx.synchronize()
    assert set(record.download(64, 1).tobytes()) == {0x7F} and (ws.download().view(U32) == POISON).all()
    ref = node_strain_weighted_reference(u, v, su, sv, state, 8, 2, 1, 4, floor=0.002, threshold=3.0, iterations=4)
    assert np.array_equal(outs["sigma_exy"].download().view(U32), bits(ref["sigma_exy"]))
    assert call(iterations=MAX_ITERATIONS) == 0 and call(threshold=0.0, iterations=0) == 0 and call() == 0
    for name, q in outs.items():
        assert np.array_equal(q.download().view(U32), bits(ref[name])), name
    check_record(record_of(ctx, record)[0], ref, "after the refusals")
