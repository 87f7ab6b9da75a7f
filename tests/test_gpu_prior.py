"""The pyramid started from a prior flow, on the MI355X.

flow2d_prior_registration_2d against the numpy restatement (the sanitised prior through np_restatement.resample and registration),
against the device's own flow2d_resample_xy_pair + flow2d_registration_2d on a finite prior, per instance of a lock-step batch and
under graph replay; OpticalFlow.compute_flow_from_prior* against ComputeFlowDevice (a zero prior at the top level: the same bytes)
and against the oracle-stage restatement of tests/test_prior_cpu.py; the correlation-seeded chain against its three steps; the
refusals; the CLI."""
import ctypes
import json
import subprocess

import numpy as np
import pytest

from oracle import np_restatement as NP
from test_correlate_cpu import F32, U32, bits, grid, scenes_module
from test_prior_cpu import CLI_DEFAULTS, compute_flow_from_prior, correlation_prior, sanitise, start_level

pytestmark = pytest.mark.gpu
POISON = U32(0x7F7F7F7F)
GREY, GRADIENT, GRADIENT_UNTILED = 0, 1, 2
AUTO, FUSED = 0, 2


def special_prior(in_w, in_h, w, h, seed):
    """A prior with what the entry treats specially: scattered NaN (with a payload), +Inf and -Inf in u alone, in v alone and in
    both; every prior pixel under one output cell not finite; vectors that point out of any frame of this size; -0."""
    rng = np.random.default_rng(seed)
    u, v = (rng.normal(0, 3, (in_h, in_w)).astype(F32) for _ in range(2))
    u[in_h // 2, :] = 1000.0
    v[:, in_w // 3] = -1000.0
    u[0, 0], v[0, 0] = -0.0, -0.0
    for k in range(12):
        y, x = int(rng.integers(0, in_h)), int(rng.integers(0, in_w))
        value = (np.nan, np.inf, -np.inf)[k % 3]
        if k % 4 != 1:
            u[y, x] = value
        if k % 4 != 0:
            v[y, x] = value
    u.view(U32)[in_h - 1, in_w - 1] = 0x7FC12345
    v[in_h - 1, 0] = np.inf
    # output cell (ox, oy): its prior pixels are columns floor(ox * in_w / w) .. ceil((ox + 1) * in_w / w) - 1, rows alike
    ox, oy = (2 * w) // 3, h // 2
    x0, x1 = (ox * in_w) // w, -((-(ox + 1) * in_w) // w)
    y0, y1 = (oy * in_h) // h, -((-(oy + 1) * in_h) // h)
    u[y0:y1, x0:x1] = np.nan
    return u, v


def restatement(prior_u, prior_v, f0, f1, w, h):
    """(out_u, out_v, output, count) of flow2d_prior_registration_2d from the numpy restatement of the operators."""
    in_h, in_w = prior_u.shape
    su, sv, count = sanitise(prior_u, prior_v)
    u, v = NP.resample(su, w, h), NP.resample(sv, w, h)
    hx, hy = F32(in_w) / F32(w), F32(in_h) / F32(h)
    return u, v, NP.registration(f0, f1, u, v, hx, hy), count, hx, hy


def level_frames(w, h, seed):
    rng = np.random.default_rng(1000 + seed)
    return rng.uniform(0, 255, (h, w)).astype(F32), rng.uniform(0, 255, (h, w)).astype(F32)


def region_only(got, w, h):
    assert (got[h:] == POISON).all() and (got[:, w:] == POISON).all(), "written beyond the level"
    return got[:h, :w]


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
SHAPES = [((96, 80), (87, 72), None), ((96, 80), (48, 40), None), ((97, 61), (33, 21), None), ((96, 80), (13, 11), None),
          ((64, 4), (64, 4), None), ((70, 50), (70, 50), 256)]


@pytest.mark.parametrize("prior_size,level_size,container", SHAPES, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
def test_entry_equals_the_restatement(ctx, prior_size, level_size, container):
    (in_w, in_h), (w, h) = prior_size, level_size
    cw = container or in_w
    pu, pv = special_prior(in_w, in_h, w, h, in_w + w)
    f0, f1 = level_frames(w, h, w)
    want_u, want_v, want_out, count, hx, hy = restatement(pu, pv, f0, f1, w, h)
    assert count >= 6
    planes = [ctx.plane(cw, in_h + 2).fill_bytes(0x7F).upload(a) for a in (pu, pv, f0, f1)]
    outs = [ctx.plane(cw, in_h + 2).fill_bytes(0x7F) for _ in range(3)]
    got = ctx.prior_registration(planes[0], planes[1], in_w, in_h, outs[0], outs[1], planes[2], planes[3], w, h, float(hx), float(hy), outs[2])
    for q, want, name in zip(outs, (want_u, want_v, want_out), ("out_u", "out_v", "output")):
        same = region_only(bits(q.download()), w, h) == bits(want)
        assert same.all(), "%s differs at %d places, first (y, x) = %s" % (name, (~same).sum(), np.argwhere(~same)[0])
    assert got == count
    assert np.isfinite(want_u).all() and np.isfinite(want_v).all()  # (no NaN or infinity of the prior reaches the level)


@pytest.mark.parametrize("prior_size,level_size", [((96, 80), (87, 72)), ((96, 80), (48, 40)), ((130, 70), (33, 21)), ((70, 50), (70, 50))])
def test_finite_prior_equals_resample_and_registration_on_the_device(ctx, prior_size, level_size):
    (in_w, in_h), (w, h) = prior_size, level_size
    rng = np.random.default_rng(in_w * w)
    pu, pv = (rng.normal(0, 4, (in_h, in_w)).astype(F32) for _ in range(2))
    pu[3, :] = -500.0
    pv[0, 0] = -0.0
    f0, f1 = level_frames(w, h, 7)
    hx, hy = 1.37, float(F32(in_h) / F32(h))
    planes = [ctx.plane(in_w, in_h, a) for a in (pu, pv, f0, f1)]
    got = [ctx.plane(in_w, in_h).fill_bytes(0x7F) for _ in range(3)]
    want = [ctx.plane(in_w, in_h).fill_bytes(0x7F) for _ in range(3)]
    count = ctx.prior_registration(planes[0], planes[1], in_w, in_h, got[0], got[1], planes[2], planes[3], w, h, hx, hy, got[2])
    ctx.resample_xy(planes[0], want[0], in_w, in_h, w, h, planes[1], want[1])
    ctx.registration(planes[2], planes[3], want[0], want[1], w, h, hx, hy, want[2])
    ctx.synchronize()
    assert count == 0
    for a, b, name in zip(got, want, ("out_u", "out_v", "output")):
        assert np.array_equal(bits(a.download()), bits(b.download())), name


def test_batch_of_three_with_a_padded_stride(ctx):
    (in_w, in_h), (w, h), G, pad = (97, 61), (33, 21), 3, 5
    stride_rows = in_h + pad
    priors = [special_prior(in_w, in_h, w, h, 40 + b) for b in range(G)]
    for b in range(G):  # different counts per instance
        priors[b][0][5 + b, 0:3 + 4 * b] = np.nan
    frames = [level_frames(w, h, 50 + b) for b in range(G)]
    hx, hy = float(F32(in_w) / F32(w)), float(F32(in_h) / F32(h))

    def stack(arrays):
        full = np.full((stride_rows * G, in_w), POISON, U32)
        for b, a in enumerate(arrays):
            full[b * stride_rows:b * stride_rows + a.shape[0], :a.shape[1]] = bits(a)
        return ctx.plane(in_w, stride_rows * G).upload(full.view(F32))

    lone, counts = [], []
    for b in range(G):
        planes = [ctx.plane(in_w, in_h, a) for a in priors[b] + frames[b]]
        outs = [ctx.plane(in_w, in_h).fill_bytes(0x7F) for _ in range(3)]
        counts.append(ctx.prior_registration(planes[0], planes[1], in_w, in_h, outs[0], outs[1], planes[2], planes[3], w, h, hx, hy, outs[2]))
        lone.append([region_only(bits(q.download()), w, h) for q in outs])
    assert len(set(counts)) == G
    d = [stack([p[0] for p in priors]), stack([p[1] for p in priors]), stack([f[0] for f in frames]), stack([f[1] for f in frames])]
    outs = [stack([]) for _ in range(3)]
    record = ctx.prior_records(G).fill_bytes(0x7F)
    with ctx.set_batch(G, stride_rows * d[0].pitch):
        ctx.prior_registration(d[0], d[1], in_w, in_h, outs[0], outs[1], d[2], d[3], w, h, hx, hy, outs[2], record=record)
    ctx.synchronize()
    assert ctx.read_prior_records(record, G) == counts
    for k, q in enumerate(outs):
        got = bits(q.download())
        outside = np.ones(got.shape, bool)
        for b in range(G):
            r = b * stride_rows
            assert np.array_equal(got[r:r + h, :w], lone[b][k]), (k, b)
            outside[r:r + h, :w] = False
        assert (got[outside] == POISON).all(), "words outside the instances' regions were written"


def test_two_replays_of_a_captured_launch(flow2d, ctx):
    (in_w, in_h), (w, h) = (96, 80), (48, 40)
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    pu, pv = special_prior(in_w, in_h, w, h, 77)
    f0, f1 = level_frames(w, h, 78)
    planes = [ctx.plane(in_w, in_h, a) for a in (pu, pv, f0, f1)]
    outs = [ctx.plane(in_w, in_h).fill_bytes(0x7F) for _ in range(3)]
    record = ctx.prior_records().fill_bytes(0x7F)
    args = (planes[0], planes[1], in_w, in_h, outs[0], outs[1], planes[2], planes[3], w, h, 2.0, 2.0, outs[2])
    count = ctx.prior_registration(*args)
    eager = [bits(q.download()) for q in outs]
    for q in outs:
        q.fill_bytes(0x7F)
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    try:
        ctx.prior_registration(*args, record=record)
    finally:
        graph = vp()
        assert lib.flow2d_capture_end(ctx.handle, ctypes.byref(graph)) == 0
    try:
        ctx.synchronize()
        assert (bits(outs[2].download()) == POISON).all()  # captured, not run
        for _ in range(2):
            for q in outs:
                q.fill_bytes(0x3C)
            assert lib.flow2d_graph_launch(ctx.handle, graph) == 0
            ctx.synchronize()
            for q, want in zip(outs, eager):
                got = bits(q.download())
                assert np.array_equal(got[:h, :w], want[:h, :w])
            assert ctx.read_prior_records(record) == [count]  # zeroed and counted again: not doubled
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)


# ---- the host layer ---------------------------------------------------------------------------------------------------------------
SHORT = (3, 5, 35.0, 0.001, 0.001, 5, 1.5)  # outer, inner, alpha, e_smooth, e_data, median, sigma


@pytest.mark.parametrize("constancy", [GREY, GRADIENT], ids=["grey", "gradient"])
@pytest.mark.parametrize("scale", [0.9, 0.5])
def test_zero_prior_at_the_top_level_gives_compute_flow_devices_bytes(flow2d, ctx, oracle, scale, constancy):
    w, h = 96, 80
    f0, f1 = oracle.synthetic_pair(w, h, 1.5, -0.75, seed=4, noise=True)
    top = min(50, flow2d.max_warp_level(w, h, scale)) - 1
    p = flow2d.OpticalFlow.params(50, scale, *SHORT)
    flow = flow2d.OpticalFlow(w, h, constancy, ctx=ctx)
    try:
        d = [ctx.plane(w, h, a) for a in (f0, f1, np.zeros_like(f0), np.zeros_like(f0))]
        want, got = [ctx.plane(w, h) for _ in range(2)], [ctx.plane(w, h) for _ in range(2)]
        for graph, rounds in ((False, 1), (True, 2)):
            flow.use_graph(graph)
            for rnd in range(rounds):
                for q in want + got:
                    q.fill_bytes(0x55)
                flow.compute_flow_device(d[0].ptr, d[1].ptr, want[0].ptr, want[1].ptr, p)
                report = flow.compute_flow_from_prior_device(d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, got[0].ptr, got[1].ptr, p, level=top)
                ctx.synchronize()
                assert (report.start_level, report.levels_run, report.not_finite) == (top, top + 1, 0)
                for a, b in zip(got, want):
                    assert np.array_equal(bits(a.download()), bits(b.download())), (graph, rnd)
        assert not (bits(got[0].download()) == 0x55555555).all()
    finally:
        flow.close()


@pytest.fixture(scope="module")
def speckle_pair():
    sc = scenes_module().make_speckle_scene("large_translation", 96, 80, seed=0)
    return sc, correlation_prior(sc.frame_0, sc.frame_1, 7, 12, 8)


@pytest.mark.parametrize("scale,reach", [(0.9, 2.0), (0.5, 4.0)])
@pytest.mark.parametrize("constancy", [GREY, GRADIENT_UNTILED], ids=["grey", "gradient_untiled"])
def test_correlation_prior_equals_the_oracle_stage_restatement(flow2d, ctx, oracle, speckle_pair, scale, reach, constancy):
    sc, (pu, pv, (nu, nv, score, record, lo_scale)) = speckle_pair
    w, h = 96, 80
    start = start_level(w, h, 50, scale, reach)
    assert start == {0.9: 7, 0.5: 2}[scale]
    want_u, want_v, count = compute_flow_from_prior(oracle, sc.frame_0, sc.frame_1, pu, pv, 50, scale, *SHORT, constancy, start)
    flow = flow2d.OpticalFlow(w, h, constancy, ctx=ctx)
    try:
        out = flow.compute_flow_correlation_seeded(sc.frame_0, sc.frame_1, flow2d.OpticalFlow.params(50, scale, *SHORT), radius=7,
                                                   search=12, spacing=8, reach=reach)
    finally:
        flow.close()
    assert np.array_equal(bits(out["prior"][0]), bits(pu)) and np.array_equal(bits(out["prior"][1]), bits(pv))
    assert np.array_equal(bits(out["nodes"][0]), bits(nu)) and np.array_equal(bits(out["nodes"][1]), bits(nv))
    assert bytes(out["record"]) == record.tobytes()
    assert out["report"].summary() == dict(start_level=start, levels_run=start + 1, not_finite=count)
    assert np.array_equal(bits(out["u"]), bits(want_u)) and np.array_equal(bits(out["v"]), bits(want_v))


def test_a_strip_solved_level_below_the_start_level(flow2d, ctx, oracle):
    """Scale 0.5, reach 2: the prior enters at level 1, and level 0 -- exactly twice it -- keeps its base flow at level 1's size when
    the strips solve it.  The smallest such frame (even sizes, 4 : 3) by the solver's own answer."""
    pick = flow2d.hip_lib().flow2d_solver_algorithm_for
    pitch = flow2d.hip_lib().flow2d_plane_pitch_bytes
    outer, inner = 2, 3
    w = h = 0
    for n in range(64, 2048, 8):
        w, h = n, (n * 3 // 4 + 1) // 2 * 2
        if pick(AUTO, w, h, pitch(w), outer, inner, GREY) == FUSED:
            break
    assert pick(AUTO, w, h, pitch(w), outer, inner, GREY) == FUSED and pick(AUTO, w - 8, ((w - 8) * 3 // 4 + 1) // 2 * 2, pitch(w - 8), outer,
                                                                          inner, GREY) != FUSED
    f0, f1 = oracle.synthetic_pair(w, h, 2.5, -1.25, seed=6, noise=True)
    rng = np.random.default_rng(6)
    pu = (2.5 + rng.normal(0, 0.3, (h, w))).astype(F32)
    pv = (-1.25 + rng.normal(0, 0.3, (h, w))).astype(F32)
    pu[10:14, 20:40], pv[h - 1, w - 1] = np.nan, np.inf
    args = (2, 0.5, outer, inner, 35.0, 0.001, 0.001, 5, 1.5)
    assert start_level(w, h, 2, 0.5, 2.0) == 1
    want_u, want_v, count = compute_flow_from_prior(oracle, f0, f1, pu, pv, *args, GREY, 1)
    flow = flow2d.OpticalFlow(w, h, GREY, ctx=ctx)
    try:
        d = [ctx.plane(w, h, a) for a in (f0, f1, pu, pv)] + [ctx.plane(w, h), ctx.plane(w, h)]
        before = flow2d.half_base_flow_launches()
        report = flow.compute_flow_from_prior_device(*[q.ptr for q in d], flow2d.OpticalFlow.params(*args))
        assert flow2d.half_base_flow_launches() == before + 1
        assert (report.start_level, report.levels_run, report.not_finite) == (1, 2, count) and count == 81
        assert np.array_equal(bits(d[4].download()), bits(want_u)) and np.array_equal(bits(d[5].download()), bits(want_v))
    finally:
        flow.close()


def flat_patch_pair():
    """A speckle pair whose frame 0 has a textureless patch: the nodes inside it are invalid and the expansion is NaN there."""
    sc = scenes_module().make_speckle_scene("translation", 96, 80, seed=1)
    f0, f1 = sc.frame_0.copy(), sc.frame_1.copy()
    f0[8:72, 8:64] = 100.0
    return f0, f1


def test_chain_equals_its_three_steps_and_reports_the_count(flow2d, ctx):
    w, h, r, d, s = 96, 80, 7, 6, 8
    f0, f1 = flat_patch_pair()
    p = flow2d.OpticalFlow.params(50, 0.9, *SHORT)
    flow = flow2d.OpticalFlow(w, h, GRADIENT, ctx=ctx)
    try:
        frames = [ctx.plane(w, h, f0), ctx.plane(w, h, f1)]
        by_hand = [ctx.plane(w, h).fill_bytes(0x7F) for _ in range(6)]  # node u, node v, prior u, prior v, u, v
        chain = [ctx.plane(w, h).fill_bytes(0x7F) for _ in range(6)]
        rec = flow.correlate_device(frames[0].ptr, frames[1].ptr, 0.0, 1.0, r, d, s, dev_nodes=(by_hand[0].ptr, by_hand[1].ptr),
                                    dev_flow=(by_hand[2].ptr, by_hand[3].ptr))
        report = flow.compute_flow_from_prior_device(frames[0].ptr, frames[1].ptr, by_hand[2].ptr, by_hand[3].ptr, by_hand[4].ptr,
                                                     by_hand[5].ptr, p)
        got_report, got_rec = flow.compute_flow_correlation_seeded_device(
            frames[0].ptr, frames[1].ptr, chain[4].ptr, chain[5].ptr, p, 0.0, 1.0, r, d, s, dev_nodes=(chain[0].ptr, chain[1].ptr),
            dev_prior=(chain[2].ptr, chain[3].ptr))
        ctx.synchronize()
        nw, nh = grid(w, h, r, s)
        for k, (a, b) in enumerate(zip(chain, by_hand)):
            size = (nw, nh) if k < 2 else (w, h)
            assert np.array_equal(bits(a.download(*size)), bits(b.download(*size))), k
        assert bytes(got_rec) == bytes(rec) and rec.invalid > 0
        assert got_report.summary() == report.summary()
        prior = by_hand[2].download(), by_hand[3].download()
        not_finite = int((~(np.isfinite(prior[0]) & np.isfinite(prior[1]))).sum())
        assert not_finite > 0 and report.not_finite == not_finite and report.start_level == 7
        assert np.isfinite(by_hand[4].download()).all()
    finally:
        flow.close()


def test_another_prior_plane_records_a_second_graph(flow2d, ctx, oracle):
    w, h = 96, 80
    f0, f1 = oracle.synthetic_pair(w, h, 1.5, -0.75, seed=8, noise=True)
    rng = np.random.default_rng(8)
    priors = [[(c + rng.normal(0, 0.2, (h, w))).astype(F32) for c in (1.5, -0.75)] for _ in range(2)]
    priors[1][0][3, 4:9] = np.nan
    p = flow2d.OpticalFlow.params(50, 0.5, *SHORT)
    flow = flow2d.OpticalFlow(w, h, GREY, ctx=ctx)
    try:
        frames = [ctx.plane(w, h, f0), ctx.plane(w, h, f1)]
        dev = [[ctx.plane(w, h, a) for a in pair] for pair in priors]
        out = [ctx.plane(w, h), ctx.plane(w, h)]

        def run(k):
            for q in out:
                q.fill_bytes(0x55)
            report = flow.compute_flow_from_prior_device(frames[0].ptr, frames[1].ptr, dev[k][0].ptr, dev[k][1].ptr, out[0].ptr, out[1].ptr, p)
            return bits(out[0].download()), bits(out[1].download()), report.not_finite

        eager = [run(0), run(1)]
        assert (eager[0][2], eager[1][2]) == (0, 5) and not np.array_equal(eager[0][0], eager[1][0])
        flow.use_graph(True)
        for k in (0, 1, 0, 1):  # record, record, replay, replay
            u, v, count = run(k)
            assert np.array_equal(u, eager[k][0]) and np.array_equal(v, eager[k][1]) and count == eager[k][2], k
    finally:
        flow.close()


def test_refusals(flow2d, ctx, oracle):
    w, h = 96, 80
    f0, f1 = oracle.synthetic_pair(w, h, 1.5, -0.75, seed=9, noise=True)
    p = flow2d.OpticalFlow.params(50, 0.9, *SHORT)
    flow = flow2d.OpticalFlow(w, h, GREY, ctx=ctx)
    try:
        d = [ctx.plane(w, h, a) for a in (f0, f1, np.zeros_like(f0), np.zeros_like(f0))] + [ctx.plane(w, h), ctx.plane(w, h)]
        ptr = [q.ptr for q in d]
        flow.compute_flow_from_prior_device(*ptr, p)  # (accepted as it stands)
        for bad in ((ptr[0], ptr[1], ptr[4], ptr[3], ptr[4], ptr[5]),   # prior u is flow u
                    (ptr[0], ptr[1], ptr[2], ptr[5], ptr[4], ptr[5]),   # prior v is flow v
                    (ptr[0], ptr[1], ptr[2], ptr[4] + d[4].pitch, ptr[4], ptr[5]),  # prior v starts inside flow u
                    (ptr[0], ptr[1], None, ptr[3], ptr[4], ptr[5])):
            with pytest.raises(flow2d.Flow2DError):
                flow.compute_flow_from_prior_device(*bad, p)
        for kw in (dict(reach=0.0), dict(reach=float("nan")), dict(reach=float("inf")), dict(reach=-2.0)):
            with pytest.raises(flow2d.Flow2DError):
                flow.compute_flow_from_prior_device(*ptr, p, **kw)
        with pytest.raises(ValueError):
            flow.compute_flow_from_prior_device(*ptr, p, level=-1)
        with pytest.raises(ValueError):  # a prior of another size
            flow.compute_flow_from_prior(f0, f1, np.zeros((h, w + 1), F32), np.zeros((h, w + 1), F32), p)
        assert flow.bidirectional_refuses_prior(p)
        u, v, _ = flow.compute_flow_bidirectional(f0, f1, p)[:3]  # (without the keys it runs)
        assert np.isfinite(u).all()
    finally:
        flow.close()
    grouped = flow2d.OpticalFlow(w, h, GREY, ctx=ctx, group_size=2)
    try:
        tall = [ctx.plane(w, 2 * h, np.zeros((2 * h, w), F32)) for _ in range(6)]
        with pytest.raises(flow2d.Flow2DError):
            grouped.compute_flow_from_prior_device(*[q.ptr for q in tall], p)
        with pytest.raises(flow2d.Flow2DError):
            grouped.compute_flow_correlation_seeded_device(tall[0].ptr, tall[1].ptr, tall[4].ptr, tall[5].ptr, p, 0.0, 1.0)
    finally:
        grouped.close()


def test_cli(flow2d, ctx, tmp_path):
    """--initial-flow and --correlation-prior write the bytes of the Python path and print one "Prior:" line; a run without them
    prints none; the excluded combinations and bad values are usage errors; a prior of another size is refused."""
    w, h = 96, 80
    sc = scenes_module().make_speckle_scene("large_translation", w, h, seed=0)
    names = [str(tmp_path / "f0.raw"), str(tmp_path / "f1.raw")]
    sc.frame_0.tofile(names[0])
    sc.frame_1.tofile(names[1])
    pu, pv = sc.gt_u.copy(), sc.gt_v.copy()
    pu[5, 6:9] = np.nan
    prior_file, small_file = str(tmp_path / "prior.flo"), str(tmp_path / "small.flo")
    flow2d.write_flo(prior_file, pu, pv)
    flow2d.write_flo(small_file, pu[:, :-1], pv[:, :-1])

    def run(options, out):
        out.mkdir()
        q = subprocess.run([flow2d.CLI_PATH] + options + names + [str(w), str(h), "t_", str(out) + "/"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=300)
        return q, {f.name: f.read_bytes() for f in out.iterdir()}

    def prior_line(q):
        lines = [x for x in q.stdout.splitlines() if x.startswith("Prior: ")]
        assert len(lines) == 1, q.stdout[-2000:]
        return json.loads(lines[0][len("Prior: "):])

    p = flow2d.OpticalFlow.params(*CLI_DEFAULTS)
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        u, v, report, _ = flow.compute_flow_from_prior(sc.frame_0, sc.frame_1, pu, pv, p, reach=4.0)
        seeded = flow.compute_flow_correlation_seeded(sc.frame_0, sc.frame_1, p, radius=7, search=12, spacing=8)
        leveled = flow.compute_flow_from_prior(sc.frame_0, sc.frame_1, pu, pv, p, level=3)
    finally:
        flow.close()
    q, files = run(["--initial-flow", prior_file, "--prior-reach", "4"], tmp_path / "initial")
    assert q.returncode == 0, q.stdout[-2000:]
    assert files["t_flow-u-96-80.raw"] == u.tobytes() and files["t_flow-v-96-80.raw"] == v.tobytes()
    assert prior_line(q) == dict(source="initial-flow", reach=4.0, start_level=14, levels_run=15, not_finite=3)
    assert report.summary() == dict(start_level=14, levels_run=15, not_finite=3)
    q, files = run(["--initial-flow", prior_file, "--prior-level", "3"], tmp_path / "level")
    assert q.returncode == 0 and files["t_flow-u-96-80.raw"] == leveled[0].tobytes() and prior_line(q)["start_level"] == 3
    q, files = run(["--correlation-prior", "7", "--correlation-range", "12"], tmp_path / "seeded")
    assert q.returncode == 0, q.stdout[-2000:]
    assert files["t_flow-u-96-80.raw"] == seeded["u"].tobytes() and files["t_flow-v-96-80.raw"] == seeded["v"].tobytes()
    nw, nh = grid(w, h, 7, 8)
    assert prior_line(q) == dict(seeded["record"].summary(), **seeded["report"].summary(), source="correlation", reach=2.0, radius=7,
                                 range=12, spacing=8, min_score=-1.0, lo=seeded["lo_scale"][0], scale=seeded["lo_scale"][1], nw=nw, nh=nh)
    assert seeded["report"].start_level == 7 and not [f for f in files if "node" in f]
    plain, plain_files = run([], tmp_path / "plain")
    assert plain.returncode == 0 and "Prior: " not in plain.stdout
    assert plain_files["t_flow-u-96-80.raw"] != files["t_flow-u-96-80.raw"]
    q, _ = run(["--initial-flow", small_file], tmp_path / "small")
    assert q.returncode == 2, q.stdout[-500:]
    for bad in (["--initial-flow", prior_file, "--correlation-prior", "7"], ["--initial-flow", prior_file, "--correlation", "7"],
                ["--correlation-prior", "7", "--correlation", "7"], ["--initial-flow", prior_file, "--backward"],
                ["--correlation-prior", "7", "--backward"], ["--correlation-prior", "0"], ["--correlation-prior", "16"],
                ["--correlation-prior"], ["--initial-flow", prior_file, "--prior-reach", "0"],
                ["--initial-flow", prior_file, "--prior-reach", "nan"], ["--initial-flow", prior_file, "--prior-level", "-1"],
                ["--prior-reach", "2"], ["--prior-level", "1"], ["--correlation-prior", "7", "--refine", "3"]):
        q = subprocess.run([flow2d.CLI_PATH] + bad + names + [str(w), str(h), "t_"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert q.returncode == 5, (bad, q.stdout[-500:])
