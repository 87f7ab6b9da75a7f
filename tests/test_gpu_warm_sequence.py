"""Sequences warm-started from the previous pair's flow, on the MI355X: ComputeFlowSequenceWarmDevice is its parts -- pair 0
ComputeFlowDevice, every later pair ComputeFlowFromPriorDevice from Context.propagate_flow of the delivered flow before it --, with
and without reports and through the host-image forms; the adaptive mode over a scene cut, where pyramid levels above the last start
level have to be built late; ComputeFlowSequenceDevice unchanged beside it; the CLI's --previous-flow; the refusals."""
import json
import subprocess

import numpy as np
import pytest

from test_propagate_cpu import F32, bits, scenes_module

pytestmark = pytest.mark.gpu
W, H, N = 96, 80, 5
GREY, GRADIENT = 0, 1
UNSEEDED, SEEDED, REDONE = 0, 1, 2
MEDIUM = (10, 5, 35.0, 0.001, 0.001, 5, 1.5)  # outer, inner, alpha, e_smooth, e_data, median, sigma
CLI_DEFAULTS = (50, 0.9, 40, 5, 35.0, 0.001, 0.001, 5, 1.5)
FILL, PHOTO = 4, 1.0


@pytest.fixture(scope="module")
def two_layer():
    return scenes_module().make_sequence("two_layer", N, W, H, seed=0)


def device_frames(ctx, frames):
    return [ctx.plane(W, H, f) for f in frames]


def flow_planes(ctx, count):
    return [ctx.plane(W, H).fill_bytes(0x55) for _ in range(count)], [ctx.plane(W, H).fill_bytes(0x55) for _ in range(count)]


def ptrs(planes):
    return [q.ptr for q in planes]


def downloaded(us, vs):
    return [(bits(u.download()), bits(v.download())) for u, v in zip(us, vs)]


def from_parts(flow2d, ctx, flow, frames, p, k, prev, reach=2.0, level=None):
    """Pair k >= 1 from its parts: Context.propagate_flow of the delivered flow k - 1 (Planes `prev`), then ComputeFlowFromPriorDevice.
    Returns ((u bits, v bits), PropagateRecord, PriorReport)."""
    prior = [ctx.plane(W, H).fill_bytes(0x55) for _ in range(2)]
    out = [ctx.plane(W, H).fill_bytes(0x55) for _ in range(2)]
    _, _, rec = ctx.propagate_flow(prev[0], prev[1], W, H, frame_from=frames[k - 1], frame_to=frames[k], photo_scale=PHOTO, fill_passes=FILL,
                                   out_u=prior[0], out_v=prior[1])
    report = flow.compute_flow_from_prior_device(frames[k].ptr, frames[k + 1].ptr, prior[0].ptr, prior[1].ptr, out[0].ptr, out[1].ptr, p,
                                                 reach=reach, level=level)
    return (bits(out[0].download()), bits(out[1].download())), rec, report


def plain_pair(ctx, flow, frames, p, k):
    out = [ctx.plane(W, H).fill_bytes(0x55) for _ in range(2)]
    flow.compute_flow_device(frames[k].ptr, frames[k + 1].ptr, out[0].ptr, out[1].ptr, p)
    ctx.synchronize()
    return bits(out[0].download()), bits(out[1].download())


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- the composition identity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("constancy,scale,reach", [(GREY, 0.5, 2.0), (GRADIENT, 0.5, 2.0), (GREY, 0.5, 4.0), (GRADIENT, 0.5, 4.0),
                                                   (GREY, 0.9, 2.0)])
def test_warm_sequence_is_its_parts(flow2d, ctx, two_layer, constancy, scale, reach):
    p = flow2d.OpticalFlow.params(50, scale, *MEDIUM)
    start = flow2d.prior_start_level(W, H, 50, scale, reach)
    assert start == {(0.5, 2.0): 1, (0.5, 4.0): 2, (0.9, 2.0): 7}[(scale, reach)]
    flow = flow2d.OpticalFlow(W, H, constancy, ctx=ctx)
    try:
        frames = device_frames(ctx, two_layer.frames)
        us, vs = flow_planes(ctx, N - 1)
        assert flow.compute_flow_sequence_warm_device(ptrs(frames), ptrs(us), ptrs(vs), p, reach=reach, fill_passes=FILL,
                                                      photo_scale=PHOTO) is None
        ctx.synchronize()
        warm = downloaded(us, vs)
        assert same(warm[0], plain_pair(ctx, flow, frames, p, 0)), "pair 0 is ComputeFlowDevice's"
        parts = {}
        for k in range(1, N - 1):
            parts[k] = from_parts(flow2d, ctx, flow, frames, p, k, (us[k - 1], vs[k - 1]), reach)
            assert same(warm[k], parts[k][0]), "pair %d is not ComputeFlowFromPriorDevice from the propagated flow %d" % (k, k - 1)
            assert not same(warm[k], plain_pair(ctx, flow, frames, p, k))  # (the prior does something at these settings)
        # with reports: the same flows, and what the parts report
        us2, vs2 = flow_planes(ctx, N - 1)
        reports = flow.compute_flow_sequence_warm_device(ptrs(frames), ptrs(us2), ptrs(vs2), p, reach=reach, fill_passes=FILL,
                                                         photo_scale=PHOTO, reports=True)
        ctx.synchronize()
        for k, pair in enumerate(downloaded(us2, vs2)):
            assert same(pair, warm[k]), k
        assert reports[0].mode == UNSEEDED and reports[0].propagation.pixels == 0 and list(reports[0].share) == [-1.0] * 3
        for k in range(1, N - 1):
            r, (_, rec, prior_report) = reports[k], parts[k]
            assert (r.mode, r.reach, r.start_level, r.levels_run, r.not_finite) == (SEEDED, 0, start, start + 1, prior_report.not_finite), k
            assert bytes(r.propagation) == bytes(rec) and rec.pixels == W * H and rec.landed > 0, k
            assert list(r.share) == [-1.0] * 3
    finally:
        flow.close()


def test_host_forms_and_one_pair_from_the_previous(flow2d, ctx, two_layer):
    p = flow2d.OpticalFlow.params(50, 0.5, *MEDIUM)
    flow = flow2d.OpticalFlow(W, H, GREY, ctx=ctx)
    try:
        frames = device_frames(ctx, two_layer.frames)
        us, vs = flow_planes(ctx, N - 1)
        flow.compute_flow_sequence_warm_device(ptrs(frames), ptrs(us), ptrs(vs), p)
        ctx.synchronize()
        warm = downloaded(us, vs)
        host_us, host_vs, reports, _ = flow.compute_flow_sequence_warm(two_layer.frames, p)
        for k in range(N - 1):
            assert same((bits(host_us[k]), bits(host_vs[k])), warm[k]), k
        assert [r.mode for r in reports] == [UNSEEDED] + [SEEDED] * (N - 2)
        # one pair from the previous pair's flow: the device form and the host-image form, with the earlier frame
        k = 2
        out = [ctx.plane(W, H).fill_bytes(0x55) for _ in range(2)]
        report = flow.compute_flow_from_previous_device(frames[k].ptr, frames[k + 1].ptr, us[k - 1].ptr, vs[k - 1].ptr, out[0].ptr, out[1].ptr,
                                                        p, dev_prev_frame=frames[k - 1].ptr)
        assert same((bits(out[0].download()), bits(out[1].download())), warm[k])
        assert report.mode == SEEDED and bytes(report.propagation) == bytes(reports[k].propagation) and report.start_level == 1
        u, v, host_report, _ = flow.compute_flow_from_previous(two_layer.frames[k], two_layer.frames[k + 1], host_us[k - 1], host_vs[k - 1], p,
                                                               prev_frame=two_layer.frames[k - 1])
        assert same((bits(u), bits(v)), warm[k]) and host_report.summary() == report.summary()
        # without the earlier frame there is no photometric term, and a mask keeps vectors from being carried
        _, _, rec = ctx.propagate_flow(us[k - 1], vs[k - 1], W, H, fill_passes=FILL)
        plain = flow.compute_flow_from_previous_device(frames[k].ptr, frames[k + 1].ptr, us[k - 1].ptr, vs[k - 1].ptr, out[0].ptr, out[1].ptr, p)
        assert bytes(plain.propagation) == bytes(rec)
        mask = np.zeros((H, W), F32)
        mask[10:20, 30:50] = 1
        masked = flow.compute_flow_from_previous(two_layer.frames[k], two_layer.frames[k + 1], host_us[k - 1], host_vs[k - 1], p, prev_mask=mask)[2]
        assert masked.propagation.unusable == 200
        # PropagateFlowDevice: the object's own workspace and record, the entry's bytes
        got, want = [ctx.plane(W, H).fill_bytes(0x55) for _ in range(2)], [ctx.plane(W, H).fill_bytes(0x55) for _ in range(2)]
        rec_a = flow.propagate_flow_device(us[0].ptr, vs[0].ptr, got[0].ptr, got[1].ptr, dev_frame_from=frames[0].ptr, dev_frame_to=frames[1].ptr,
                                           step=-1.0, photo_scale=0.5, fill_passes=2)
        _, _, rec_b = ctx.propagate_flow(us[0], vs[0], W, H, frame_from=frames[0], frame_to=frames[1], step=-1.0, photo_scale=0.5,
                                         fill_passes=2, out_u=want[0], out_v=want[1])
        assert bytes(rec_a) == bytes(rec_b) and same(downloaded(got[:1], got[1:])[0], downloaded(want[:1], want[1:])[0])
    finally:
        flow.close()


# ---- the adaptive mode over a scene cut ------------------------------------------------------------------------------------------------
def test_adaptive_run_over_a_scene_cut(flow2d, ctx, two_layer):
    """two_layer with an unrelated frame (a speckle pattern) spliced in as frame 3, the CLI's parameters (scale 0.9, 33 levels), gradient
    constancy, a tail of half a per cent.  Pair 1 is seeded at reach 2 (level 7) and holds; pair 2 runs INTO the cut and pair 3 out of
    it: both must end as ComputeFlowDevice's flow, reported as redone or unseeded.  The redone pair needs every level of the frames
    2 and 3 above the level its seeded run started at: they are built then, late.
    (The rule sees a cut only through how far the seeded solve moves away from its prior, and a solve that enters at a fine level
    cannot move far: on this sequence 2.2 % of the pixels move more than a pixel at the cut, none before it -- hence the strict tail.)"""
    frames_host = two_layer.frames.copy()
    frames_host[3] = scenes_module().make_speckle_scene("translation", W, H, seed=3).frame_0
    p = flow2d.OpticalFlow.params(*CLI_DEFAULTS)
    tail = 0.005
    flow = flow2d.OpticalFlow(W, H, GRADIENT, ctx=ctx)
    try:
        frames = device_frames(ctx, frames_host)
        us, vs = flow_planes(ctx, N - 1)
        reports = flow.compute_flow_sequence_warm_device(ptrs(frames), ptrs(us), ptrs(vs), p, reach=2.0, fill_passes=FILL,
                                                         photo_scale=PHOTO, tail=tail, reports=True)
        got = downloaded(us, vs)
        for k, r in enumerate(reports):
            print("pair %d: %s" % (k, r.summary()))
        assert reports[0].mode == UNSEEDED and same(got[0], plain_pair(ctx, flow, frames, p, 0))
        assert (reports[1].mode, reports[1].reach, reports[1].start_level) == (SEEDED, 2, 7)
        assert reports[1].share[1] <= tail
        assert same(got[1], from_parts(flow2d, ctx, flow, frames, p, 1, (us[0], vs[0]), 2.0)[0])
        for k in (2, 3):
            assert reports[k].mode in (UNSEEDED, REDONE), "pair %d at the cut was kept as seeded: %s" % (k, reports[k].summary())
            assert same(got[k], plain_pair(ctx, flow, frames, p, k)), k
            assert reports[k].propagation.pixels == W * H and reports[k].share[2] > tail  # a prediction was made and did not hold
        assert REDONE in (reports[2].mode, reports[3].mode)
        # without reports the adaptive run gives the same flows
        us2, vs2 = flow_planes(ctx, N - 1)
        assert flow.compute_flow_sequence_warm_device(ptrs(frames), ptrs(us2), ptrs(vs2), p, reach=2.0, tail=tail) is None
        ctx.synchronize()
        for k, pair in enumerate(downloaded(us2, vs2)):
            assert same(pair, got[k]), k
    finally:
        flow.close()


# ---- the neighbours -------------------------------------------------------------------------------------------------------------------
def test_plain_sequence_after_a_warm_one_is_unchanged(flow2d, ctx, two_layer):
    p = flow2d.OpticalFlow.params(50, 0.5, *MEDIUM)
    fresh = flow2d.OpticalFlow(W, H, GREY, ctx=ctx)
    try:
        frames = device_frames(ctx, two_layer.frames)
        us, vs = flow_planes(ctx, N - 1)
        fresh.compute_flow_sequence_device(ptrs(frames), ptrs(us), ptrs(vs), p)
        ctx.synchronize()
        want = downloaded(us, vs)
        for k in range(N - 1):
            assert same(want[k], plain_pair(ctx, fresh, frames, p, k)), k
    finally:
        fresh.close()
    flow = flow2d.OpticalFlow(W, H, GREY, ctx=ctx)
    try:
        frames = device_frames(ctx, two_layer.frames)
        us, vs = flow_planes(ctx, N - 1)
        flow.compute_flow_sequence_warm_device(ptrs(frames), ptrs(us), ptrs(vs), p, reach=4.0)  # leaves pyramids of three levels behind
        ctx.synchronize()
        warm = downloaded(us, vs)
        for q in us + vs:
            q.fill_bytes(0x55)
        flow.compute_flow_sequence_device(ptrs(frames), ptrs(us), ptrs(vs), p)
        ctx.synchronize()
        for k, pair in enumerate(downloaded(us, vs)):
            assert same(pair, want[k]), k
        assert not same(warm[2], want[2])
        bu, bv = flow_planes(ctx, N - 1)
        flow.compute_flow_bidirectional_device(ptrs(frames), ptrs(us), ptrs(vs), ptrs(bu), ptrs(bv), p)
        ctx.synchronize()
        for k, pair in enumerate(downloaded(us, vs)):
            assert same(pair, want[k]), k
    finally:
        flow.close()


# ---- the CLI and the refusals ---------------------------------------------------------------------------------------------------------
def test_cli_chain_over_three_frames(flow2d, ctx, two_layer, tmp_path):
    names = [str(tmp_path / ("f%d.raw" % k)) for k in range(3)]
    for k, name in enumerate(names):
        two_layer.frames[k].tofile(name)

    def run(options, pair, out):
        out.mkdir()
        q = subprocess.run([flow2d.CLI_PATH] + options + pair + [str(W), str(H), "t_", str(out) + "/"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=300)
        return q, {f.name: f.read_bytes() for f in out.iterdir()}

    def line(q, head):
        lines = [x for x in q.stdout.splitlines() if x.startswith(head)]
        assert len(lines) == 1, q.stdout[-2000:]
        return json.loads(lines[0][len(head):])

    p = flow2d.OpticalFlow.params(*CLI_DEFAULTS)
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        us, vs, reports, _ = flow.compute_flow_sequence_warm(two_layer.frames[:3], p, reach=2.0)
        u_plain, v_plain, report_plain, _ = flow.compute_flow_from_previous(two_layer.frames[1], two_layer.frames[2], us[0], vs[0], p, fill_passes=2)
    finally:
        flow.close()
    first, files = run(["--flo"], names[0:2], tmp_path / "first")
    assert first.returncode == 0 and "Propagation: " not in first.stdout and "Prior: " not in first.stdout
    assert files["t_flow-u-96-80.raw"] == us[0].tobytes()
    flo = str(tmp_path / "first" / "t_flow.flo")
    q, files = run(["--previous-flow", flo, "--previous-frame", names[0]], names[1:3], tmp_path / "second")
    assert q.returncode == 0, q.stdout[-2000:]
    assert files["t_flow-u-96-80.raw"] == us[1].tobytes() and files["t_flow-v-96-80.raw"] == vs[1].tobytes()
    assert line(q, "Propagation: ") == dict(reports[1].propagation.summary(), fill=4, photometric=True)
    assert line(q, "Prior: ") == dict(source="previous-flow", reach=2.0, start_level=7, levels_run=8, not_finite=reports[1].not_finite)
    q, files = run(["--previous-flow", flo, "--propagate-fill", "2"], names[1:3], tmp_path / "plain")
    assert q.returncode == 0 and files["t_flow-u-96-80.raw"] == u_plain.tobytes() and files["t_flow-v-96-80.raw"] == v_plain.tobytes()
    assert line(q, "Propagation: ") == dict(report_plain.propagation.summary(), fill=2, photometric=False)
    q, files = run(["--previous-flow", flo, "--prior-level", "3"], names[1:3], tmp_path / "level")
    assert q.returncode == 0 and line(q, "Prior: ")["start_level"] == 3
    for bad in (["--previous-flow", flo, "--initial-flow", flo], ["--previous-flow", flo, "--correlation-prior", "7"],
                ["--previous-flow", flo, "--correlation", "7"], ["--previous-flow", flo, "--backward"], ["--previous-flow", flo, "--refine", "3"],
                ["--previous-frame", names[0]], ["--propagate-fill", "2"], ["--previous-flow", flo, "--propagate-fill", "65"],
                ["--previous-flow", flo, "--propagate-fill", "-1"], ["--previous-flow", flo, "--propagate-fill"]):
        q = subprocess.run([flow2d.CLI_PATH] + bad + names[1:3] + [str(W), str(H), "t_"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert q.returncode == 5, (bad, q.stdout[-500:])
    small = str(tmp_path / "small.flo")
    flow2d.write_flo(small, us[0][:, :-1], vs[0][:, :-1])
    q, _ = run(["--previous-flow", small], names[1:3], tmp_path / "small")
    assert q.returncode == 2, q.stdout[-500:]


def test_refusals(flow2d, ctx, two_layer):
    p = flow2d.OpticalFlow.params(50, 0.9, *MEDIUM)
    flow = flow2d.OpticalFlow(W, H, GREY, ctx=ctx)
    try:
        frames = device_frames(ctx, two_layer.frames[:3])
        us, vs = flow_planes(ctx, 2)
        f, u, v = ptrs(frames), ptrs(us), ptrs(vs)
        flow.compute_flow_sequence_warm_device(f, u, v, p, reach=3.0, tail=0.05)  # (accepted as it stands)
        for kw in (dict(reach=3.5, tail=0.05), dict(reach=4.0, tail=0.0), dict(level=2, tail=0.05), dict(reach=0.0), dict(reach=float("nan"))):
            with pytest.raises(flow2d.Flow2DError):
                flow.compute_flow_sequence_warm_device(f, u, v, p, **kw)
        for kw in (dict(tail=1.0), dict(tail=-0.5), dict(fill_passes=65), dict(photo_scale=-1.0), dict(level=-1)):
            with pytest.raises(ValueError):
                flow.compute_flow_sequence_warm_device(f, u, v, p, **kw)
        with pytest.raises(ValueError):
            flow.compute_flow_sequence_warm_device(f, u[:1], v, p)
        for bad in ((f, [u[0], u[0]], v), (f, [f[0], u[1]], v), (f, u, [u[0], v[1]]), (f, [None, u[1]], v)):  # written twice, a frame, null
            with pytest.raises(flow2d.Flow2DError):
                flow.compute_flow_sequence_warm_device(*bad, p)
        # one frame without the other
        with pytest.raises(flow2d.Flow2DError):
            flow.propagate_flow_device(u[0], v[0], u[1], v[1], dev_frame_from=f[0])
        with pytest.raises(flow2d.Flow2DError):
            flow.propagate_flow_device(u[0], v[0], u[1], v[1], dev_frame_to=f[1])
        with pytest.raises(flow2d.Flow2DError):
            flow.propagate_flow_device(u[0], v[0], u[1], v[1], step=0.0)
        with pytest.raises(flow2d.Flow2DError):  # the output is the input
            flow.propagate_flow_device(u[0], v[0], u[0], v[1])
        with pytest.raises(flow2d.Flow2DError):
            ctx.propagate_flow(us[0], vs[0], W, H, frame_from=frames[0], out_u=us[1], out_v=vs[1])
        with pytest.raises(flow2d.Flow2DError):
            flow.compute_flow_from_previous_device(f[1], f[2], u[0], None, u[1], v[1], p)
        with pytest.raises(ValueError):
            flow.compute_flow_sequence_warm(two_layer.frames[:1], p)
    finally:
        flow.close()
    grouped = flow2d.OpticalFlow(W, H, GREY, ctx=ctx, group_size=2)
    try:
        tall = [ctx.plane(W, 2 * H, np.zeros((2 * H, W), F32)) for _ in range(7)]
        t = ptrs(tall)
        with pytest.raises(flow2d.Flow2DError):
            grouped.compute_flow_sequence_warm_device(t[:3], t[3:5], t[5:7], p)
        with pytest.raises(flow2d.Flow2DError):
            grouped.compute_flow_from_previous_device(t[0], t[1], t[2], t[3], t[4], t[5], p)
        with pytest.raises(flow2d.Flow2DError):
            grouped.propagate_flow_device(t[2], t[3], t[4], t[5])
    finally:
        grouped.close()
