"""The layers above flow2d_compose_nodes_2d on the device: OpticalFlow.correlate_subset_sequence* with reference_every against the
chain spelled out by hand from the Context entries and compose_nodes, byte for byte, records included; reference_every = 0 against
the call without the keyword; the rotation to 36 degrees, where a moving reference finds every judged node and the fixed one none;
B-spline interpolation and order 2 through a reference change; the refusals; the CLI's --subset-base with and without
--subset-previous against the sequence call's steps."""
import json
import subprocess

import numpy as np
import pytest

from test_correlate_cpu import F32, U32, frame_range, grid
from test_gpu_multipass import POISON
from test_subset_cpu import Refined
from test_subset_reference_cpu import ROTATION, rotation_scenes
from test_subset_sequence_cpu import judge

pytestmark = pytest.mark.gpu
W, H, R = ROTATION["width"], ROTATION["height"], ROTATION["R"]
PASSES = ((7, 6, 8),)  # the search after every reference change: 4 degrees move a node by 3.7 pixels at most
FILES = dict(zip(Refined.NAMES, ("node-u", "node-v", "node-ux", "node-uy", "node-vx", "node-vy", "node-score", "node-state")))


def frames_of_the_rotation(steps):
    scenes = rotation_scenes()[:steps]
    return scenes, [scenes[0].frame_0] + [sc.frame_1 for sc in scenes]


def refilled(ctx, field, nw, nh, s, new):
    """Two prediction passes over a dict of planes by hand: (the seven planes u, v, ux, uy, vx, vy, state, the passes' records)."""
    names = ("u", "v", "ux", "uy", "vx", "vy")
    ping, pong = [new() for _ in range(7)], [new() for _ in range(7)]
    precs = [ctx.predict_records().fill_bytes(0x7F) for _ in range(2)]
    ctx.predict_nodes([field[n] for n in names], field["state"], nw, nh, s, 1, 1, ping[:6], ping[6], precs[0])
    ctx.predict_nodes(ping[:6], ping[6], nw, nh, s, 1, 1, pong[:6], pong[6], precs[1])
    ctx.synchronize()
    return pong, [q.download(16, 1).tobytes() for q in precs]


def test_a_moving_reference_equals_the_chain_by_hand(flow2d, ctx):
    """Five frames, a new reference every 2 steps: steps 1 and 2 against frame 0, step 3 the pair chain from frame 2, step 4 from
    step 3's increment; both composed with the refilled field of step 2."""
    steps_n = 4
    _, frames = frames_of_the_rotation(steps_n)
    lo, scale = frame_range(frames[0], frames[1])
    names = flow2d.OpticalFlow.SUBSET_PLANES
    six = names[:6]
    r, _, s = PASSES[-1]
    nw, nh = grid(W, H, r, s)
    dev = [ctx.plane(W, H, f) for f in frames]
    new = lambda: ctx.plane(W, H).fill_bytes(0x7F)  # noqa: E731
    ptrs = lambda planes: {n: q.ptr for n, q in planes.items()}  # noqa: E731
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        out = [{name: new() for name in names} for _ in range(steps_n)]
        fu, fv = new(), new()
        reports, steps = flow.correlate_subset_sequence_device([q.ptr for q in dev], lo, scale, PASSES, R, [ptrs(step) for step in out],
                                                               dev_flows=[None, None, None, (fu.ptr, fv.ptr)], reference_every=2)
        records = flow.compose_records
        assert len(steps) == steps_n and len(records) == steps_n
        assert not any(bytes(records[k]).strip(b"\0") for k in (0, 1)) and all(records[k].nodes == nw * nh for k in (2, 3))
        # by hand: steps 1 and 2 as they always were
        hand = [{name: new() for name in names} for _ in range(steps_n)]
        _, rec1 = flow.correlate_subset_device(dev[0].ptr, dev[1].ptr, lo, scale, PASSES, R, dev_out=ptrs(hand[0]))
        assert bytes(rec1) == bytes(steps[0].subset)
        start, precs = refilled(ctx, hand[0], nw, nh, s, new)
        record = ctx.subset_records().fill_bytes(0x7F)
        h = hand[1]
        ctx.subset_refine_from(dev[0], dev[2], W, H, start[0], start[1], start[2:6], nw, nh, r, s, R, max_shift=4.0, out_u=h["u"], out_v=h["v"],
                               out_gradients=[h[n] for n in names[2:6]], out_score=h["score"], out_state=h["state"], record=record)
        ctx.synchronize()
        assert bytes(steps[1].subset) == record.download(16, 1).tobytes()
        assert [bytes(steps[1].prediction[p]) for p in range(2)] == precs
        # step 3: the base from step 2, the pair chain from frame 2
        base, base_records = refilled(ctx, hand[1], nw, nh, s, new)
        assert [bytes(steps[2].prediction[p]) for p in range(2)] == base_records
        inc3 = {name: new() for name in names}
        _, rec3 = flow.correlate_subset_device(dev[2].ptr, dev[3].ptr, lo, scale, PASSES, R, dev_out=ptrs(inc3))
        assert bytes(rec3) == bytes(steps[2].subset)
        # step 4: from step 3's increment, against frame 2
        start, precs = refilled(ctx, inc3, nw, nh, s, new)
        inc4 = {name: new() for name in names}
        ctx.subset_refine_from(dev[2], dev[4], W, H, start[0], start[1], start[2:6], nw, nh, r, s, R, max_shift=4.0, out_u=inc4["u"],
                               out_v=inc4["v"], out_gradients=[inc4[n] for n in names[2:6]], out_score=inc4["score"], out_state=inc4["state"],
                               record=record)
        ctx.synchronize()
        assert bytes(steps[3].subset) == record.download(16, 1).tobytes()
        assert [bytes(steps[3].prediction[p]) for p in range(2)] == precs
        for k, inc in ((2, inc3), (3, inc4)):
            h = hand[k]
            crec = ctx.compose_records().fill_bytes(0x7F)
            ctx.compose_nodes(base, [inc[n] for n in six] + [inc["state"]], nw, nh, r, s, 1, inc["score"], [h[n] for n in six], h["state"],
                              h["score"], crec)
            ctx.synchronize()
            assert bytes(records[k]) == crec.download(16, 1).tobytes(), "composition record of step %d" % (k + 1)
            print("step %d:" % (k + 1), json.dumps(records[k].summary()))
            assert records[k].composed >= 60
        for k in range(steps_n):
            for name in names:
                got = out[k][name].download().view(U32)
                assert np.array_equal(got[:nh, :nw], hand[k][name].download(nw, nh).view(U32)), (k, name)
                assert (got[nh:] == POISON).all() and (got[:, nw:] == POISON).all(), (k, name)
        assert set(np.unique(out[3]["state"].download(nw, nh))) == {-1.0, float(flow2d.SUBSET_STATE_COMPOSED)}
        du, dv = new(), new()
        ctx.expand_nodes(hand[3]["u"], hand[3]["v"], nw, nh, r, s, du, dv, W, H)
        ctx.synchronize()
        assert fu.download().tobytes() == du.download().tobytes() and fv.download().tobytes() == dv.download().tobytes()
        # compose_nodes_device is the same composition; without a record it only queues
        again = {name: new() for name in names}
        base_ptrs = dict(zip(flow.COMPOSE_BASE, [q.ptr for q in base]))
        rec = flow.compose_nodes_device(base_ptrs, ptrs(inc4), r, s, ptrs(again))
        assert bytes(rec) == bytes(records[3])
        for name in names:
            assert again[name].download().tobytes() == out[3][name].download().tobytes(), name
        bare = {name: new() for name in six}
        assert flow.compose_nodes_device(base_ptrs, ptrs(inc4), r, s, ptrs(bare), record=False) is None
        ctx.synchronize()
        assert bare["vy"].download().tobytes() == out[3]["vy"].download().tobytes()
        for bad in (dict(base=dict(base_ptrs, state=None)), dict(inc=dict(ptrs(inc4), ux=None)), dict(out=dict(ptrs(bare), score=again["score"].ptr),
                    inc={n: q for n, q in ptrs(inc4).items() if n != "score"}), dict(min_state=2)):
            with pytest.raises(flow2d.Flow2DError):
                flow.compose_nodes_device(bad.get("base", base_ptrs), bad.get("inc", ptrs(inc4)), r, s, bad.get("out", ptrs(again)),
                                          min_state=bad.get("min_state", 1))
        # the host-image form, and its own composition
        nodes, _, psteps, _ = flow.correlate_subset_sequence(frames, PASSES, R, reference_every=2)
        assert [bytes(q) for q in psteps] == [bytes(q) for q in steps] and [bytes(q) for q in flow.compose_records] == [bytes(q) for q in records]
        for k in range(steps_n):
            for name in names:
                assert nodes[k][name].tobytes() == out[k][name].download(nw, nh).tobytes(), (k, name)
        base_arrays = dict(zip(flow.COMPOSE_BASE, [q.download(nw, nh) for q in base]))
        composed, rec = flow.compose_nodes(base_arrays, {n: q.download(nw, nh) for n, q in inc4.items()}, r, s)
        assert bytes(rec) == bytes(records[3]) and all(composed[n].tobytes() == nodes[3][n].tobytes() for n in names)
        # refusals: a negative value, a mask, curvature planes
        ok = [ptrs(step) for step in out]
        frames_ptr = [q.ptr for q in dev]
        with pytest.raises(flow2d.Flow2DError):
            flow.correlate_subset_sequence_device(frames_ptr, lo, scale, PASSES, R, ok, reference_every=-1)
        mask = ctx.plane(W, H, np.zeros((H, W), F32))
        with pytest.raises(flow2d.Flow2DError):
            flow.correlate_subset_sequence_device(frames_ptr, lo, scale, PASSES, R, ok, reference_every=2, mask=mask.ptr)
        with pytest.raises(flow2d.Flow2DError):
            flow.correlate_subset_sequence(frames, PASSES, R, reference_every=2, mask=np.zeros((H, W), F32))
        flow.correlate_subset_sequence_device(frames_ptr, lo, scale, PASSES, R, ok, mask=mask.ptr)  # ... which the fixed reference takes
        # order 2 runs through a reference change without curvature planes, and is refused with them
        curved = [dict(step, **{n: new().ptr for n in flow.SUBSET2_PLANES[8:]}) for step in ok]
        with pytest.raises(flow2d.Flow2DError):
            flow.correlate_subset_sequence_device(frames_ptr, lo, scale, PASSES, R, curved, reference_every=2, order=2)
        flow.correlate_subset_sequence_device(frames_ptr, lo, scale, PASSES, R, curved, order=2)
        _, second = flow.correlate_subset_sequence_device(frames_ptr, lo, scale, PASSES, R, ok, reference_every=2, order=2)
        assert flow.compose_records[3].composed >= 60 and second[3].subset.converged >= 60
    finally:
        flow.close()
    grouped = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx, group_size=2)
    try:
        tall = [ctx.plane(W, 2 * H, np.zeros((2 * H, W), F32)) for _ in range(23)]
        with pytest.raises(flow2d.Flow2DError):
            grouped.compose_nodes_device(dict(zip(flow2d.OpticalFlow.COMPOSE_BASE, [q.ptr for q in tall[:7]])),
                                         dict(zip(names, [q.ptr for q in tall[7:15]])), r, s, dict(zip(names, [q.ptr for q in tall[15:23]])))
    finally:
        grouped.close()


def test_reference_every_0_is_the_call_without_the_keyword(flow2d, ctx):
    _, frames = frames_of_the_rotation(3)
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        moved = flow.correlate_subset_sequence(frames, PASSES, R, reference_every=1)  # (an earlier call's value does not stick)
        plain = flow.correlate_subset_sequence(frames, PASSES, R, flow=True)
        assert not any(bytes(q).strip(b"\0") for q in flow.compose_records)
        zero = flow.correlate_subset_sequence(frames, PASSES, R, flow=True, reference_every=0)
        assert not any(bytes(q).strip(b"\0") for q in flow.compose_records)
        # every step against the frame before it
        again = flow.correlate_subset_sequence(frames, PASSES, R, reference_every=1)
        assert [q.nodes for q in flow.compose_records] == [0, 99, 99]
    finally:
        flow.close()
    for k in range(3):
        for name in plain[0][k]:
            assert plain[0][k][name].tobytes() == zero[0][k][name].tobytes(), (k, name)
            assert moved[0][k][name].tobytes() == again[0][k][name].tobytes(), (k, name)
        assert bytes(plain[2][k]) == bytes(zero[2][k])
        assert plain[4][k][0].tobytes() == zero[4][k][0].tobytes() and plain[4][k][1].tobytes() == zero[4][k][1].tobytes()
    assert moved[0][1]["u"].tobytes() != plain[0][1]["u"].tobytes()


def as_refined(nodes):
    got = Refined()
    for name in Refined.NAMES:
        setattr(got, name, nodes[name])
    return got


def test_a_moving_reference_follows_36_degrees_the_fixed_one_does_not(flow2d, ctx):
    """Nine steps of 4 degrees.  With a new reference every 3 steps the last step finds every judged node; against frame 0 none."""
    scenes, frames = frames_of_the_rotation(9)
    r, _, s = PASSES[-1]
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        moving = flow.correlate_subset_sequence(frames, PASSES, R, reference_every=3)[0]
        records = flow.compose_records
        fixed = flow.correlate_subset_sequence(frames, PASSES, R)[0]
    finally:
        flow.close()
    row = judge(scenes[8], as_refined(moving[8]), r, s, R)
    print("36 degrees, a new reference every 3 steps:", json.dumps(row), json.dumps(records[8].summary()))
    assert row["judged"] >= 50 and row["good"] == row["judged"] and row["wrong"] == 0
    lost = judge(scenes[8], as_refined(fixed[8]), r, s, R)
    print("36 degrees, the fixed reference:", json.dumps(lost))
    assert lost["good"] == 0


def test_bspline_interpolation_goes_through_a_reference_change(flow2d, ctx):
    """Four frames, a new reference every 2 steps, frame k sampled through its B-spline coefficients: step 3 is the composition of
    step 2's refilled field with the B-spline pair chain of (frame 2, frame 3)."""
    _, frames = frames_of_the_rotation(3)
    r, _, s = PASSES[-1]
    nw, nh = grid(W, H, r, s)
    new = lambda: ctx.plane(W, H).fill_bytes(0x7F)  # noqa: E731
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        nodes = flow.correlate_subset_sequence(frames, PASSES, R, reference_every=2, interpolation="bspline")[0]
        record = flow.compose_records[2]
        other = flow.correlate_subset_sequence(frames, PASSES, R, reference_every=2)[0]
        inc = flow.correlate_subset(frames[2], frames[3], PASSES, R, interpolation="bspline")[0]
        field = {n: ctx.plane(W, H, np.pad(nodes[1][n], ((0, H - nh), (0, W - nw)))) for n in flow.COMPOSE_BASE}
        base, _ = refilled(ctx, field, nw, nh, s, new)
        composed, rec = flow.compose_nodes(dict(zip(flow.COMPOSE_BASE, [q.download(nw, nh) for q in base])), inc, r, s)
    finally:
        flow.close()
    assert bytes(rec) == bytes(record) and record.composed >= 60
    for name in composed:
        assert composed[name].tobytes() == nodes[2][name].tobytes(), name
    assert nodes[2]["u"].tobytes() != other[2]["u"].tobytes()


def test_cli_subset_base(flow2d, ctx, tmp_path):
    """Frame by frame through the command line with a moved reference: the base files are step 2's refilled field; the run on
    (frame 2, frame 3) with --subset-base writes step 3 of the sequence call and its increment, the run on (frame 2, frame 4) with
    --subset-previous (that increment) and --subset-base writes step 4."""
    _, frames = frames_of_the_rotation(4)
    r, _, s = PASSES[-1]
    nw, nh = grid(W, H, r, s)
    paths = []
    for k, f in enumerate(frames):
        paths.append(str(tmp_path / ("f%d.raw" % k)))
        f.tofile(paths[-1])
    grid_options = ["--correlation", "7", "--correlation-range", "6", "--subset-refine", str(R)]
    new = lambda: ctx.plane(W, H).fill_bytes(0x7F)  # noqa: E731

    def run(options, pair, out):
        out.mkdir()
        q = subprocess.run([flow2d.CLI_PATH, "--flo"] + options + [paths[pair[0]], paths[pair[1]], str(W), str(H), "t_", str(out) + "/"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        return q, {f.name: f.read_bytes() for f in out.iterdir()}

    def printed(q, what):
        line = [x for x in q.stdout.splitlines() if x.startswith(what + ": ")]
        assert len(line) == 1, q.stdout[-2000:]
        return json.loads(line[0][len(what) + 2:])

    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        nodes = flow.correlate_subset_sequence(frames, PASSES, R, reference_every=2)[0]
        records = flow.compose_records
        inc3 = flow.correlate_subset(frames[2], frames[3], PASSES, R)[0]
        field = {n: ctx.plane(W, H, np.pad(nodes[1][n], ((0, H - nh), (0, W - nw)))) for n in flow.COMPOSE_BASE}
        base, _ = refilled(ctx, field, nw, nh, s, new)
        base = dict(zip(flow.COMPOSE_BASE, [q.download(nw, nh) for q in base]))
        by_python, _ = flow.compose_nodes(base, inc3, r, s)
    finally:
        flow.close()
    (tmp_path / "base").mkdir()
    prefix = str(tmp_path / "base") + "/t_"
    for name, plane in base.items():
        plane.tofile("%s%s-%d-%d.raw" % (prefix, FILES[name], nw, nh))
    q3, files3 = run(grid_options + ["--subset-base", prefix], (2, 3), tmp_path / "step3")
    assert q3.returncode == 0, q3.stdout[-2000:]
    for name in Refined.NAMES:
        assert files3["t_%s-%d-%d.raw" % (FILES[name], nw, nh)] == nodes[2][name].tobytes() == by_python[name].tobytes(), name
        assert files3["t_increment-%s-%d-%d.raw" % (FILES[name], nw, nh)] == inc3[name].tobytes(), name
    line = printed(q3, "Compose")
    assert {k: line[k] for k in records[2].summary()} == records[2].summary() and line["min_state"] == 1
    q4, files4 = run(grid_options + ["--subset-previous", str(tmp_path / "step3") + "/t_increment-", "--subset-base", prefix, "--subset-strain", "0"],
                     (2, 4), tmp_path / "step4")
    assert q4.returncode == 0, q4.stdout[-2000:]
    for name in Refined.NAMES:
        assert files4["t_%s-%d-%d.raw" % (FILES[name], nw, nh)] == nodes[3][name].tobytes(), name
    line = printed(q4, "Compose")
    assert {k: line[k] for k in records[3].summary()} == records[3].summary()
    # the strain is the composed field's: its valid nodes are the composed ones
    assert printed(q4, "NodeStrain")["valid"] == records[3].composed
    # base files of another grid are a bad input; the option alone is a usage error
    q5, _ = run(["--correlation", "7", "--correlation-range", "6", "--correlation-spacing", "7", "--subset-refine", str(R), "--subset-base", prefix],
                (2, 3), tmp_path / "other_grid")
    assert q5.returncode == 2, q5.stdout[-2000:]
    q = subprocess.run([flow2d.CLI_PATH, "--subset-base", "x_"] + paths[:2] + [str(W), str(H), "t_"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=60)
    assert q.returncode == 5, q.stdout[-500:]
