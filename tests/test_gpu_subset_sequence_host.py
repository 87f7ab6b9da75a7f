"""The layers above flow2d_subset_refine_from_2d and flow2d_predict_nodes_2d on the device: three steps of the rotation sequence
through OpticalFlow.correlate_subset_sequence_device against the chain spelled out by hand -- correlate_subset_device, then per
step Context.predict_nodes twice and Context.subset_refine_from -- byte for byte, records included; refine_nodes_from_device; the
host-image form; the refusals and lock-step groups; the CLI's --subset-previous (files, the "Prediction:" and "Subset:" lines, a
grid that does not match)."""
import json
import subprocess

import numpy as np
import pytest

from test_correlate_cpu import F32, U32, frame_range, grid
from test_gpu_multipass import POISON, report_bytes
from test_subset_cpu import Refined
from test_subset_sequence_cpu import ROTATION, judge, rotation_scenes

pytestmark = pytest.mark.gpu
W, H, R = ROTATION["width"], ROTATION["height"], ROTATION["R"]
PASSES = ((7, 6, 8),)  # the search of step 1: 4 degrees move a node by 3.7 pixels at most
STEPS = 3
FILES = dict(zip(Refined.NAMES, ("node-u", "node-v", "node-ux", "node-uy", "node-vx", "node-vy", "node-score", "node-state")))


def frames_of_the_rotation():
    scenes = rotation_scenes()[:STEPS]
    return scenes, [scenes[0].frame_0] + [sc.frame_1 for sc in scenes]


def test_sequence_equals_the_chain_by_hand(flow2d, ctx):
    scenes, frames = frames_of_the_rotation()
    lo, scale = frame_range(frames[0], frames[1])
    names = flow2d.OpticalFlow.SUBSET_PLANES
    r, _, s = PASSES[-1]
    nw, nh = grid(W, H, r, s)
    dev = [ctx.plane(W, H, f) for f in frames]
    new = lambda: ctx.plane(W, H).fill_bytes(0x7F)  # noqa: E731
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        out = [{name: new() for name in names} for _ in range(STEPS)]
        fu, fv = new(), new()
        reports, steps = flow.correlate_subset_sequence_device([q.ptr for q in dev], lo, scale, PASSES, R,
                                                               [{n: q.ptr for n, q in step.items()} for step in out],
                                                               dev_flows=[None, None, (fu.ptr, fv.ptr)])
        assert len(reports) == 1 and len(steps) == STEPS
        # by hand
        hand = [{name: new() for name in names} for _ in range(STEPS)]
        first, rec1 = flow.correlate_subset_device(dev[0].ptr, dev[1].ptr, lo, scale, PASSES, R, dev_out={n: q.ptr for n, q in hand[0].items()})
        assert report_bytes(first) == report_bytes(reports) and bytes(rec1) == bytes(steps[0].subset)
        assert not any(bytes(steps[0].prediction[k]).strip(b"\0") for k in range(flow2d.SEQUENCE_MAX_FILL))
        for k in range(1, STEPS):
            last = hand[k - 1]
            ping, pong = [new() for _ in range(7)], [new() for _ in range(7)]
            precs = [ctx.predict_records().fill_bytes(0x7F) for _ in range(2)]
            ctx.predict_nodes([last[n] for n in names[:6]], last["state"], nw, nh, s, 1, 1, ping[:6], ping[6], precs[0])
            ctx.predict_nodes(ping[:6], ping[6], nw, nh, s, 1, 1, pong[:6], pong[6], precs[1])
            record = ctx.subset_records().fill_bytes(0x7F)
            h = hand[k]
            ctx.subset_refine_from(dev[0], dev[k + 1], W, H, pong[0], pong[1], pong[2:6], nw, nh, r, s, R, max_shift=4.0, out_u=h["u"],
                                   out_v=h["v"], out_gradients=[h[n] for n in names[2:6]], out_score=h["score"], out_state=h["state"],
                                   record=record)
            ctx.synchronize()
            assert bytes(steps[k].subset) == record.download(16, 1).tobytes(), "record of step %d" % (k + 1)
            for p in range(2):
                assert bytes(steps[k].prediction[p]) == precs[p].download(16, 1).tobytes(), "prediction %d of step %d" % (p, k + 1)
            assert not any(bytes(steps[k].prediction[p]).strip(b"\0") for p in range(2, flow2d.SEQUENCE_MAX_FILL))
            print("step %d:" % (k + 1), json.dumps(steps[k].summary(2)))
        for k in range(STEPS):
            for name in names:
                got = out[k][name].download().view(U32)
                assert np.array_equal(got[:nh, :nw], hand[k][name].download(nw, nh).view(U32)), (k, name)
                assert (got[nh:] == POISON).all() and (got[:, nw:] == POISON).all(), (k, name)
        du, dv = new(), new()
        ctx.expand_nodes(hand[2]["u"], hand[2]["v"], nw, nh, r, s, du, dv, W, H)
        ctx.synchronize()
        assert fu.download().tobytes() == du.download().tobytes() and fv.download().tobytes() == dv.download().tobytes()
        # what the chain is for: at 12 degrees the judged nodes are found
        got = Refined()
        for name in names:
            setattr(got, name, out[2][name].download(nw, nh))
        row = judge(scenes[2], got, r, s, R)
        print("12 degrees:", json.dumps(row))
        assert row["good"] >= 0.95 * row["judged"] and row["wrong"] == 0
        # refine_nodes_from_device: step 3 again from step 2's planes through one prediction
        again = {name: new() for name in names}
        start = [new() for _ in range(7)]
        ctx.predict_nodes([out[1][n] for n in names[:6]], out[1]["state"], nw, nh, s, 1, 1, start[:6], start[6], None)
        rec = flow.refine_nodes_from_device(dev[0].ptr, dev[3].ptr, {n: q.ptr for n, q in zip(names[:6], start)}, r, s, R,
                                            dev_out={n: q.ptr for n, q in again.items()})
        assert rec.nodes == nw * nh and rec.converged >= 60
        with pytest.raises(ValueError):
            flow.refine_nodes_from_device(dev[0].ptr, dev[3].ptr, {"u": start[0].ptr, "v": start[1].ptr}, r, s, R)
        # the host-image form
        nodes, preports, psteps, (plo, pscale), flows = flow.correlate_subset_sequence(frames, PASSES, R, flow=True)
        assert (F32(plo), F32(pscale)) == (lo, scale) and report_bytes(preports) == report_bytes(reports)
        assert [bytes(q) for q in psteps] == [bytes(q) for q in steps]
        for k in range(STEPS):
            for name in names:
                assert nodes[k][name].tobytes() == out[k][name].download(nw, nh).tobytes(), (k, name)
        assert flows[2][0].tobytes() == fu.download(W, H).tobytes() and flows[2][1].tobytes() == fv.download(W, H).tobytes()
        # refusals
        ok = [{n: q.ptr for n, q in step.items()} for step in out]
        frames_ptr = [q.ptr for q in dev]
        for bad in (dict(fill=0), dict(fill=5), dict(min_state=2), dict(min_state=-1), dict(predict_neighbours=0), dict(predict_neighbours=9),
                    dict(sequence_max_shift=0.0), dict(sequence_max_shift=float("nan")), dict(radius=16), dict(passes=[])):
            kw = dict(dict(passes=PASSES, radius=R), **bad)
            with pytest.raises(flow2d.Flow2DError):
                flow.correlate_subset_sequence_device(frames_ptr, lo, scale, kw.pop("passes"), kw.pop("radius"), ok, **kw)
        without_state = [dict(step) for step in ok]
        del without_state[1]["state"]
        shared = [dict(step) for step in ok]
        shared[2]["ux"] = shared[0]["ux"]
        a_frame = [dict(step) for step in ok]
        a_frame[0]["u"] = dev[2].ptr
        for planes in (without_state, shared, a_frame):
            with pytest.raises(flow2d.Flow2DError):
                flow.correlate_subset_sequence_device(frames_ptr, lo, scale, PASSES, R, planes)
        with pytest.raises(ValueError):
            flow.correlate_subset_sequence_device(frames_ptr[:1], lo, scale, PASSES, R, [])
        assert flow2d.OpticalFlow.sequence_options_ok(4, 0, 8, 0.5) and not flow2d.OpticalFlow.sequence_options_ok(5)
    finally:
        flow.close()
    grouped = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx, group_size=2)
    try:
        tall = [ctx.plane(W, 2 * H, np.zeros((2 * H, W), F32)) for _ in range(11)]
        planes = [dict(zip(Refined.NAMES, [q.ptr for q in tall[3:11]]))]
        with pytest.raises(flow2d.Flow2DError):
            grouped.correlate_subset_sequence_device([tall[0].ptr, tall[1].ptr], 0.0, 1.0, PASSES, R, planes)
    finally:
        grouped.close()


def test_cli_subset_previous(flow2d, ctx, tmp_path):
    """Frame by frame through the command line: the second run reads the first one's node files and writes the planes of step 2 of
    OpticalFlow.correlate_subset_sequence; one "Prediction:" line; a grid that does not match the files is refused."""
    _, frames = frames_of_the_rotation()
    paths = []
    for k, f in enumerate(frames[:3]):
        paths.append(str(tmp_path / ("f%d.raw" % k)))
        f.tofile(paths[-1])
    grid_options = ["--correlation", "7", "--correlation-range", "6", "--subset-refine", str(R)]

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
        nodes, _, steps, _, flows = flow.correlate_subset_sequence(frames[:3], PASSES, R, flow=True)
    finally:
        flow.close()
    nw, nh = grid(W, H, 7, 8)
    q1, files1 = run(grid_options, (0, 1), tmp_path / "step1")
    assert q1.returncode == 0 and "Prediction: " not in q1.stdout, q1.stdout[-2000:]
    for name, plane in nodes[0].items():
        assert files1["t_%s-%d-%d.raw" % (FILES[name], nw, nh)] == plane.tobytes(), name
    q2, files2 = run(grid_options + ["--subset-previous", str(tmp_path / "step1") + "/t_"], (0, 2), tmp_path / "step2")
    assert q2.returncode == 0, q2.stdout[-2000:]
    for name, plane in nodes[1].items():
        assert files2["t_%s-%d-%d.raw" % (FILES[name], nw, nh)] == plane.tobytes(), name
    assert files2["t_flow-u-96-80.raw"] == flows[1][0].tobytes() and files2["t_flow-v-96-80.raw"] == flows[1][1].tobytes()
    line = printed(q2, "Prediction")
    assert (line["fill"], line["min_state"], line["min_neighbours"]) == (2, 1, 1)
    assert line["passes"] == [steps[1].prediction[k].summary() for k in range(2)]
    subset = printed(q2, "Subset")
    counts = steps[1].subset.summary()
    counts["iterations_run"] = counts.pop("iterations")
    assert {k: subset[k] for k in counts} == counts and subset["passes"] == 0 and F32(subset["max_shift"]) == F32(4.0)
    # other options reach the prediction; a grid the files do not have is a bad input; the option alone is a usage error
    q3, _ = run(grid_options + ["--subset-previous", str(tmp_path / "step1") + "/t_", "--subset-fill", "1", "--subset-min-state", "0",
                                "--subset-predict-neighbours", "3", "--subset-max-shift", "3"], (0, 2), tmp_path / "step2b")
    line = printed(q3, "Prediction")
    assert q3.returncode == 0 and (line["fill"], line["min_state"], line["min_neighbours"], len(line["passes"])) == (1, 0, 3, 1)
    assert F32(printed(q3, "Subset")["max_shift"]) == F32(3.0)
    q4, files4 = run(["--correlation", "7", "--correlation-range", "6", "--correlation-spacing", "7", "--subset-refine", str(R),
                      "--subset-previous", str(tmp_path / "step1") + "/t_"], (0, 2), tmp_path / "other_grid")
    assert q4.returncode == 2 and not files4, q4.stdout[-2000:]
    for bad in (["--subset-previous", "x_"], ["--subset-fill", "2"] + grid_options,
                grid_options + ["--subset-previous", "x_", "--subset-fill", "5"], grid_options + ["--subset-previous", "x_", "--subset-min-state", "2"]):
        q = subprocess.run([flow2d.CLI_PATH] + bad + paths[:2] + [str(W), str(H), "t_"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=60)
        assert q.returncode == 5, (bad, q.stdout[-500:])
