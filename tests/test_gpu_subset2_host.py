"""The layers above flow2d_subset_refine2_2d on the device: OpticalFlow.correlate_subset(order=2) and correlate_subset_device
against the chain assembled from the Context calls (the multi-pass chain validated with replacement, Context.subset_refine2,
Context.expand_nodes) byte for byte and against the restatement; order=1 against the call without the argument; refine_nodes*;
three steps of a sequence at order 2 against predict_nodes + subset_refine2 assembled by hand; the refusals and lock-step groups;
the CLI's --subset-order 2 (the six extra files, the "SubsetOrder:" line, a run with --subset-order 1 unchanged)."""
import json
import subprocess

import numpy as np
import pytest

from test_correlate_cpu import F32, U32, frame_range, grid, scenes_module
from test_gpu_multipass import POISON, report_bytes
from test_gpu_subset2 import OUT_NAMES, compare2
from test_subset2_cpu import CURVATURES, all_orders2
from test_subset_sequence_cpu import ROTATION, rotation_scenes

pytestmark = pytest.mark.gpu
PASSES = ((15, 8, 16), (7, 3, 8))
W, H, R = 96, 80, 7
FILES = dict(u="node-u", v="node-v", ux="node-ux", uy="node-uy", vx="node-vx", vy="node-vy", score="node-score", state="node-state",
             **{c: "node-" + c for c in CURVATURES})


def bending_pair():
    sc = scenes_module().make_speckle_bending("bend", W, H, seed=0)
    return sc, sc.frame_0, sc.frame_1


def test_chain_equals_its_parts(flow2d, ctx):
    sc, frame_0, frame_1 = bending_pair()
    lo, scale = frame_range(frame_0, frame_1)
    names = flow2d.OpticalFlow.SUBSET2_PLANES
    assert names[:8] == flow2d.OpticalFlow.SUBSET_PLANES and set(names) == set(OUT_NAMES) and names[8:] == CURVATURES
    f0, f1 = ctx.plane(W, H, frame_0), ctx.plane(W, H, frame_1)
    new = lambda: ctx.plane(W, H).fill_bytes(0x7F)  # noqa: E731
    r, _, s = PASSES[-1]
    nw, nh = grid(W, H, r, s)
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        # the host-image form at order 2 against the chain assembled from the Context calls
        nodes, preports, prec, (plo, pscale), (qu, qv) = flow.correlate_subset(frame_0, frame_1, PASSES, R, flow=True, order=2)
        assert tuple(nodes) == names and (F32(plo), F32(pscale)) == (lo, scale)
        su, sv = new(), new()
        chain = flow.correlate_multipass_device(f0.ptr, f1.ptr, lo, scale, PASSES, replace=True, validate_last=True, dev_nodes=(su.ptr, sv.ptr))
        assert report_bytes(chain) == report_bytes(preports)
        hand = {name: new() for name in names}
        record = ctx.subset_records().fill_bytes(0x7F)
        ctx.subset_refine2(f0, f1, W, H, su, sv, nw, nh, r, s, R, out_u=hand["u"], out_v=hand["v"], out_gradients=[hand[n] for n in names[2:6]],
                           out_curvatures=[hand[n] for n in CURVATURES], out_score=hand["score"], out_state=hand["state"], record=record)
        du, dv = new(), new()
        ctx.expand_nodes(hand["u"], hand["v"], nw, nh, r, s, du, dv, W, H)
        ctx.synchronize()
        for name in names:
            assert nodes[name].tobytes() == hand[name].download(nw, nh).tobytes(), name
        assert qu.tobytes() == du.download(W, H).tobytes() and qv.tobytes() == dv.download(W, H).tobytes()
        assert bytes(prec) == record.download(16, 1).tobytes() and prec.nodes == nw * nh and prec.no_input == 0
        print("chain at order 2:", json.dumps(prec.summary()))
        # ... the restatement from the chain's nodes, and what the order is for: the curvature of the bend is found
        want, spread = all_orders2(frame_0, frame_1, su.download(nw, nh), sv.download(nw, nh), r, s, R)
        compare2(({name: nodes[name].view(U32) for name in names}, bytes(prec)), want, spread, "chain")
        inner = (slice(2, -2), slice(2, -2))
        cy, cx = r + np.arange(nh) * s, r + np.arange(nw) * s
        epe = np.hypot(want.u - sc.gt_u[np.ix_(cy, cx)], want.v - sc.gt_v[np.ix_(cy, cx)])[inner]
        assert (want.state[inner] >= 1).all() and epe.mean() < 0.02 and abs(float(nodes["uxy"][inner].mean()) - 0.004) < 1e-3
        # the device form: the same bytes, nothing beyond the grid; u and v alone; refine_nodes_device
        out = {name: new() for name in names}
        fu, fv = new(), new()
        reports, rec = flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, PASSES, R, dev_out={n: q.ptr for n, q in out.items()},
                                                    dev_flow=(fu.ptr, fv.ptr), order=2)
        assert report_bytes(reports) == report_bytes(preports) and bytes(rec) == bytes(prec)
        for name in names:
            got = out[name].download().view(U32)
            assert np.array_equal(got[:nh, :nw], nodes[name].view(U32)), name
            assert (got[nh:] == POISON).all() and (got[:, nw:] == POISON).all(), name
        assert fu.download().tobytes() == du.download().tobytes()
        only = {"u": new(), "v": new()}
        _, rec2 = flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, PASSES, R, dev_out={n: q.ptr for n, q in only.items()}, order=2)
        assert bytes(rec2) == bytes(rec) and only["u"].download().tobytes() == out["u"].download().tobytes()
        again = {name: new() for name in names}
        rec3 = flow.refine_nodes_device(f0.ptr, f1.ptr, su.ptr, sv.ptr, r, s, R, dev_out={n: q.ptr for n, q in again.items()}, order=2)
        assert bytes(rec3) == bytes(rec)
        for name in names:
            assert again[name].download().tobytes() == out[name].download().tobytes(), name
        # order=1 is the call without the argument, byte for byte
        plain = flow.correlate_subset(frame_0, frame_1, PASSES, R, flow=True)
        first = flow.correlate_subset(frame_0, frame_1, PASSES, R, flow=True, order=1, max_curvature=0.05)
        assert tuple(plain[0]) == tuple(first[0]) == flow2d.OpticalFlow.SUBSET_PLANES
        assert all(plain[0][n].tobytes() == first[0][n].tobytes() for n in plain[0]) and bytes(plain[2]) == bytes(first[2])
        assert plain[4][0].tobytes() == first[4][0].tobytes() and report_bytes(plain[1]) == report_bytes(first[1])
        a, b = {n: new() for n in names[:8]}, {n: new() for n in names[:8]}
        _, ra = flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, PASSES, R, dev_out={n: q.ptr for n, q in a.items()})
        _, rb = flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, PASSES, R, dev_out={n: q.ptr for n, q in b.items()}, order=1)
        assert bytes(ra) == bytes(rb) == bytes(plain[2]) and all(a[n].download().tobytes() == b[n].download().tobytes() for n in a)
        assert np.abs(plain[0]["u"] - nodes["u"]).max() > 0.01  # (and the two orders are different refinements)
        # refusals
        for bad in (dict(radius=1), dict(radius=16), dict(order=0), dict(order=3), dict(max_curvature=0.0), dict(max_curvature=float("nan")),
                    dict(iterations=65), dict(passes=[])):
            with pytest.raises(flow2d.Flow2DError):
                flow.correlate_subset(frame_0, frame_1, **dict(dict(passes=PASSES, radius=R, order=2), **bad))
        ok = {n: q.ptr for n, q in out.items()}
        with pytest.raises(flow2d.Flow2DError):  # curvatures in part
            flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, PASSES, R, dev_out={k: v for k, v in ok.items() if k != "vxy"}, order=2)
        with pytest.raises(flow2d.Flow2DError):  # a curvature plane that is a frame
            flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, PASSES, R, dev_out=dict(ok, uyy=f1.ptr), order=2)
        with pytest.raises(ValueError):  # curvature planes belong to order 2
            flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, PASSES, R, dev_out=ok)
        check = flow2d.OpticalFlow.subset_options_ok
        assert check(2, order=2) and check(15, 64, 0.0, order=2, max_curvature=1.0) and not check(1, order=2) and not check(7, order=2, max_curvature=-1.0)
    finally:
        flow.close()
    grouped = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx, group_size=2)
    try:
        tall = [ctx.plane(W, 2 * H, np.zeros((2 * H, W), F32)) for _ in range(6)]
        with pytest.raises(flow2d.Flow2DError):
            grouped.correlate_subset_device(tall[0].ptr, tall[1].ptr, 0.0, 1.0, PASSES, R, dev_out={"u": tall[2].ptr, "v": tall[3].ptr}, order=2)
        with pytest.raises(flow2d.Flow2DError):
            grouped.refine_nodes_device(tall[0].ptr, tall[1].ptr, tall[4].ptr, tall[5].ptr, 7, 8, R, dev_out={"u": tall[2].ptr, "v": tall[3].ptr},
                                        order=2)
    finally:
        grouped.close()


def test_sequence_equals_the_chain_by_hand(flow2d, ctx):
    """Three steps of the rotation sequence at order 2: step 1 is correlate_subset_device(order=2); steps 2 and 3 are two passes of
    predict_nodes on the six first-order planes and subset_refine2 from them with no start curvatures."""
    steps_count, w, h, radius = 3, ROTATION["width"], ROTATION["height"], ROTATION["R"]
    passes = ((7, 6, 8),)
    scenes = rotation_scenes()[:steps_count]
    frames = [scenes[0].frame_0] + [q.frame_1 for q in scenes]
    lo, scale = frame_range(frames[0], frames[1])
    names = flow2d.OpticalFlow.SUBSET2_PLANES
    r, _, s = passes[-1]
    nw, nh = grid(w, h, r, s)
    dev = [ctx.plane(w, h, f) for f in frames]
    new = lambda: ctx.plane(w, h).fill_bytes(0x7F)  # noqa: E731
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        out = [{name: new() for name in names} for _ in range(steps_count)]
        fu, fv = new(), new()
        reports, steps = flow.correlate_subset_sequence_device([q.ptr for q in dev], lo, scale, passes, radius,
                                                               [{n: q.ptr for n, q in step.items()} for step in out],
                                                               dev_flows=[None, None, (fu.ptr, fv.ptr)], order=2)
        hand = [{name: new() for name in names} for _ in range(steps_count)]
        first, rec1 = flow.correlate_subset_device(dev[0].ptr, dev[1].ptr, lo, scale, passes, radius, dev_out={n: q.ptr for n, q in hand[0].items()},
                                                   order=2)
        assert report_bytes(first) == report_bytes(reports) and bytes(rec1) == bytes(steps[0].subset)
        for k in range(1, steps_count):
            last = hand[k - 1]
            ping, pong = [new() for _ in range(7)], [new() for _ in range(7)]
            precs = [ctx.predict_records().fill_bytes(0x7F) for _ in range(2)]
            ctx.predict_nodes([last[n] for n in names[:6]], last["state"], nw, nh, s, 1, 1, ping[:6], ping[6], precs[0])
            ctx.predict_nodes(ping[:6], ping[6], nw, nh, s, 1, 1, pong[:6], pong[6], precs[1])
            record = ctx.subset_records().fill_bytes(0x7F)
            q = hand[k]
            ctx.subset_refine2(dev[0], dev[k + 1], w, h, pong[0], pong[1], nw, nh, r, s, radius, max_shift=4.0, start_gradients=pong[2:6],
                               out_u=q["u"], out_v=q["v"], out_gradients=[q[n] for n in names[2:6]], out_curvatures=[q[n] for n in CURVATURES],
                               out_score=q["score"], out_state=q["state"], record=record)
            ctx.synchronize()
            assert bytes(steps[k].subset) == record.download(16, 1).tobytes(), "record of step %d" % (k + 1)
            for p in range(2):
                assert bytes(steps[k].prediction[p]) == precs[p].download(16, 1).tobytes(), "prediction %d of step %d" % (p, k + 1)
            print("step %d:" % (k + 1), json.dumps(steps[k].summary(2)))
            assert steps[k].subset.converged >= 0.5 * steps[k].subset.nodes
        for k in range(steps_count):
            for name in names:
                got = out[k][name].download().view(U32)
                assert np.array_equal(got[:nh, :nw], hand[k][name].download(nw, nh).view(U32)), (k, name)
                assert (got[nh:] == POISON).all() and (got[:, nw:] == POISON).all(), (k, name)
        du, dv = new(), new()
        ctx.expand_nodes(hand[2]["u"], hand[2]["v"], nw, nh, r, s, du, dv, w, h)
        ctx.synchronize()
        assert fu.download().tobytes() == du.download().tobytes() and fv.download().tobytes() == dv.download().tobytes()
        # the host-image form, and refine_nodes_from_device: step 3 from step 2's planes through the two predictions
        nodes, preports, psteps, _, flows = flow.correlate_subset_sequence(frames, passes, radius, flow=True, order=2)
        assert [bytes(q) for q in psteps] == [bytes(q) for q in steps] and report_bytes(preports) == report_bytes(reports)
        for k in range(steps_count):
            assert tuple(nodes[k]) == names
            for name in names:
                assert nodes[k][name].tobytes() == out[k][name].download(nw, nh).tobytes(), (k, name)
        assert flows[2][0].tobytes() == fu.download(w, h).tobytes()
        again = {name: new() for name in names}
        rec = flow.refine_nodes_from_device(dev[0].ptr, dev[3].ptr, {n: q.ptr for n, q in zip(names[:6], pong)}, r, s, radius,
                                            dev_out={n: q.ptr for n, q in again.items()}, order=2)
        assert bytes(rec) == bytes(steps[2].subset)
        for name in names:
            assert again[name].download().tobytes() == out[2][name].download().tobytes(), name
        # the curvature planes all or none per step; order 1 takes none
        ok = [{n: q.ptr for n, q in step.items()} for step in out]
        part = [dict(step) for step in ok]
        del part[1]["vyy"]
        with pytest.raises(flow2d.Flow2DError):
            flow.correlate_subset_sequence_device([q.ptr for q in dev], lo, scale, passes, radius, part, order=2)
        with pytest.raises(ValueError):
            flow.correlate_subset_sequence_device([q.ptr for q in dev], lo, scale, passes, radius, ok)
    finally:
        flow.close()


def test_cli_subset_order(flow2d, ctx, tmp_path):
    """--subset-order 2 writes the six curvature planes beside the node files of OpticalFlow.correlate_subset(order=2) and prints one
    "SubsetOrder:" line; --subset-order 1 is the run without the option; a bad value or combination is a usage error."""
    sc, frame_0, frame_1 = bending_pair()
    paths = [str(tmp_path / "f0.raw"), str(tmp_path / "f1.raw")]
    frame_0.tofile(paths[0])
    frame_1.tofile(paths[1])
    spec = ",".join("%d:%d:%d" % p for p in PASSES)
    nw, nh = grid(W, H, 7, 8)

    def run(options, out):
        out.mkdir()
        q = subprocess.run([flow2d.CLI_PATH] + options + paths + [str(W), str(H), "t_", str(out) + "/"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=300)
        assert q.returncode == 0, q.stdout[-2000:]
        return q, {f.name: f.read_bytes() for f in out.iterdir()}

    base = ["--flo", "--correlation-passes", spec, "--subset-refine", "7"]
    q, files = run(base + ["--subset-order", "2", "--subset-max-curvature", "0.04"], tmp_path / "second")
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        nodes, _, rec, _, (fu, fv) = flow.correlate_subset(frame_0, frame_1, PASSES, 7, flow=True, order=2, max_curvature=0.04)
    finally:
        flow.close()
    for name, plane in nodes.items():
        assert files["t_%s-%d-%d.raw" % (FILES[name], nw, nh)] == plane.tobytes(), name
    assert sorted(f for f in files if "node" in f) == sorted("t_%s-%d-%d.raw" % (f, nw, nh) for f in FILES.values())
    assert files["t_flow-u-96-80.raw"] == fu.tobytes() and files["t_flow-v-96-80.raw"] == fv.tobytes()
    line = [x for x in q.stdout.splitlines() if x.startswith("SubsetOrder: ")]
    assert len(line) == 1
    printed = json.loads(line[0][len("SubsetOrder: "):])
    assert printed["order"] == 2 and F32(printed["max_curvature"]) == F32(0.04) and set(printed) == {"order", "max_curvature"}
    subset = json.loads([x for x in q.stdout.splitlines() if x.startswith("Subset: ")][0][len("Subset: "):])
    assert subset["converged"] == rec.converged and subset["iterations_run"] == rec.iterations and rec.converged > 30
    q0, plain = run(base, tmp_path / "plain")
    q1, first = run(base + ["--subset-order", "1"], tmp_path / "first")
    strip = lambda text: [x for x in text.splitlines() if "ms" not in x and "time" not in x.lower()]  # noqa: E731
    assert plain == first and len([f for f in plain if "node" in f]) == 8 and "SubsetOrder: " not in q1.stdout
    assert [x for x in strip(q0.stdout) if x.startswith("Subset: ")] == [x for x in strip(q1.stdout) if x.startswith("Subset: ")]
    for bad in (["--subset-order", "2", "--correlation", "7"], ["--subset-refine", "7", "--subset-order", "3", "--correlation", "7"],
                ["--subset-refine", "1", "--subset-order", "2", "--correlation", "7"], ["--subset-refine", "7", "--subset-order"],
                ["--subset-refine", "7", "--subset-max-curvature", "0.1", "--correlation", "7"],
                ["--subset-refine", "7", "--subset-order", "2", "--subset-max-curvature", "0", "--correlation", "7"]):
        q = subprocess.run([flow2d.CLI_PATH] + bad + paths + [str(W), str(H), "t_"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=60)
        assert q.returncode == 5, (bad, q.stdout[-500:])
