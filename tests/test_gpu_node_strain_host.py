"""The layers above flow2d_node_strain_2d on the device: OpticalFlow.node_strain_device, OpticalFlow.node_strain and the CLI's
--subset-strain on one 96 x 80 speckle deformation pair and on three steps of the rotation sequence, each against
Context.node_strain called by hand on the same node planes -- planes byte for byte, records byte for byte; the CLI's node files
read back; the refusals and lock-step groups."""
import json
import subprocess

import numpy as np
import pytest

from test_correlate_cpu import F32, U32, frame_range, grid, scenes_module
from test_gpu_multipass import POISON
from test_gpu_subset_sequence_host import FILES, PASSES, STEPS, H, R, W, frames_of_the_rotation

pytestmark = pytest.mark.gpu
STRAIN_FILES = {"divergence": "node-divergence", "vorticity": "node-vorticity", "dilatation": "node-dilatation", "exx": "node-exx",
                "eyy": "node-eyy", "exy": "node-exy", "e1": "node-e1", "e2": "node-e2", "max_shear": "node-max-shear"}
# (window, order, measure, min_nodes)
FORMS = [(2, 1, 0, 0), (0, 1, 1, 0), (3, 2, 1, 9)]


def by_hand(flow2d, ctx, step, nw, nh, s, window, order, measure, min_nodes, min_state=1, state=True, gradients=True):
    """Context.node_strain on a step's device planes: ({name: bits of the grid}, record bytes)."""
    planes = {name: ctx.plane(W, H).fill_bytes(0x7F) for name in flow2d.DEFORMATION_PLANES}
    record = ctx.deformation_records().fill_bytes(0x7F)
    ctx.node_strain(step["u"], step["v"], nw, nh, s, window, order, min_nodes, min_state, measure, state=step["state"] if state else None,
                    gradients=[step[n] for n in ("ux", "uy", "vx", "vy")] if gradients else None, planes=planes, stats=record)
    ctx.synchronize()
    return {name: q.download(nw, nh).view(U32) for name, q in planes.items()}, bytes(ctx.read_deformation_stats(record)[0])


def check_device(flow2d, ctx, flow, steps, nw, nh, s):
    """node_strain_device over the steps' planes against by_hand, with and without the record."""
    names = flow2d.DEFORMATION_PLANES
    new = lambda: ctx.plane(W, H).fill_bytes(0x7F)  # noqa: E731
    ptrs = [{n: q.ptr for n, q in step.items()} for step in steps]
    for window, order, measure, min_nodes in FORMS:
        outs = [{name: new() for name in names} for _ in steps]
        dev_planes = [{n: q.ptr for n, q in out.items()} for out in outs]
        if len(steps) == 1:
            recs = [flow.node_strain_device(ptrs[0], nw, nh, s, window, order, min_nodes, measure=measure, dev_planes=dev_planes[0])]
        else:
            recs = flow.node_strain_device(ptrs, nw, nh, s, window, order, min_nodes, measure=measure, dev_planes=dev_planes)
        assert len(recs) == len(steps)
        for k, step in enumerate(steps):
            want, want_record = by_hand(flow2d, ctx, step, nw, nh, s, window, order, measure, min_nodes)
            assert bytes(recs[k]) == want_record, (window, k)
            assert recs[k].valid > 0.5 * nw * nh and recs[k].valid + recs[k].invalid == nw * nh
            for name in names:
                got = outs[k][name].download().view(U32)
                assert np.array_equal(got[:nh, :nw], want[name]), (window, k, name)
                assert (got[nh:] == POISON).all() and (got[:, nw:] == POISON).all(), (window, k, name)
        # two planes and no record: only queued, the other planes untouched; the record alone
        some = [{name: new() for name in ("exx", "e2")} for _ in steps]
        assert flow.node_strain_device(ptrs if len(steps) > 1 else ptrs[0], nw, nh, s, window, order, min_nodes, measure=measure,
                                       dev_planes=[{n: q.ptr for n, q in out.items()} for out in some] if len(steps) > 1
                                       else {n: q.ptr for n, q in some[0].items()}, stats=False) is None
        ctx.synchronize()
        alone = flow.node_strain_device(ptrs if len(steps) > 1 else ptrs[0], nw, nh, s, window, order, min_nodes, measure=measure)
        alone = alone if len(steps) > 1 else [alone]
        for k in range(len(steps)):
            assert bytes(alone[k]) == bytes(recs[k])
            for name in some[k]:
                assert np.array_equal(some[k][name].download(nw, nh).view(U32), outs[k][name].download(nw, nh).view(U32)), (window, k, name)
    return recs


def run_cli(flow2d, options, files, out):
    out.mkdir()
    q = subprocess.run([flow2d.CLI_PATH, "--flo"] + options + list(files) + [str(W), str(H), "t_", str(out) + "/"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    return q, {f.name: f.read_bytes() for f in out.iterdir()}


def printed(q, what):
    line = [x for x in q.stdout.splitlines() if x.startswith(what + ": ")]
    assert len(line) == 1, q.stdout[-2000:]
    return json.loads(line[0][len(what) + 2:])


def check_cli_files(files, nw, nh, planes, stats, line):
    for name, plane in planes.items():
        assert files["t_%s-%d-%d.raw" % (STRAIN_FILES[name], nw, nh)] == plane.tobytes(), name
    assert (line["valid"], line["invalid"]) == (stats.valid, stats.invalid)
    assert [line["centre"], line["sparse"], line["degenerate"]] == list(stats.reserved[:3])
    for name in ("divergence", "vorticity", "dilatation", "e1", "e2", "max_shear"):
        m = getattr(stats, name)
        assert line[name]["sum"] == m.sum and line[name]["sum_sq"] == m.sum_sq, name
        assert F32(line[name]["min"]) == F32(m.min) and F32(line[name]["max"]) == F32(m.max), name


def test_pair(flow2d, ctx, tmp_path):
    scene = scenes_module().make_speckle_deformation("stretch", W, H, seed=0)
    f0, f1 = scene.frame_0, scene.frame_1
    lo, scale = frame_range(f0, f1)
    names = flow2d.OpticalFlow.SUBSET_PLANES
    r, _, s = PASSES[-1]
    nw, nh = grid(W, H, r, s)
    d0, d1 = ctx.plane(W, H, f0), ctx.plane(W, H, f1)
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        step = {name: ctx.plane(W, H).fill_bytes(0x7F) for name in names}
        flow.correlate_subset_device(d0.ptr, d1.ptr, lo, scale, PASSES, R, dev_out={n: q.ptr for n, q in step.items()})
        recs = check_device(flow2d, ctx, flow, [step], nw, nh, s)
        print("pair, window 3 order 2:", json.dumps(recs[0].summary()))
        # the host-image form, on the arrays correlate_subset returns
        nodes = flow.correlate_subset(f0, f1, PASSES, R)[0]
        for name in names:
            assert nodes[name].tobytes() == step[name].download(nw, nh).tobytes(), name
        for window, order, measure, min_nodes in FORMS:
            got, stats = flow.node_strain(nodes, s, window, order, min_nodes, measure=measure)
            want, want_record = by_hand(flow2d, ctx, step, nw, nh, s, window, order, measure, min_nodes)
            assert bytes(stats) == want_record and set(got) == set(flow2d.DEFORMATION_PLANES)
            for name in got:
                assert np.array_equal(got[name].view(U32), want[name]), (window, name)
        # a field from the search alone: u and v, no state, every finite node usable; one plane, no record
        got, stats = flow.node_strain({"u": nodes["u"], "v": nodes["v"]}, s, 1, planes=("vorticity",), stats=False)
        want, _ = by_hand(flow2d, ctx, step, nw, nh, s, 1, 1, 0, 0, state=False, gradients=False)
        assert stats is None and list(got) == ["vorticity"] and np.array_equal(got["vorticity"].view(U32), want["vorticity"])
        # min_state 0 takes the unconverged nodes too: the same call by hand
        got, stats = flow.node_strain(nodes, s, 2, min_state=0)
        want, want_record = by_hand(flow2d, ctx, step, nw, nh, s, 2, 1, 0, 0, min_state=0)
        assert bytes(stats) == want_record and np.array_equal(got["e1"].view(U32), want["e1"])
        # refusals
        ptrs = {n: q.ptr for n, q in step.items()}
        for bad in (dict(window=8), dict(window=-1), dict(order=3), dict(min_nodes=2), dict(min_nodes=26), dict(min_state=2), dict(measure=2)):
            assert not flow2d.OpticalFlow.strain_options_ok(**bad), bad
            with pytest.raises(flow2d.Flow2DError):
                flow.node_strain_device(ptrs, nw, nh, s, **bad)
            with pytest.raises(flow2d.Flow2DError):
                flow.node_strain(nodes, s, **bad)
        assert flow2d.OpticalFlow.strain_options_ok(7, 2, 225, 0, 1) and flow2d.OpticalFlow.strain_options_ok(0, 5, 99)
        for bad_nodes in ({"u": ptrs["u"], "v": ptrs["v"]}, {"u": ptrs["u"], "v": ptrs["v"], "ux": ptrs["ux"]}):
            with pytest.raises(flow2d.Flow2DError):
                flow.node_strain_device(bad_nodes, nw, nh, s, 0 if len(bad_nodes) == 2 else 2)
        with pytest.raises(flow2d.Flow2DError):
            flow.node_strain_device({"v": ptrs["v"]}, nw, nh, s)
        with pytest.raises(flow2d.Flow2DError):
            flow.node_strain_device(ptrs, W + 1, nh, s)
        with pytest.raises(flow2d.Flow2DError):
            flow.node_strain_device(ptrs, nw, nh, s, dev_planes={"exx": ptrs["u"]})  # an output on an input
        with pytest.raises(ValueError):
            flow.node_strain({"u": nodes["u"]}, s)
        with pytest.raises(ValueError):
            flow.node_strain(nodes, s, planes=("strain",))
        # the CLI: refined nodes with states, then the search alone
        paths = [str(tmp_path / "f0.raw"), str(tmp_path / "f1.raw")]
        f0.tofile(paths[0])
        f1.tofile(paths[1])
        chain = ["--correlation", "7", "--correlation-range", "6", "--subset-refine", str(R)]
        q, files = run_cli(flow2d, chain + ["--subset-strain", "3", "--strain-order", "2", "--strain-min-nodes", "9", "--strain", "green"],
                           paths, tmp_path / "refined")
        assert q.returncode == 0, q.stdout[-2000:]
        for name in names:
            assert files["t_%s-%d-%d.raw" % (FILES[name], nw, nh)] == nodes[name].tobytes(), name
        planes, stats = flow.node_strain(nodes, s, 3, 2, 9, measure=1)
        line = printed(q, "NodeStrain")
        assert (line["window"], line["order"], line["min_nodes"], line["min_state"], line["measure"], line["spacing"]) == (3, 2, 9, 1, "green", s)
        check_cli_files(files, nw, nh, planes, stats, line)
        q, files = run_cli(flow2d, chain + ["--subset-strain", "0"], paths, tmp_path / "direct")
        assert q.returncode == 0, q.stdout[-2000:]
        check_cli_files(files, nw, nh, *flow.node_strain(nodes, s, 0), printed(q, "NodeStrain"))
        q, files = run_cli(flow2d, ["--correlation", "7", "--correlation-range", "6", "--subset-strain", "1"], paths, tmp_path / "search")
        assert q.returncode == 0, q.stdout[-2000:]
        found = {n: np.frombuffer(files["t_node-%s-%d-%d.raw" % (n, nw, nh)], F32).reshape(nh, nw) for n in ("u", "v")}
        check_cli_files(files, nw, nh, *flow.node_strain(found, s, 1), printed(q, "NodeStrain"))
        q, files = run_cli(flow2d, ["--correlation-passes", "7:6:8", "--subset-strain", "2", "--strain-order", "2"], paths, tmp_path / "passes")
        assert q.returncode == 0, q.stdout[-2000:]
        found = {n: np.frombuffer(files["t_node-%s-%d-%d.raw" % (n, nw, nh)], F32).reshape(nh, nw) for n in ("u", "v")}
        check_cli_files(files, nw, nh, *flow.node_strain(found, s, 2, 2), printed(q, "NodeStrain"))
    finally:
        flow.close()
    grouped = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx, group_size=2)
    try:
        tall = [ctx.plane(W, 2 * H, np.zeros((2 * H, W), F32)) for _ in range(3)]
        with pytest.raises(flow2d.Flow2DError):
            grouped.node_strain_device({"u": tall[0].ptr, "v": tall[1].ptr}, nw, nh, s, dev_planes={"exx": tall[2].ptr})
    finally:
        grouped.close()


def test_sequence(flow2d, ctx, tmp_path):
    _, frames = frames_of_the_rotation()
    lo, scale = frame_range(frames[0], frames[1])
    names = flow2d.OpticalFlow.SUBSET_PLANES
    r, _, s = PASSES[-1]
    nw, nh = grid(W, H, r, s)
    dev = [ctx.plane(W, H, f) for f in frames]
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        steps = [{name: ctx.plane(W, H).fill_bytes(0x7F) for name in names} for _ in range(STEPS)]
        flow.correlate_subset_sequence_device([q.ptr for q in dev], lo, scale, PASSES, R, [{n: q.ptr for n, q in step.items()} for step in steps])
        recs = check_device(flow2d, ctx, flow, steps, nw, nh, s)
        assert len({bytes(q) for q in recs}) == STEPS  # three different steps
        # the host-image form over the list of steps correlate_subset_sequence returns
        nodes = flow.correlate_subset_sequence(frames, PASSES, R)[0]
        for window, order, measure, min_nodes in FORMS:
            got = flow.node_strain(nodes, s, window, order, min_nodes, measure=measure)
            assert len(got) == STEPS
            for k, (planes, stats) in enumerate(got):
                want, want_record = by_hand(flow2d, ctx, steps[k], nw, nh, s, window, order, measure, min_nodes)
                assert bytes(stats) == want_record, (window, k)
                for name in planes:
                    assert np.array_equal(planes[name].view(U32), want[name]), (window, k, name)
        with pytest.raises(ValueError):
            flow.node_strain_device([{n: q.ptr for n, q in step.items()} for step in steps], nw, nh, s, dev_planes=[{}])
        # the CLI frame by frame: step 2 through --subset-previous, with the prediction's least state
        paths = []
        for k, f in enumerate(frames[:3]):
            paths.append(str(tmp_path / ("f%d.raw" % k)))
            f.tofile(paths[-1])
        chain = ["--correlation", "7", "--correlation-range", "6", "--subset-refine", str(R), "--subset-strain", "2"]
        q1, files1 = run_cli(flow2d, chain, (paths[0], paths[1]), tmp_path / "step1")
        assert q1.returncode == 0, q1.stdout[-2000:]
        check_cli_files(files1, nw, nh, *flow.node_strain(nodes[0], s, 2), printed(q1, "NodeStrain"))
        q2, files2 = run_cli(flow2d, chain + ["--subset-previous", str(tmp_path / "step1") + "/t_"], (paths[0], paths[2]), tmp_path / "step2")
        assert q2.returncode == 0, q2.stdout[-2000:]
        for name in names:
            assert files2["t_%s-%d-%d.raw" % (FILES[name], nw, nh)] == nodes[1][name].tobytes(), name
        check_cli_files(files2, nw, nh, *flow.node_strain(nodes[1], s, 2), printed(q2, "NodeStrain"))
    finally:
        flow.close()
