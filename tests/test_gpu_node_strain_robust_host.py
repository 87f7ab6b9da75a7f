"""The layers above flow2d_node_strain_robust_2d on the device: OpticalFlow.node_strain and node_strain_device with sigma= over
one 96 x 80 speckle pair and over two steps of the rotation sequence, each against Context.node_strain_robust called by hand on
the same node planes -- the twelve planes and the records byte for byte; with sigma unset the plain entry's bytes and the CLI's
lines as they were; the CLI's twelve files and both lines against the Python route."""
import numpy as np
import pytest

from test_correlate_cpu import F32, U32, frame_range, grid, scenes_module
from test_gpu_multipass import POISON
from test_gpu_node_strain_host import STRAIN_FILES, by_hand, check_cli_files, printed, run_cli
from test_gpu_subset_sequence_host import PASSES, H, R, W, frames_of_the_rotation

pytestmark = pytest.mark.gpu
DIAGNOSTIC_FILES = {"residual": "node-strain-residual", "rejected": "node-strain-rejected", "centre": "node-strain-centre"}
SIGMA = 0.05
# (window, order, measure, min_nodes, iterations)
FORMS = [(2, 1, 0, 0, 8), (3, 2, 1, 9, 4), (1, 1, 0, 0, 0)]


def spoil(nodes):
    """The node field with one usable interior node moved by 2.5 px: what a refinement that converged to a wrong place delivers."""
    out = {name: np.array(a) for name, a in nodes.items()}
    nh, nw = out["u"].shape
    j, i = nh // 2, nw // 2
    assert out["state"][j, i] >= 1
    out["u"][j, i] += F32(2.5)
    return out, (j, i)


def robust_by_hand(flow2d, ctx, nodes, s, window, order, measure, min_nodes, iterations, min_state=1):
    """Context.node_strain_robust on the uploaded arrays: ({name: bits of the grid} for the twelve planes, record bytes)."""
    nh, nw = nodes["u"].shape
    names = flow2d.DEFORMATION_PLANES + flow2d.NODE_STRAIN_DIAGNOSTICS
    held = {name: ctx.plane(W, H).fill_bytes(0x7F) for name in names}
    record = ctx.deformation_records().fill_bytes(0x7F)
    up = {name: ctx.plane(W, H, np.pad(nodes[name], ((0, H - nh), (0, W - nw)))) for name in ("u", "v", "state")}
    ctx.node_strain_robust(up["u"], up["v"], nw, nh, s, window, order, min_nodes, min_state, measure, SIGMA, iterations, state=up["state"],
                           planes={n: held[n] for n in flow2d.DEFORMATION_PLANES},
                           diagnostics={n: held[n] for n in flow2d.NODE_STRAIN_DIAGNOSTICS}, stats=record)
    ctx.synchronize()
    return {name: q.download(nw, nh).view(U32) for name, q in held.items()}, bytes(ctx.read_deformation_stats(record)[0])


def check_both_routes(flow2d, ctx, flow, steps, s):
    """node_strain and node_strain_device with sigma over the steps (host arrays) against robust_by_hand; returns what
    robust_by_hand gave per step for the first of FORMS."""
    nh, nw = steps[0]["u"].shape
    names = flow2d.DEFORMATION_PLANES + flow2d.NODE_STRAIN_DIAGNOSTICS
    single = len(steps) == 1
    first = None
    for window, order, measure, min_nodes, iterations in FORMS:
        wants = [robust_by_hand(flow2d, ctx, q, s, window, order, measure, min_nodes, iterations) for q in steps]
        got = flow.node_strain(steps[0] if single else steps, s, window, order, min_nodes, measure=measure, sigma=SIGMA, iterations=iterations,
                               diagnostics=flow2d.NODE_STRAIN_DIAGNOSTICS)
        got = [got] if single else got
        assert len(got) == len(steps)
        for k, (planes, stats) in enumerate(got):
            assert set(planes) == set(names) and bytes(stats) == wants[k][1], (window, k)
            for name in names:
                assert np.array_equal(planes[name].view(U32), wants[k][0][name]), (window, k, name)
        # the device form on uploaded planes, the outputs in containers whose padding stays
        dev = [{n: ctx.plane(W, H, np.pad(q[n], ((0, H - nh), (0, W - nw)))) for n in ("u", "v", "state")} for q in steps]
        outs = [{n: ctx.plane(W, H).fill_bytes(0x7F) for n in names} for _ in steps]
        ptr = lambda d, keys: {n: d[n].ptr for n in keys}  # noqa: E731
        nodes_arg = [ptr(d, d) for d in dev]
        planes_arg = [ptr(o, flow2d.DEFORMATION_PLANES) for o in outs]
        diag_arg = [ptr(o, flow2d.NODE_STRAIN_DIAGNOSTICS) for o in outs]
        recs = flow.node_strain_device(nodes_arg[0] if single else nodes_arg, nw, nh, s, window, order, min_nodes, measure=measure,
                                       dev_planes=planes_arg[0] if single else planes_arg, sigma=SIGMA, iterations=iterations,
                                       diagnostics=diag_arg[0] if single else diag_arg)
        recs = [recs] if single else recs
        for k in range(len(steps)):
            assert bytes(recs[k]) == wants[k][1], (window, k)
            for name in names:
                full = outs[k][name].download().view(U32)
                assert np.array_equal(full[:nh, :nw], wants[k][0][name]), (window, k, name)
                assert (full[nh:] == POISON).all() and (full[:, nw:] == POISON).all(), (window, k, name)
        # a diagnostic plane alone, no record: only queued
        alone = [ctx.plane(W, H).fill_bytes(0x7F) for _ in steps]
        only = [{"rejected": q.ptr} for q in alone]
        assert flow.node_strain_device(nodes_arg[0] if single else nodes_arg, nw, nh, s, window, order, min_nodes, measure=measure, stats=False,
                                       sigma=SIGMA, iterations=iterations, diagnostics=only[0] if single else only) is None
        ctx.synchronize()
        for k in range(len(steps)):
            assert np.array_equal(alone[k].download(nw, nh).view(U32), wants[k][0]["rejected"]), (window, k)
        first = first or wants
    return first  # (of FORMS[0])


def test_pair_and_cli(flow2d, ctx, tmp_path):
    scene = scenes_module().make_speckle_deformation("stretch", W, H, seed=0)
    f0, f1 = scene.frame_0, scene.frame_1
    r, _, s = PASSES[-1]
    nw, nh = grid(W, H, r, s)
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        nodes = flow.correlate_subset(f0, f1, PASSES, R)[0]
        spoiled, (j, i) = spoil(nodes)
        wants = check_both_routes(flow2d, ctx, flow, [spoiled], s)
        # the spoiled node is named: with m = 2 its own tap is not kept, and every window around it rejected one tap
        planes, stats = flow.node_strain(spoiled, s, 2, sigma=SIGMA, diagnostics=("rejected", "centre"))
        counts = flow2d.node_strain_robust_counts(stats)
        print("robust counts on the spoiled pair:", counts)
        assert counts["suspect"] >= 1 and planes["centre"][j, i] > 2.0 and planes["rejected"][j, i] >= 1
        assert bytes(stats) == wants[0][1]
        # sigma unset: the plain entry's bytes, whatever was set before, and no diagnostics with it
        for window, order, measure, min_nodes in ((2, 1, 0, 0), (3, 2, 1, 9)):
            got, rec = flow.node_strain(spoiled, s, window, order, min_nodes, measure=measure)
            up = {n: ctx.plane(W, H, np.pad(spoiled[n], ((0, H - nh), (0, W - nw)))) for n in ("u", "v", "ux", "uy", "vx", "vy", "state")}
            want, want_record = by_hand(flow2d, ctx, up, nw, nh, s, window, order, measure, min_nodes)
            assert bytes(rec) == want_record and set(got) == set(flow2d.DEFORMATION_PLANES) and not any(rec.reserved[3:])
            for name in got:
                assert np.array_equal(got[name].view(U32), want[name]), (window, name)
        with pytest.raises(ValueError):
            flow.node_strain(spoiled, s, 2, diagnostics=("rejected",))
        with pytest.raises(ValueError):
            flow.node_strain(spoiled, s, 2, sigma=SIGMA, diagnostics=("kept",))
        for bad in (dict(window=0, sigma=SIGMA), dict(sigma=SIGMA, iterations=17)):
            with pytest.raises((flow2d.Flow2DError, ValueError)):
                flow.node_strain(spoiled, s, **bad)
        # the CLI on the clean pair: the twelve files and both lines against the Python route; without the option the lines
        # and the files are what they were
        paths = [str(tmp_path / "f0.raw"), str(tmp_path / "f1.raw")]
        f0.tofile(paths[0])
        f1.tofile(paths[1])
        chain = ["--correlation", "7", "--correlation-range", "6", "--subset-refine", str(R), "--subset-strain", "2", "--strain-order", "2"]
        q, files = run_cli(flow2d, chain + ["--strain-sigma", "0.05", "--strain-iterations", "4"], paths, tmp_path / "robust")
        assert q.returncode == 0, q.stdout[-2000:]
        planes, stats = flow.node_strain(nodes, s, 2, 2, sigma=SIGMA, iterations=4, diagnostics=flow2d.NODE_STRAIN_DIAGNOSTICS)
        check_cli_files(files, nw, nh, {n: planes[n] for n in STRAIN_FILES}, stats, printed(q, "NodeStrain"))
        for name, stem in DIAGNOSTIC_FILES.items():
            assert files["t_%s-%d-%d.raw" % (stem, nw, nh)] == planes[name].tobytes(), name
        line = printed(q, "NodeStrainRobust")
        counts = flow2d.node_strain_robust_counts(stats)
        assert F32(line["sigma"]) == F32(SIGMA) and line["iterations"] == 4
        assert {k: line[k] for k in counts} == counts
        q0, files0 = run_cli(flow2d, chain, paths, tmp_path / "plain")
        assert q0.returncode == 0 and "NodeStrainRobust" not in q0.stdout
        assert not [name for name in files0 if "node-strain-" in name] and len(files) == len(files0) + 3
        check_cli_files(files0, nw, nh, *flow.node_strain(nodes, s, 2, 2), printed(q0, "NodeStrain"))
        assert set(printed(q0, "NodeStrain")) == set(printed(q, "NodeStrain"))
    finally:
        flow.close()


def test_sequence(flow2d, ctx):
    _, frames = frames_of_the_rotation()
    r, _, s = PASSES[-1]
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        nodes = flow.correlate_subset_sequence(frames[:3], PASSES, R)[0]
        assert len(nodes) == 2
        steps = [spoil(q)[0] for q in nodes]
        wants = check_both_routes(flow2d, ctx, flow, steps, s)
        assert wants[0][1] != wants[1][1]  # two different steps
    finally:
        flow.close()
