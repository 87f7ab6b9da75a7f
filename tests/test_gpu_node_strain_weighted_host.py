"""The layers above flow2d_node_strain_weighted_2d on the device: OpticalFlow.node_strain and node_strain_device with
uncertainty= (the host C API's flow2d_host_node_strain_weighted[_device] behind them) over one 96 x 80 pair of the patchy speckle
scene, behind the refinement and its uncertainty, each against Context.node_strain_weighted called by hand on the same node
planes -- the twenty-one planes and the records byte for byte; afterwards the plain call is the plain entry's again; the CLI's
nine sigma files, its diagnostic files and its "WeightedStrain:" line against the Python route."""
import numpy as np
import pytest

from test_correlate_cpu import F32, U32, grid, scenes_module
from test_gpu_multipass import POISON
from test_gpu_node_strain_host import STRAIN_FILES, by_hand, check_cli_files, printed, run_cli
from test_gpu_node_strain_robust_host import DIAGNOSTIC_FILES
from test_gpu_subset_sequence_host import PASSES, H, R, W

pytestmark = pytest.mark.gpu
SIGMA_FILES = {"sigma_ux": "node-sigma-strain-ux", "sigma_uy": "node-sigma-strain-uy", "sigma_vx": "node-sigma-strain-vx",
               "sigma_vy": "node-sigma-strain-vy", "sigma_divergence": "node-sigma-divergence", "sigma_vorticity": "node-sigma-vorticity",
               "sigma_exx": "node-sigma-exx", "sigma_eyy": "node-sigma-eyy", "sigma_exy": "node-sigma-exy"}
# (window, order, measure, min_nodes, sigma_floor, threshold, iterations)
FORMS = [(2, 1, 0, 0, 0.0, 0.0, 8), (3, 2, 1, 9, 0.005, 3.0, 4), (1, 1, 0, 0, 0.005, 3.0, 0)]


def weighted_by_hand(flow2d, ctx, nodes, unc, s, window, order, measure, min_nodes, floor, threshold, iterations):
    """Context.node_strain_weighted on the uploaded arrays: ({name: bits of the grid} for the twenty-one planes, record bytes)."""
    nh, nw = nodes["u"].shape
    names = flow2d.DEFORMATION_PLANES + flow2d.NODE_STRAIN_DIAGNOSTICS + flow2d.STRAIN_SIGMA_PLANES
    held = {name: ctx.plane(W, H).fill_bytes(0x7F) for name in names}
    record = ctx.deformation_records().fill_bytes(0x7F)
    up = {name: ctx.plane(W, H, np.pad(a[name], ((0, H - nh), (0, W - nw)))) for a, keys in ((nodes, ("u", "v", "state")), (unc, ("sigma_u", "sigma_v")))
          for name in keys}
    pick = lambda keys: {n: held[n] for n in keys}  # noqa: E731
    ctx.node_strain_weighted(up["u"], up["v"], up["sigma_u"], up["sigma_v"], nw, nh, s, window, order, min_nodes, 1, measure, floor, threshold,
                             iterations if threshold > 0 else 0, state=up["state"], planes=pick(flow2d.DEFORMATION_PLANES),
                             diagnostics=pick(flow2d.NODE_STRAIN_DIAGNOSTICS), sigmas=pick(flow2d.STRAIN_SIGMA_PLANES), stats=record)
    ctx.synchronize()
    return {name: q.download(nw, nh).view(U32) for name, q in held.items()}, bytes(ctx.read_deformation_stats(record)[0])


def test_pair_and_cli(flow2d, ctx, tmp_path):
    scene = scenes_module().make_speckle_patchy("stretch", W, H, seed=0)
    f0, f1 = scene.frame_0, scene.frame_1
    r, _, s = PASSES[-1]
    nw, nh = grid(W, H, r, s)
    names = flow2d.DEFORMATION_PLANES + flow2d.NODE_STRAIN_DIAGNOSTICS + flow2d.STRAIN_SIGMA_PLANES
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        nodes = flow.correlate_subset(f0, f1, PASSES, R)[0]
        unc, counts = flow.node_uncertainty(f0, f1, nodes, r, s, R)
        su = unc["sigma_u"][np.isfinite(unc["sigma_u"])]
        print("patchy stretch: %d of %d nodes evaluated, sigma_u %.4g .. %.4g px" % (counts.evaluated, counts.nodes, su.min(), su.max()))
        # the scene does what it is for: the interior nodes are found, and their sigmas spread over most of a decade (the numpy
        # restatements, started from the truth, give 79 of 99 nodes and 0.0040 .. 0.067 px)
        assert counts.evaluated >= 63 and su.max() > 5 * su.min()
        for window, order, measure, min_nodes, floor, threshold, iterations in FORMS:
            want, want_record = weighted_by_hand(flow2d, ctx, nodes, unc, s, window, order, measure, min_nodes, floor, threshold, iterations)
            form = dict(measure=measure, iterations=iterations, sigma_floor=floor, threshold=threshold)
            planes, stats = flow.node_strain(nodes, s, window, order, min_nodes, uncertainty=unc, diagnostics=flow2d.NODE_STRAIN_DIAGNOSTICS,
                                             strain_sigmas=flow2d.STRAIN_SIGMA_PLANES, **form)
            assert set(planes) == set(names) and bytes(stats) == want_record, window
            for name in names:
                assert np.array_equal(planes[name].view(U32), want[name]), (window, name)
            assert np.isfinite(planes["sigma_exx"]).sum() == stats.valid > 0
            # the device form on uploaded planes, the outputs in containers whose padding stays
            pad = lambda a: ctx.plane(W, H, np.pad(a, ((0, H - nh), (0, W - nw))))  # noqa: E731
            dev = {n: pad(nodes[n]).ptr for n in ("u", "v", "state")}
            dev_unc = {n: pad(unc[n]).ptr for n in ("sigma_u", "sigma_v")}
            outs = {n: ctx.plane(W, H).fill_bytes(0x7F) for n in names}
            ptr = lambda keys: {n: outs[n].ptr for n in keys}  # noqa: E731
            rec = flow.node_strain_device(dev, nw, nh, s, window, order, min_nodes, dev_planes=ptr(flow2d.DEFORMATION_PLANES),
                                          diagnostics=ptr(flow2d.NODE_STRAIN_DIAGNOSTICS), uncertainty=dev_unc,
                                          strain_sigmas=ptr(flow2d.STRAIN_SIGMA_PLANES), **form)
            assert bytes(rec) == want_record, window
            for name in names:
                full = outs[name].download().view(U32)
                assert np.array_equal(full[:nh, :nw], want[name]), (window, name)
                assert (full[nh:] == POISON).all() and (full[:, nw:] == POISON).all(), (window, name)
            # a sigma plane alone, no record: only queued
            alone = ctx.plane(W, H).fill_bytes(0x7F)
            assert flow.node_strain_device(dev, nw, nh, s, window, order, min_nodes, stats=False, uncertainty=dev_unc,
                                           strain_sigmas={"sigma_exy": alone.ptr}, **form) is None
            ctx.synchronize()
            assert np.array_equal(alone.download(nw, nh).view(U32), want["sigma_exy"]), window
        # afterwards a call without uncertainty is the plain entry's again
        got, rec = flow.node_strain(nodes, s, 2, 1)
        up = {n: ctx.plane(W, H, np.pad(nodes[n], ((0, H - nh), (0, W - nw)))) for n in ("u", "v", "ux", "uy", "vx", "vy", "state")}
        want, want_record = by_hand(flow2d, ctx, up, nw, nh, s, 2, 1, 0, 0)
        assert bytes(rec) == want_record and not any(rec.reserved[3:])
        for name in got:
            assert np.array_equal(got[name].view(U32), want[name]), name
        # what the host layer refuses
        with pytest.raises(ValueError):
            flow.node_strain(nodes, s, 2, strain_sigmas=("sigma_exx",))
        with pytest.raises(ValueError):
            flow.node_strain(nodes, s, 2, uncertainty=unc, strain_sigmas=("sigma_xx",))
        with pytest.raises(ValueError):
            flow.node_strain(nodes, s, 2, uncertainty={"sigma_u": unc["sigma_u"]})
        for bad in (dict(window=0), dict(sigma=0.05), dict(threshold=3.0, iterations=17), dict(sigma_floor=-1.0)):
            with pytest.raises((flow2d.Flow2DError, ValueError)):
                flow.node_strain(nodes, s, **dict(dict(window=2, uncertainty=unc), **bad))
        # the CLI: the nine sigma files, the diagnostic files and the line against the Python route
        paths = [str(tmp_path / "f0.raw"), str(tmp_path / "f1.raw")]
        f0.tofile(paths[0])
        f1.tofile(paths[1])
        chain = ["--correlation", "7", "--correlation-range", "6", "--subset-refine", str(R), "--subset-uncertainty", "--subset-strain", "2",
                 "--strain-order", "2"]
        q, files = run_cli(flow2d, chain + ["--strain-weighted", "--strain-sigma-floor", "0.005", "--strain-threshold", "3",
                                            "--strain-iterations", "4"], paths, tmp_path / "weighted")
        assert q.returncode == 0, q.stdout[-2000:]
        planes, stats = flow.node_strain(nodes, s, 2, 2, uncertainty=unc, sigma_floor=0.005, threshold=3.0, iterations=4,
                                         diagnostics=flow2d.NODE_STRAIN_DIAGNOSTICS, strain_sigmas=flow2d.STRAIN_SIGMA_PLANES)
        check_cli_files(files, nw, nh, {n: planes[n] for n in STRAIN_FILES}, stats, printed(q, "NodeStrain"))
        for stems in (DIAGNOSTIC_FILES, SIGMA_FILES):
            for name, stem in stems.items():
                assert files["t_%s-%d-%d.raw" % (stem, nw, nh)] == planes[name].tobytes(), name
        assert files["t_node-sigma-u-%d-%d.raw" % (nw, nh)] == unc["sigma_u"].tobytes()
        line = printed(q, "WeightedStrain")
        counts = flow2d.node_strain_weighted_counts(stats)
        assert F32(line["sigma_floor"]) == F32(0.005) and F32(line["threshold"]) == F32(3.0) and line["iterations"] == 4
        assert {k: line[k] for k in counts} == counts and "NodeStrainRobust" not in q.stdout
        # without the option the files and the lines are what they were
        q0, files0 = run_cli(flow2d, chain, paths, tmp_path / "plain")
        assert q0.returncode == 0 and "WeightedStrain" not in q0.stdout
        assert len(files) == len(files0) + 12 and not [name for name in files0 if "node-sigma-e" in name or "node-sigma-strain" in name]
        check_cli_files(files0, nw, nh, *flow.node_strain(nodes, s, 2, 2), printed(q0, "NodeStrain"))
    finally:
        flow.close()
