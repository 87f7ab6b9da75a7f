"""The layers above flow2d_subset_refine_2d on the device: OpticalFlow.correlate_subset_device against its parts (the multi-pass
chain validated with replacement, Context.subset_refine, Context.expand_nodes) byte for byte and against the restatement,
refine_nodes_device, the host-image form, the refusals and lock-step groups; the CLI's --subset-refine (files and the "Subset:"
line, and a run without it unchanged); the device rows of tools/subset_table.py against the committed restatement rows."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_correlate_cpu import F32, U32, bits, frame_range, grid, scenes_module
from test_gpu_multipass import POISON, report_bytes
from test_gpu_subset import compare
from test_subset_cpu import ROOT, SUBSET_DTYPE, Refined, all_orders

pytestmark = pytest.mark.gpu
PASSES = ((15, 8, 16), (7, 3, 8))
W, H, R = 96, 80, 7


def speckle_pair():
    sc = scenes_module().make_speckle_deformation("rotation", W, H, seed=0)
    return sc, sc.frame_0, sc.frame_1


def test_chain_equals_its_parts(flow2d, ctx):
    sc, frame_0, frame_1 = speckle_pair()
    lo, scale = frame_range(frame_0, frame_1)
    names = flow2d.OpticalFlow.SUBSET_PLANES
    assert names == Refined.NAMES
    f0, f1 = ctx.plane(W, H, frame_0), ctx.plane(W, H, frame_1)
    new = lambda: ctx.plane(W, H).fill_bytes(0x7F)  # noqa: E731
    r, _, s = PASSES[-1]
    nw, nh = grid(W, H, r, s)
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        out = {name: new() for name in names}
        fu, fv = new(), new()
        reports, rec = flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, PASSES, R, dev_out={n: q.ptr for n, q in out.items()},
                                                    dev_flow=(fu.ptr, fv.ptr))
        # by hand: the chain with the last pass validated in REPLACE mode, the refinement, the expansion
        su, sv = new(), new()
        chain = flow.correlate_multipass_device(f0.ptr, f1.ptr, lo, scale, PASSES, replace=True, validate_last=True, dev_nodes=(su.ptr, sv.ptr))
        assert report_bytes(chain) == report_bytes(reports) and reports[-1].validation.remaining_invalid == 0
        hand = [new() for _ in range(8)]
        record = ctx.subset_records().fill_bytes(0x7F)
        ctx.subset_refine(f0, f1, W, H, su, sv, nw, nh, r, s, R, out_u=hand[0], out_v=hand[1], out_gradients=hand[2:6], out_score=hand[6],
                          out_state=hand[7], record=record)
        du, dv = new(), new()
        ctx.expand_nodes(hand[0], hand[1], nw, nh, r, s, du, dv, W, H)
        ctx.synchronize()
        for name, q in zip(names, hand):
            got = out[name].download().view(U32)
            assert np.array_equal(got[:nh, :nw], q.download(nw, nh).view(U32)), name
            assert (got[nh:] == POISON).all() and (got[:, nw:] == POISON).all(), name
        assert fu.download().tobytes() == du.download().tobytes() and fv.download().tobytes() == dv.download().tobytes()
        assert bytes(rec) == record.download(16, 1).tobytes() and rec.nodes == nw * nh and rec.no_input == 0
        print("chain:", json.dumps(rec.summary()))
        # the restatement, from the chain's nodes
        want, spread = all_orders(frame_0, frame_1, su.download(nw, nh), sv.download(nw, nh), r, s, R)
        compare(([out[name].download(nw, nh).view(U32) for name in names], bytes(rec)), want, spread, "chain")
        inner = (slice(2, -2), slice(2, -2))
        cy, cx = r + np.arange(nh) * s, r + np.arange(nw) * s
        epe = np.hypot(want.u - sc.gt_u[np.ix_(cy, cx)], want.v - sc.gt_v[np.ix_(cy, cx)])[inner]
        assert (want.state[inner] >= 1).all() and epe.mean() < 0.02
        # u and v alone; the object's own planes behind a dense flow; refine_nodes_device
        only = {"u": new(), "v": new()}
        _, rec2 = flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, PASSES, R, dev_out={n: q.ptr for n, q in only.items()})
        assert bytes(rec2) == bytes(rec) and only["u"].download().tobytes() == out["u"].download().tobytes()
        gu, gv = new(), new()
        flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, PASSES, R, dev_flow=(gu.ptr, gv.ptr))
        assert gu.download().tobytes() == fu.download().tobytes() and gv.download().tobytes() == fv.download().tobytes()
        again = {name: new() for name in names}
        rec3 = flow.refine_nodes_device(f0.ptr, f1.ptr, su.ptr, sv.ptr, r, s, R, dev_out={n: q.ptr for n, q in again.items()})
        assert bytes(rec3) == bytes(rec)
        for name in names:
            assert again[name].download().tobytes() == out[name].download().tobytes(), name
        assert flow.refine_nodes_device(f0.ptr, f1.ptr, su.ptr, sv.ptr, r, s, R, record=False) is None
        ctx.synchronize()
        # one pass without a predictor, other options
        _, rec4 = flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, [(7, 8, 8)], 5, iterations=3, epsilon=0.0, max_shift=1.0,
                                               max_gradient=0.25)
        assert rec4.converged == 0 and rec4.unconverged > 0 and rec4.iterations <= 3 * rec4.nodes
        # the host-image form
        nodes, preports, prec, (plo, pscale), (qu, qv) = flow.correlate_subset(frame_0, frame_1, PASSES, R, flow=True)
        assert (F32(plo), F32(pscale)) == (lo, scale) and bytes(prec) == bytes(rec) and report_bytes(preports) == report_bytes(reports)
        for name in names:
            assert nodes[name].tobytes() == out[name].download(nw, nh).tobytes(), name
        assert qu.tobytes() == fu.download(W, H).tobytes() and qv.tobytes() == fv.download(W, H).tobytes()
        # refusals
        for bad in (dict(radius=0), dict(radius=16), dict(iterations=0), dict(iterations=65), dict(epsilon=-1.0), dict(epsilon=float("nan")),
                    dict(max_shift=0.0), dict(max_gradient=float("inf")), dict(passes=[]), dict(passes=[(16, 8, 8)]), dict(threshold=0.0)):
            with pytest.raises(flow2d.Flow2DError):
                flow.correlate_subset(frame_0, frame_1, **dict(dict(passes=PASSES, radius=R), **bad))
        with pytest.raises(flow2d.Flow2DError):  # an output plane that is a frame
            flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, PASSES, R, dev_out={"u": f0.ptr, "v": out["v"].ptr})
        with pytest.raises(flow2d.Flow2DError):  # gradients in part
            flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, PASSES, R, dev_out={"u": out["u"].ptr, "v": out["v"].ptr, "ux": out["ux"].ptr})
        with pytest.raises(ValueError):
            flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, PASSES, R, dev_out={"w": out["u"].ptr})
        assert flow2d.OpticalFlow.subset_options_ok(15, 64, 0.0) and not flow2d.OpticalFlow.subset_options_ok(16)
    finally:
        flow.close()
    grouped = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx, group_size=2)
    try:
        tall = [ctx.plane(W, 2 * H, np.zeros((2 * H, W), F32)) for _ in range(6)]
        with pytest.raises(flow2d.Flow2DError):
            grouped.correlate_subset_device(tall[0].ptr, tall[1].ptr, 0.0, 1.0, PASSES, R, dev_out={"u": tall[2].ptr, "v": tall[3].ptr})
        with pytest.raises(flow2d.Flow2DError):
            grouped.refine_nodes_device(tall[0].ptr, tall[1].ptr, tall[4].ptr, tall[5].ptr, 7, 8, R, dev_out={"u": tall[2].ptr, "v": tall[3].ptr})
    finally:
        grouped.close()


def test_cli_subset_refine(flow2d, ctx, tmp_path):
    """--subset-refine with --correlation-passes and with --correlation writes the files of OpticalFlow.correlate_subset and prints
    one "Subset:" line; without it no file and no line changes; a bad value or combination is a usage error."""
    sc, frame_0, frame_1 = speckle_pair()
    paths = [str(tmp_path / "f0.raw"), str(tmp_path / "f1.raw")]
    frame_0.tofile(paths[0])
    frame_1.tofile(paths[1])
    spec = ",".join("%d:%d:%d" % p for p in PASSES)

    def run(options, out):
        out.mkdir()
        q = subprocess.run([flow2d.CLI_PATH] + options + paths + [str(W), str(H), "t_", str(out) + "/"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=300)
        return q, {f.name: f.read_bytes() for f in out.iterdir()}

    def printed(q):
        line = [x for x in q.stdout.splitlines() if x.startswith("Subset: ")]
        assert len(line) == 1, q.stdout[-2000:]
        return json.loads(line[0][len("Subset: "):])

    file_of = dict(zip(Refined.NAMES, ("node-u", "node-v", "node-ux", "node-uy", "node-vx", "node-vy", "node-score", "node-state")))
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        for options, passes, kw in ((["--correlation-passes", spec, "--subset-refine", "7"], PASSES, {}),
                                    (["--correlation", "7", "--correlation-range", "6", "--subset-refine", "5", "--subset-iterations", "30",
                                      "--subset-epsilon", "0.01", "--subset-max-shift", "1.5", "--subset-max-gradient", "0.25"], [(7, 6, 8)],
                                     dict(iterations=30, epsilon=0.01, max_shift=1.5, max_gradient=0.25))):
            radius = int(options[options.index("--subset-refine") + 1])
            q, files = run(["--flo"] + options, tmp_path / ("run%d" % radius))
            assert q.returncode == 0, q.stdout[-2000:]
            nodes, reports, rec, (lo, scale), (fu, fv) = flow.correlate_subset(frame_0, frame_1, passes, radius, flow=True, **kw)
            nw, nh = grid(W, H, passes[-1][0], passes[-1][2])
            for name, plane in nodes.items():
                assert files["t_%s-%d-%d.raw" % (file_of[name], nw, nh)] == plane.tobytes(), name
            assert files["t_flow-u-96-80.raw"] == fu.tobytes() and files["t_flow-v-96-80.raw"] == fv.tobytes()
            line = printed(q)
            counts = rec.summary()
            counts["iterations_run"] = counts.pop("iterations")
            assert {k: line[k] for k in counts} == counts and rec.converged > 30
            assert (line["radius"], line["passes"], line["grid_radius"], line["spacing"], line["nw"], line["nh"]) == (radius, len(passes), 7, 8, nw, nh)
            assert (line["iterations"], F32(line["epsilon"]), F32(line["max_shift"]), F32(line["max_gradient"])) == (
                kw.get("iterations", 20), F32(kw.get("epsilon", 1e-3)), F32(kw.get("max_shift", 2.0)), F32(kw.get("max_gradient", 0.5)))
            assert (F32(line["lo"]), F32(line["scale"])) == (F32(lo), F32(scale))
            assert "Correlation: " not in q.stdout and "CorrelationPasses: " not in q.stdout
        # without the option: the files and the line of --correlation-passes, nothing of the subsets
        q, files = run(["--flo", "--correlation-passes", spec], tmp_path / "plain")
        assert q.returncode == 0 and "Subset: " not in q.stdout and "CorrelationPasses: " in q.stdout
        nu, nv, ns, _, _, (fu, fv) = flow.correlate_multipass(frame_0, frame_1, PASSES, flow=True)
        nw, nh = grid(W, H, 7, 8)
        assert sorted(f for f in files if "node" in f) == ["t_node-score-%d-%d.raw" % (nw, nh), "t_node-u-%d-%d.raw" % (nw, nh),
                                                          "t_node-v-%d-%d.raw" % (nw, nh)]
        assert files["t_node-u-%d-%d.raw" % (nw, nh)] == nu.tobytes() and files["t_node-score-%d-%d.raw" % (nw, nh)] == ns.tobytes()
        assert files["t_flow-u-96-80.raw"] == fu.tobytes()
    finally:
        flow.close()
    for bad in (["--subset-refine", "7"], ["--subset-iterations", "5", "--correlation", "7"], ["--subset-refine", "0", "--correlation", "7"],
                ["--subset-refine", "16", "--correlation", "7"], ["--subset-refine", "7", "--subset-iterations", "65", "--correlation", "7"],
                ["--subset-refine", "7", "--subset-epsilon", "-1", "--correlation", "7"], ["--subset-refine", "7", "--subset-max-shift", "0", "--correlation", "7"],
                ["--subset-refine", "7", "--subset-max-gradient", "nan", "--correlation", "7"], ["--subset-refine", "7", "--refine", "3"],
                ["--subset-refine"], ["--subset-refine", "x", "--correlation", "7"]):
        q = subprocess.run([flow2d.CLI_PATH] + bad + paths + [str(W), str(H), "t_"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=60)
        assert q.returncode == 5, (bad, q.stdout[-500:])


def test_table_rows_equal_the_restatement(flow2d, ctx, tmp_path):
    """The device rows of tools/subset_table.py are the committed rows of the restatement, digit for digit."""
    q = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "subset_table.py"), "--out", str(tmp_path)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert q.returncode == 0, q.stdout[-2000:]
    assert "equal to the committed restatement rows" in q.stdout
    got = (tmp_path / "table.md").read_text().splitlines()
    want = open(os.path.join(ROOT, "profiles", "subset", "table_numpy.md")).read().splitlines()
    assert got == want and len(got) == 8
