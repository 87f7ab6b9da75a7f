"""The layers above flow2d_subset_uncertainty_2d on the device: OpticalFlow.node_uncertainty_device after refine_nodes_device
against the entry called by hand (Context.subset_uncertainty) and against the restatement (tests/test_subset_uncertainty_cpu.py),
byte for byte, for both interpolations and with a mask; its host-image form; the order-2 refusal; the record's round trip; and the
CLI's --subset-uncertainty, whose files are the Python call's planes."""
import json
import subprocess

import numpy as np
import pytest

from test_correlate_cpu import F32, bits, grid
from test_subset_masked_cpu import SPECIMEN, specimen_case
from test_subset_uncertainty_cpu import PLANES, UNCERTAINTY_DTYPE, subset_uncertainty_reference

pytestmark = pytest.mark.gpu
W, H, R = SPECIMEN["width"], SPECIMEN["height"], SPECIMEN["R"]
PASSES = ((SPECIMEN["r"], SPECIMEN["d"], SPECIMEN["s"]),)
FILES = dict(zip(PLANES, ("node-sigma-u", "node-sigma-v", "node-rho", "node-sigma-ux", "node-sigma-uy", "node-sigma-vx", "node-sigma-vy",
                          "node-noise")))
FIELD = ("u", "v", "ux", "uy", "vx", "vy")


def same_planes(got, want, what):
    """got: {name: [nh, nw] array}; want: the restatement or another such dict.  Byte for byte; prints the words that differ first."""
    other = want if isinstance(want, dict) else {name: getattr(want, name) for name in PLANES}
    differ = {name: int((bits(got[name]) != bits(other[name])).sum()) for name in PLANES}
    print("%s: words that differ %s" % (what, differ))
    assert not any(differ.values()), "%s: %s" % (what, differ)


@pytest.mark.parametrize("interpolation", ["catmull-rom", "bspline"])
@pytest.mark.parametrize("masked", [False, True])
def test_node_uncertainty_after_refine_nodes(flow2d, ctx, interpolation, masked):
    """refine_nodes_device, then node_uncertainty_device on its planes: the bytes of Context.subset_uncertainty on the same planes
    (with the coefficients of Context.bspline_prefilter), and of the restatement on the downloaded field."""
    scene, mask, u0, v0 = specimen_case("stretch")
    r, _, s = PASSES[-1]
    nw, nh = grid(W, H, r, s)
    spline = interpolation == "bspline"
    f0, f1, pm = ctx.plane(W, H, scene.frame_0), ctx.plane(W, H, scene.frame_1), ctx.plane(W, H, mask)
    start = [ctx.plane(W, H, np.pad(q, ((0, H - nh), (0, W - nw)))) for q in (u0, v0)]
    new = lambda: ctx.plane(W, H).fill_bytes(0x7F)  # noqa: E731
    names = flow2d.OpticalFlow.SUBSET_PLANES
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        field = {name: new() for name in names}
        kw = dict(mask=pm.ptr, min_pixels=57) if masked else {}
        flow.refine_nodes_device(f0.ptr, f1.ptr, start[0].ptr, start[1].ptr, r, s, R, dev_out={n: q.ptr for n, q in field.items()},
                                 interpolation=interpolation, **kw)
        out = {name: new() for name in PLANES}
        rec = flow.node_uncertainty_device(f0.ptr, f1.ptr, {n: q.ptr for n, q in field.items()}, r, s, R, {n: q.ptr for n, q in out.items()},
                                           interpolation=interpolation, **kw)
        got = {n: q.download(nw, nh) for n, q in out.items()}
        for q in out.values():
            assert (q.download().view(np.uint32)[nh:] == 0x7F7F7F7F).all()  # nothing beyond the grid
        # the entry by hand on the same device planes
        second = ctx.bspline_prefilter(f1, W, H) if spline else f1
        by_hand = [new() for _ in PLANES]
        hand_rec = ctx.uncertainty_records()
        ctx.subset_uncertainty(f0, second, W, H, [field[n] for n in FIELD], field["state"], nw, nh, r, s, R, 1, int(spline), pm if masked else None,
                               57, by_hand, hand_rec)
        same_planes(got, {n: q.download(nw, nh) for n, q in zip(PLANES, by_hand)}, "node_uncertainty_device against the entry")
        assert bytes(rec) == bytes(ctx.read_uncertainty_record(hand_rec)[0])
        # ... and the restatement at the field the device refined
        nodes = [field[n].download(nw, nh) for n in FIELD]
        want = subset_uncertainty_reference(scene.frame_0, second.download(W, H), nodes, field["state"].download(nw, nh), r, s, R, 1,
                                            mask if masked else None, 57, int(spline))
        same_planes(got, want, "node_uncertainty_device against the restatement")
        assert bytes(rec) == want.record.tobytes() and rec.nodes == 99 and rec.evaluated >= 40 and (rec.masked == 55) == masked
        print(rec.summary())
        # without a record the call only queues; the planes are the same
        again = {name: new() for name in PLANES}
        assert flow.node_uncertainty_device(f0.ptr, f1.ptr, {n: q.ptr for n, q in field.items()}, r, s, R, {n: q.ptr for n, q in again.items()},
                                            interpolation=interpolation, record=False, **kw) is None
        ctx.synchronize()
        same_planes({n: q.download(nw, nh) for n, q in again.items()}, got, "without a record")
        # optional planes absent: sigma_u and sigma_v alone
        few = {name: new() for name in PLANES[:2]}
        flow.node_uncertainty_device(f0.ptr, f1.ptr, {n: q.ptr for n, q in field.items()}, r, s, R, {n: q.ptr for n, q in few.items()},
                                     interpolation=interpolation, **kw)
        assert all(np.array_equal(bits(few[n].download(nw, nh)), bits(got[n])) for n in few)
        if not spline:
            # the host-image form uploads field and mask itself
            host_nodes = {n: field[n].download(nw, nh) for n in names}
            planes, hrec = flow.node_uncertainty(scene.frame_0, scene.frame_1, host_nodes, r, s, R, mask=mask if masked else None,
                                                 min_pixels=57 if masked else 0)
            same_planes(planes, got, "node_uncertainty")
            assert bytes(hrec) == bytes(rec)
    finally:
        flow.close()


def test_refusals_and_the_record(flow2d, ctx):
    scene, mask, u0, v0 = specimen_case("stretch")
    r, _, s = PASSES[-1]
    nw, nh = grid(W, H, r, s)
    f0, f1 = ctx.plane(W, H, scene.frame_0), ctx.plane(W, H, scene.frame_1)
    new = lambda: ctx.plane(W, H).fill_bytes(0x7F)  # noqa: E731
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        field = {name: new() for name in flow.SUBSET2_PLANES}
        start = [ctx.plane(W, H, np.pad(q, ((0, H - nh), (0, W - nw)))) for q in (u0, v0)]
        flow.refine_nodes_device(f0.ptr, f1.ptr, start[0].ptr, start[1].ptr, r, s, R, dev_out={n: q.ptr for n, q in field.items()}, order=2)
        out = {name: new() for name in PLANES}
        ptrs = {n: q.ptr for n, q in out.items()}
        first = {n: field[n].ptr for n in flow.SUBSET_PLANES}
        # order 2: twelve parameters need a 12 x 12 covariance
        with pytest.raises(flow2d.Flow2DError) as refused:
            flow.node_uncertainty_device(f0.ptr, f1.ptr, first, r, s, R, ptrs, order=2)
        assert refused.value.status == 1
        options = flow2d.SubsetOptions(R, 20, 1e-3, 2.0, 0.5, 2, 0.05, 0, None)
        ok = flow2d.host_lib().flow2d_host_uncertainty_options_ok
        assert ok(options, 1) == 0
        options.order = 1
        assert ok(options, 1) == 1 and ok(options, 0) == 1 and ok(options, 2) == 0 and ok(None, 1) == 0
        for bad in (dict(dev_out={n: ptrs[n] for n in PLANES[:4]}), dict(dev_out={"sigma_u": ptrs["sigma_u"]}), dict(min_state=2),
                    dict(dev_nodes={n: first[n] for n in ("u", "v", "ux", "uy", "vx", "vy")}), dict(radius=16), dict(dev_out=dict(ptrs, rho=f0.ptr)),
                    dict(min_pixels=5, mask=f1.ptr)):
            args = dict(dict(dev_nodes=first, radius=R, dev_out=ptrs), **bad)
            with pytest.raises(flow2d.Flow2DError):
                flow.node_uncertainty_device(f0.ptr, f1.ptr, args.pop("dev_nodes"), r, s, args.pop("radius"), args.pop("dev_out"), **args)
        with pytest.raises(ValueError):
            flow.node_uncertainty_device(f0.ptr, f1.ptr, first, r, s, R, dict(ptrs, sigma=1))
        ctx.synchronize()
        for q in out.values():
            assert (q.download().view(np.uint32) == 0x7F7F7F7F).all()  # a refusal writes nothing
        # the first-order planes of the order-2 field are a field like any other: accepted, and the record round trip
        rec = flow.node_uncertainty_device(f0.ptr, f1.ptr, first, r, s, R, ptrs)
        raw = np.frombuffer(bytes(rec), UNCERTAINTY_DTYPE)[0]
        assert list(rec.summary()) == list(UNCERTAINTY_DTYPE.names[:7]) and [int(raw[n]) for n in rec.summary()] == list(rec.summary().values())
        assert rec.nodes == 99 == rec.evaluated + rec.skipped + rec.masked + rec.outside + rec.flat + rec.thin and rec.reserved == 0
        plane = ctx.uncertainty_records(2).fill_bytes(0)
        assert [bytes(q) for q in ctx.read_uncertainty_record(plane, 2)] == [bytes(64)] * 2
    finally:
        flow.close()


def test_cli_subset_uncertainty(flow2d, ctx, tmp_path):
    """--subset-uncertainty writes the eight files of OpticalFlow.node_uncertainty at the nodes the run refined and prints one
    "SubsetUncertainty:" line; with --subset-mask and --subset-interpolation too; without the option no byte changes; order 2,
    --subset-base and the option alone are usage errors."""
    scene, mask, _, _ = specimen_case("stretch")
    paths = {}
    for name, image in (("f0", scene.frame_0), ("f1", scene.frame_1), ("mask", mask)):
        paths[name] = str(tmp_path / (name + ".raw"))
        image.astype(F32).tofile(paths[name])
    base = ["--correlation", "7", "--correlation-range", "6", "--subset-refine", str(R)]
    nw, nh = grid(W, H, 7, 8)

    def run(options, out):
        out.mkdir()
        q = subprocess.run([flow2d.CLI_PATH, "--flo"] + options + [paths["f0"], paths["f1"], str(W), str(H), "t_", str(out) + "/"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        return q, {f.name: f.read_bytes() for f in out.iterdir()}

    plain, plain_files = run(base, tmp_path / "plain")
    assert plain.returncode == 0 and "SubsetUncertainty" not in plain.stdout
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        for label, options, kw in (("pair", [], {}), ("masked", ["--subset-mask", paths["mask"]], dict(mask=mask)),
                                   ("spline", ["--subset-interpolation", "bspline"], dict(interpolation="bspline"))):
            q, files = run(base + options + ["--subset-uncertainty"], tmp_path / label)
            assert q.returncode == 0, q.stdout[-2000:]
            nodes, _, _, _ = flow.correlate_subset(scene.frame_0, scene.frame_1, PASSES, R, **kw)
            planes, rec = flow.node_uncertainty(scene.frame_0, scene.frame_1, nodes, 7, 8, R, **kw)
            for name, plane in planes.items():
                assert files["t_%s-%d-%d.raw" % (FILES[name], nw, nh)] == plane.tobytes(), (label, name)
            line = [x for x in q.stdout.splitlines() if x.startswith("SubsetUncertainty: ")]
            assert len(line) == 1 and q.stdout.splitlines()[-1] != "" and json.loads(line[0][19:]) == dict(radius=R, min_state=1, **rec.summary())
            assert rec.evaluated >= 40 and np.isfinite(planes["sigma_u"]).sum() == rec.evaluated
            if label == "pair":  # every other file and line is the plain run's
                assert {k: v for k, v in files.items() if "sigma" not in k and "rho" not in k and "noise" not in k} == plain_files
                assert [x for x in q.stdout.splitlines() if x.startswith("Subset: ")] == [x for x in plain.stdout.splitlines() if x.startswith("Subset: ")]
                assert q.stdout.splitlines().index(line[0]) > max(k for k, x in enumerate(q.stdout.splitlines()) if x.startswith("Subset: "))
    finally:
        flow.close()
    for bad in (base + ["--subset-uncertainty", "--subset-order", "2"], base + ["--subset-uncertainty", "--subset-base", str(tmp_path / "plain") + "/t_"],
                ["--correlation", "7", "--subset-uncertainty"]):
        q = subprocess.run([flow2d.CLI_PATH] + bad + [paths["f0"], paths["f1"], str(W), str(H), "t_"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=60)
        assert q.returncode == 5, (bad, q.stdout[-500:])
    # --subset-previous: the next step from the plain run's files, with its uncertainty
    q, files = run(base + ["--subset-previous", str(tmp_path / "plain") + "/t_", "--subset-uncertainty"], tmp_path / "next")
    assert q.returncode == 0 and len([x for x in q.stdout.splitlines() if x.startswith("SubsetUncertainty: ")]) == 1, q.stdout[-2000:]
    sigma = np.frombuffer(files["t_node-sigma-u-%d-%d.raw" % (nw, nh)], F32)
    state = np.frombuffer(files["t_node-state-%d-%d.raw" % (nw, nh)], F32)
    assert np.isfinite(sigma).sum() >= 40 and not np.isfinite(sigma[state < 1]).any()
