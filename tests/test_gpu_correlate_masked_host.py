"""The layers above flow2d_correlate_masked_2d and flow2d_validate_nodes_masked_2d on the device, on the specimen moved by
(6.4, -3.3) in front of a textured background: OpticalFlow.correlate_multipass_device with a mask against the restated chain of
masked passes (tests/test_correlate_masked_cpu.py) byte for byte, and its host-image form; correlate_subset_device with
mask_search=False against the calls there always were and with mask_search=True against its parts called by hand, the host-image
form and step 1 of a sequence; the refusals; and the CLI's --correlation-mask, --correlation-mask-invert, --correlation-min-pixels
and --subset-mask-search."""
import ctypes
import json
import subprocess

import numpy as np
import pytest

from test_correlate_cpu import F32, U32, bits, frame_range, grid
from test_correlate_masked_cpu import CLAIM_SCENE, claim_case, counts, default_min_pixels, masked_multipass_reference
from test_gpu_multipass import POISON, reference_bytes, report_bytes
from test_multipass_cpu import multipass_reference

pytestmark = pytest.mark.gpu
W, H, R = 96, 80, 7
CHAIN = ((15, 10, 16), (7, 3, 8))
FILES = dict(zip(("u", "v", "ux", "uy", "vx", "vy", "score", "state"),
                 ("node-u", "node-v", "node-ux", "node-uy", "node-vx", "node-vy", "node-score", "node-state")))


def moved_specimen(name="stretch"):
    """The scene, its mask, and lo and scale as OpticalFlow2D::CorrelationRange chooses them (the host-image forms')."""
    scene, mask, on, edge, tu, tv = claim_case(name, CLAIM_SCENE)
    lo, scale = frame_range(scene.frame_0, scene.frame_1)
    return scene, mask, lo, scale


@pytest.mark.parametrize("replace,validate_last,min_pixels", [(True, True, 0), (False, True, 40), (True, False, 0)])
def test_masked_chain_equals_the_restatement(flow2d, ctx, replace, validate_last, min_pixels):
    scene, mask, lo, scale = moved_specimen()
    cut = 0.1
    wu, wv, ws, wreports, (eu, ev) = masked_multipass_reference(scene.frame_0, scene.frame_1, lo, scale, CHAIN, mask, min_pixels, cut,
                                                                replace=replace, validate_last=validate_last)
    nw, nh = grid(W, H, CHAIN[-1][0], CHAIN[-1][2])
    f0, f1, pm = ctx.plane(W, H, scene.frame_0), ctx.plane(W, H, scene.frame_1), ctx.plane(W, H, mask)
    new = lambda: ctx.plane(W, H).fill_bytes(0x7F)  # noqa: E731
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        nu, nv, ns, fu, fv = (new() for _ in range(5))
        reports = flow.correlate_multipass_device(f0.ptr, f1.ptr, lo, scale, CHAIN, cut, replace=replace, validate_last=validate_last,
                                                  dev_nodes=(nu.ptr, nv.ptr), dev_score=ns.ptr, dev_flow=(fu.ptr, fv.ptr), mask=pm.ptr,
                                                  min_pixels=min_pixels)
        assert np.array_equal(nu.download(nw, nh).view(U32), bits(wu)) and np.array_equal(nv.download(nw, nh).view(U32), bits(wv))
        assert np.array_equal(ns.download(nw, nh).view(U32), bits(ws))
        assert np.array_equal(fu.download().view(U32), bits(eu)) and np.array_equal(fv.download().view(U32), bits(ev))
        assert (nu.download().view(U32)[nh:] == POISON).all() and (nu.download().view(U32)[:, nw:] == POISON).all()
        assert report_bytes(reports) == reference_bytes(wreports)
        print("masked chain:", json.dumps([dict(q.summary(), masked=(q.correlation.masked, q.validation.masked)) for q in reports]))
        assert all(q.correlation.masked > 0 for q in reports) and reports[0].validation.masked > 0
        assert reports[-1].correlation.masked == counts(wreports[-1][2])[6]
        if not validate_last:
            assert bytes(reports[-1].validation) == bytes(64)
        # without the mask: the chain it always was, other bytes
        gu, gv = new(), new()
        plain = flow.correlate_multipass_device(f0.ptr, f1.ptr, lo, scale, CHAIN, cut, replace=replace, validate_last=validate_last,
                                                dev_nodes=(gu.ptr, gv.ptr))
        xu, xv, _, xreports, _ = multipass_reference(scene.frame_0, scene.frame_1, lo, scale, CHAIN, cut, replace=replace, validate_last=validate_last)
        assert np.array_equal(gu.download(nw, nh).view(U32), bits(xu)) and report_bytes(plain) == reference_bytes(xreports)
        assert all(q.correlation.masked == 0 and q.validation.masked == 0 for q in plain) and not np.array_equal(bits(xu), bits(wu))
        # the host-image form uploads the mask itself
        if replace and validate_last:
            hu, hv, hs, hreports, (hlo, hscale), (qu, qv) = flow.correlate_multipass(scene.frame_0, scene.frame_1, CHAIN, cut, flow=True, mask=mask,
                                                                                    min_pixels=min_pixels)
            assert (F32(hlo), F32(hscale)) == (lo, scale)
            assert np.array_equal(bits(hu), bits(wu)) and np.array_equal(bits(hv), bits(wv)) and np.array_equal(bits(hs), bits(ws))
            assert np.array_equal(bits(qu), bits(eu)) and np.array_equal(bits(qv), bits(ev)) and report_bytes(hreports) == report_bytes(reports)
            # refusals: a min_pixels no window of the finest pass holds, one without a mask, a node plane that is the mask, a short image
            for bad in (dict(min_pixels=226), dict(min_pixels=-1)):
                with pytest.raises(flow2d.Flow2DError):
                    flow.correlate_multipass_device(f0.ptr, f1.ptr, lo, scale, CHAIN, mask=pm.ptr, **bad)
            with pytest.raises(flow2d.Flow2DError):
                flow.correlate_multipass_device(f0.ptr, f1.ptr, lo, scale, CHAIN, mask=pm.ptr, dev_nodes=(pm.ptr, nv.ptr))
            with pytest.raises(ValueError):
                flow.correlate_multipass_device(f0.ptr, f1.ptr, lo, scale, CHAIN, min_pixels=57)
            with pytest.raises(ValueError):
                flow.correlate_multipass(scene.frame_0, scene.frame_1, CHAIN, mask=mask[:-1])
            ok = flow2d.OpticalFlow.correlation_passes_ok
            assert ok(W, H, lo, scale, CHAIN, min_pixels=225) and not ok(W, H, lo, scale, CHAIN, min_pixels=226) and not ok(W, H, lo, scale, CHAIN, min_pixels=-1)
    finally:
        flow.close()


def test_mask_search_off_is_the_call_it_was_and_on_is_its_parts(flow2d, ctx):
    scene, mask, lo, scale = moved_specimen("rotation")
    passes = ((7, 10, 8),)
    r, _, s = passes[-1]
    nw, nh = grid(W, H, r, s)
    names = flow2d.OpticalFlow.SUBSET_PLANES
    f0, f1, pm = ctx.plane(W, H, scene.frame_0), ctx.plane(W, H, scene.frame_1), ctx.plane(W, H, mask)
    new = lambda: ctx.plane(W, H).fill_bytes(0x7F)  # noqa: E731
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        def chain(**kw):
            out = {name: new() for name in names}
            reports, rec = flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, passes, R, dev_out={n: q.ptr for n, q in out.items()},
                                                        mask=pm.ptr, **kw)
            return {n: q.download().tobytes() for n, q in out.items()}, reports, rec

        def by_hand(masked):
            """The passes (validated with replacement) into planes of the caller's, then the masked refinement of them."""
            su, sv = new(), new()
            reports = flow.correlate_multipass_device(f0.ptr, f1.ptr, lo, scale, passes, dev_nodes=(su.ptr, sv.ptr),
                                                      **(dict(mask=pm.ptr) if masked else {}))
            out = {name: new() for name in names}
            rec = flow.refine_nodes_device(f0.ptr, f1.ptr, su.ptr, sv.ptr, r, s, R, dev_out={n: q.ptr for n, q in out.items()}, mask=pm.ptr)
            return {n: q.download().tobytes() for n, q in out.items()}, reports, rec

        default, dreports, drec = chain()
        off, oreports, orec = chain(mask_search=False)
        hand, hreports, hrec = by_hand(False)
        assert default == off == hand and bytes(drec) == bytes(orec) == bytes(hrec) and report_bytes(dreports) == report_bytes(oreports) == report_bytes(hreports)
        assert dreports[0].correlation.masked == 0
        on, nreports, nrec = chain(mask_search=True)
        hand, hreports, hrec = by_hand(True)
        assert on == hand and bytes(nrec) == bytes(hrec) and report_bytes(nreports) == report_bytes(hreports)
        assert nreports[0].correlation.masked > 0 and nreports[0].validation.masked > 0 and on != off
        print("converged: mask_search off %d, on %d of %d nodes, %d masked" % (orec.converged, nrec.converged, nrec.nodes, nrec.masked))
        assert nrec.converged > orec.converged and nrec.masked == orec.masked  # the edge nodes the background's motion had taken
        # the flag does not outlive its call
        again, _, arec = chain()
        assert again == off and bytes(arec) == bytes(orec)
        # the host-image form, and step 1 of a sequence
        nodes, preports, prec, (hlo, hscale) = flow.correlate_subset(scene.frame_0, scene.frame_1, passes, R, mask=mask, mask_search=True)
        assert (F32(hlo), F32(hscale)) == (lo, scale)
        pitch = len(on["u"]) // (4 * H)  # (the planes were downloaded whole: H rows of the container's pitch)
        assert all(nodes[n].tobytes() == np.frombuffer(on[n], F32).reshape(H, pitch)[:nh, :nw].tobytes() for n in names)
        assert preports[0].correlation.masked == nreports[0].correlation.masked and prec.masked == nrec.masked
        per_step, sreports, _, _ = flow.correlate_subset_sequence([scene.frame_0, scene.frame_1], passes, R, mask=mask, mask_search=True)
        assert all(per_step[0][n].tobytes() == nodes[n].tobytes() for n in names) and report_bytes(sreports) == report_bytes(preports)
        # mask_search without a mask is refused, by the method and by SubsetOptionsOk
        with pytest.raises(flow2d.Flow2DError):
            flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, passes, R, mask_search=True)
        with pytest.raises(flow2d.Flow2DError):
            flow.correlate_subset(scene.frame_0, scene.frame_1, passes, R, mask_search=True)
        with_mask = flow2d.SubsetOptions(R, 20, 1e-3, 2.0, 0.5, 1, 0.05, 0, 1)
        without = flow2d.SubsetOptions(R, 20, 1e-3, 2.0, 0.5, 1, 0.05, 0, None)
        lib = flow2d.host_lib()
        assert lib.flow2d_host_subset_mask_search_ok(ctypes.byref(with_mask)) == 1
        assert lib.flow2d_host_subset_mask_search_ok(ctypes.byref(without)) == 0
        assert lib.flow2d_host_set_subset_mask_search(flow.handle, 2) == 1 and lib.flow2d_host_set_subset_mask_search(None, 1) == 1
    finally:
        flow.close()


def test_cli_correlation_mask(flow2d, ctx, tmp_path):
    """--correlation-mask FILE and --correlation-mask-invert with the region image give the same files, those of
    OpticalFlow.correlate_multipass with the mask, and one "CorrelationMask:" line behind the "CorrelationPasses:" line;
    --subset-mask-search gives the files of correlate_subset(mask_search=True); without the options no byte changes; each option
    without its partner is a usage error."""
    scene, mask, lo, scale = moved_specimen()
    paths = {}
    region = np.where(mask == 0, F32(255), F32(0))  # non-zero = inside
    for name, image in (("f0", scene.frame_0), ("f1", scene.frame_1), ("mask", mask), ("region", region)):
        paths[name] = str(tmp_path / (name + ".raw"))
        image.astype(F32).tofile(paths[name])
    spec = ",".join("%d:%d:%d" % p for p in CHAIN)
    base = ["--correlation-passes", spec]

    def run(options, out):
        out.mkdir()
        q = subprocess.run([flow2d.CLI_PATH, "--flo"] + options + [paths["f0"], paths["f1"], str(W), str(H), "t_", str(out) + "/"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        return q, {f.name: f.read_bytes() for f in out.iterdir()}

    def printed(q, key):
        line = [x for x in q.stdout.splitlines() if x.startswith(key + ": ")]
        assert len(line) == 1, q.stdout[-2000:]
        return json.loads(line[0][len(key) + 2:])

    nw, nh = grid(W, H, CHAIN[-1][0], CHAIN[-1][2])
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        nu, nv, ns, reports, _, (fu, fv) = flow.correlate_multipass(scene.frame_0, scene.frame_1, CHAIN, flow=True, mask=mask)
        mu, mv, _, more, _ = flow.correlate_multipass(scene.frame_0, scene.frame_1, CHAIN, mask=mask, min_pixels=70)
        pu, pv, _, _, _ = flow.correlate_multipass(scene.frame_0, scene.frame_1, CHAIN)
        nodes, sreports, srec, _ = flow.correlate_subset(scene.frame_0, scene.frame_1, CHAIN, R, mask=mask, mask_search=True)
    finally:
        flow.close()
    q1, files1 = run(base + ["--correlation-mask", paths["mask"]], tmp_path / "masked")
    q2, files2 = run(base + ["--correlation-mask", paths["region"], "--correlation-mask-invert"], tmp_path / "inverted")
    assert q1.returncode == 0 and q2.returncode == 0, q1.stdout[-2000:] + q2.stdout[-2000:]
    assert files1 == files2
    assert files1["t_node-u-%d-%d.raw" % (nw, nh)] == nu.tobytes() and files1["t_node-v-%d-%d.raw" % (nw, nh)] == nv.tobytes()
    assert files1["t_node-score-%d-%d.raw" % (nw, nh)] == ns.tobytes() and files1["t_flow-u-96-80.raw"] == fu.tobytes()
    for q in (q1, q2):
        line = printed(q, "CorrelationMask")
        assert line == {"min_pixels": 0, "passes": [{"min_pixels": default_min_pixels(p[0]), "masked": r_.correlation.masked,
                                                     "validation_masked": r_.validation.masked} for p, r_ in zip(CHAIN, reports)]}
        assert printed(q, "CorrelationPasses")["passes"][0]["correlation"] == reports[0].correlation.summary()
        assert q.stdout.index("CorrelationPasses: ") < q.stdout.index("CorrelationMask: ")
    assert reports[-1].correlation.masked > 0
    q3, files3 = run(base + ["--correlation-mask", paths["mask"], "--correlation-min-pixels", "70"], tmp_path / "more_pixels")
    line = printed(q3, "CorrelationMask")
    assert q3.returncode == 0 and line["min_pixels"] == 70 and [p["min_pixels"] for p in line["passes"]] == [70, 70]
    assert line["passes"][-1]["masked"] == more[-1].correlation.masked >= reports[-1].correlation.masked
    assert files3["t_node-u-%d-%d.raw" % (nw, nh)] == mu.tobytes()
    # without the options: the run it always was
    q4, files4 = run(base, tmp_path / "plain")
    assert q4.returncode == 0 and "CorrelationMask" not in q4.stdout and sorted(files4) == sorted(files1)
    assert files4["t_node-u-%d-%d.raw" % (nw, nh)] == pu.tobytes() and files4["t_node-v-%d-%d.raw" % (nw, nh)] == pv.tobytes()
    # --subset-mask-search
    refine = base + ["--subset-refine", str(R), "--subset-mask", paths["mask"]]
    q5, files5 = run(refine + ["--subset-mask-search"], tmp_path / "searched")
    assert q5.returncode == 0, q5.stdout[-2000:]
    for name, plane in nodes.items():
        assert files5["t_%s-%d-%d.raw" % (FILES[name], nw, nh)] == plane.tobytes(), name
    line = printed(q5, "CorrelationMask")
    assert [p["masked"] for p in line["passes"]] == [r_.correlation.masked for r_ in sreports] and printed(q5, "SubsetMask")["masked"] == srec.masked
    assert q5.stdout.index("CorrelationMask: ") < q5.stdout.index("SubsetMask: ")
    q6, files6 = run(refine, tmp_path / "not_searched")
    assert q6.returncode == 0 and "CorrelationMask" not in q6.stdout and files6["t_node-u-%d-%d.raw" % (nw, nh)] != files5["t_node-u-%d-%d.raw" % (nw, nh)]
    for bad in (base + ["--correlation-mask-invert"], base + ["--correlation-min-pixels", "57"],
                ["--correlation-mask", paths["mask"]], ["--correlation", "7", "--correlation-mask", paths["mask"]],
                base + ["--correlation-mask", paths["mask"], "--correlation-min-pixels", "0"],
                base + ["--correlation-mask", paths["mask"], "--correlation-min-pixels", "x"],
                refine + ["--correlation-mask", paths["mask"]], base + ["--subset-refine", str(R), "--subset-mask-search"],
                base + ["--subset-mask-search"]):
        q = subprocess.run([flow2d.CLI_PATH] + bad + [paths["f0"], paths["f1"], str(W), str(H), "t_"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=60)
        assert q.returncode == 5, (bad, q.stdout[-500:])
    # a min_pixels the finest window cannot hold is refused by the host layer, a missing file by the loader
    q = subprocess.run([flow2d.CLI_PATH] + base + ["--correlation-mask", paths["mask"], "--correlation-min-pixels", "226", paths["f0"], paths["f1"],
                                                   str(W), str(H), "t_", str(tmp_path) + "/"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=60)
    assert q.returncode == 4, q.stdout[-500:]
    q = subprocess.run([flow2d.CLI_PATH] + base + ["--correlation-mask", str(tmp_path / "missing.raw"), paths["f0"], paths["f1"], str(W), str(H), "t_"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert q.returncode == 2, q.stdout[-500:]
