"""The layers above flow2d_subset_refine_masked_2d on the device: OpticalFlow.correlate_subset_device with a mask against the
restated chain (search, validation with replacement, masked refinement: tests/test_subset_masked_cpu.py) byte for byte, its
host-image form and refine_nodes[_from]_device; three steps of the rotation sequence under a random mask through
correlate_subset_sequence_device against the restated chain -- a masked node comes out of the prediction predicted and goes back
to masked --; node_strain after a masked run; the refusals; and the CLI's --subset-mask, --subset-mask-invert and
--subset-min-pixels."""
import json
import subprocess

import numpy as np
import pytest

from test_correlate_cpu import F32, bits, frame_range, grid
from test_multipass_cpu import multipass_reference
from test_node_strain_cpu import node_strain_reference
from test_subset_cpu import Refined
from test_subset_masked_cpu import MASKED, SPECIMEN, random_mask, specimen_case, subset_refine_masked_reference, usable_counts
from test_subset_sequence_cpu import PLANES, predict_passes, rotation_scenes

pytestmark = pytest.mark.gpu
W, H, R = SPECIMEN["width"], SPECIMEN["height"], SPECIMEN["R"]
PASSES = ((SPECIMEN["r"], SPECIMEN["d"], SPECIMEN["s"]),)
MIN_PIXELS = SPECIMEN["min_pixels"]
FILES = dict(zip(Refined.NAMES, ("node-u", "node-v", "node-ux", "node-uy", "node-vx", "node-vy", "node-score", "node-state")))


def same_planes(got, want, what):
    """got: {name: [nh, nw] array}; want: a Refined.  Byte for byte; prints the words that differ first."""
    differ = {name: int((bits(got[name]) != bits(getattr(want, name))).sum()) for name in Refined.NAMES}
    print("%s: words that differ %s" % (what, differ))
    assert not any(differ.values()), "%s: %s" % (what, differ)


def same_record(rec, want, what):
    assert bytes(rec) == want.record.tobytes(), "%s: record %s, want %s" % (what, rec.summary(), want.record)


def test_the_masked_chain_and_strain(flow2d, ctx):
    scene, mask, u0, v0 = specimen_case("stretch")
    lo, scale = frame_range(scene.frame_0, scene.frame_1)
    r, _, s = PASSES[-1]
    nw, nh = grid(W, H, r, s)
    names = flow2d.OpticalFlow.SUBSET_PLANES
    want = subset_refine_masked_reference(scene.frame_0, scene.frame_1, u0, v0, None, mask, MIN_PIXELS, r, s, R, max_shift=2.0)
    f0, f1, pm = ctx.plane(W, H, scene.frame_0), ctx.plane(W, H, scene.frame_1), ctx.plane(W, H, mask)
    new = lambda: ctx.plane(W, H).fill_bytes(0x7F)  # noqa: E731
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        out = {name: new() for name in names}
        _, rec = flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, PASSES, R, dev_out={n: q.ptr for n, q in out.items()}, mask=pm.ptr,
                                              min_pixels=MIN_PIXELS)
        same_planes({n: q.download(nw, nh) for n, q in out.items()}, want, "correlate_subset_device")
        same_record(rec, want, "correlate_subset_device")
        assert rec.masked == 55 and rec.converged == 44 and rec.summary()["nodes"] == 99
        # min_pixels 0: the default, a quarter of the subset -- 57 at R = 7
        again = {name: new() for name in names}
        _, rec0 = flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, PASSES, R, dev_out={n: q.ptr for n, q in again.items()}, mask=pm.ptr)
        assert bytes(rec0) == bytes(rec) and all(again[n].download().tobytes() == out[n].download().tobytes() for n in names)
        # ... and without the keyword the call it always was: no masked node, other bytes
        _, plain = flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, PASSES, R, dev_out={n: q.ptr for n, q in again.items()})
        assert plain.masked == 0 and plain.nodes == 99 and again["u"].download().tobytes() != out["u"].download().tobytes()
        # the host-image form uploads the mask itself
        nodes, _, prec, _ = flow.correlate_subset(scene.frame_0, scene.frame_1, PASSES, R, mask=mask, min_pixels=MIN_PIXELS)
        same_planes(nodes, want, "correlate_subset")
        same_record(prec, want, "correlate_subset")
        # refine_nodes_device and refine_nodes_from_device from the restated start
        start = [ctx.plane(W, H, np.pad(q, ((0, H - nh), (0, W - nw)))) for q in (u0, v0)]
        rec2 = flow.refine_nodes_device(f0.ptr, f1.ptr, start[0].ptr, start[1].ptr, r, s, R, dev_out={n: q.ptr for n, q in again.items()},
                                        mask=pm.ptr, min_pixels=MIN_PIXELS)
        same_planes({n: q.download(nw, nh) for n, q in again.items()}, want, "refine_nodes_device")
        same_record(rec2, want, "refine_nodes_device")
        second, _, _ = predict_passes([getattr(want, n) for n in PLANES], want.state, s, 2)
        want2 = subset_refine_masked_reference(scene.frame_0, scene.frame_1, second[0], second[1], second[2:], mask, MIN_PIXELS, r, s, R)
        dev_start = [ctx.plane(W, H, np.pad(q, ((0, H - nh), (0, W - nw)))) for q in second]
        rec3 = flow.refine_nodes_from_device(f0.ptr, f1.ptr, {n: q.ptr for n, q in zip(names[:6], dev_start)}, r, s, R,
                                             dev_out={n: q.ptr for n, q in again.items()}, mask=pm.ptr, min_pixels=MIN_PIXELS)
        same_planes({n: q.download(nw, nh) for n, q in again.items()}, want2, "refine_nodes_from_device")
        same_record(rec3, want2, "refine_nodes_from_device")
        assert np.array_equal(want2.state == MASKED, want.state == MASKED)
        # strain on the node grid: state -4 is below min_state, so masked nodes drop out of every window and have no strain
        for window in (0, 2):
            planes, _ = flow.node_strain(nodes, s, window=window)
            ref = node_strain_reference(want.u, want.v, want.state, [want.ux, want.uy, want.vx, want.vy], s, window)
            for name, plane in planes.items():
                assert np.array_equal(bits(plane), bits(ref[name])), (window, name)
                assert np.isnan(plane[want.state == MASKED]).all() and np.isfinite(plane[want.state >= 1]).sum() >= (44 if window == 0 else 20)
        # refusals: a mask with order 2, a min_pixels outside its limits, an output plane that is the mask
        ok = {n: q.ptr for n, q in out.items()}
        for bad in (dict(order=2), dict(min_pixels=5), dict(min_pixels=226), dict(dev_out=dict(ok, u=pm.ptr))):
            with pytest.raises(flow2d.Flow2DError):
                flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, PASSES, R, **dict(dict(dev_out=ok, mask=pm.ptr), **bad))
        with pytest.raises(flow2d.Flow2DError):
            flow.correlate_subset(scene.frame_0, scene.frame_1, PASSES, R, mask=mask, order=2)
        with pytest.raises(ValueError):
            flow.correlate_subset(scene.frame_0, scene.frame_1, PASSES, R, mask=mask[:-1])
        with pytest.raises(ValueError):
            flow.correlate_subset(scene.frame_0, scene.frame_1, PASSES, R, min_pixels=57)
        # ... after which the object has no mask left
        _, after = flow.correlate_subset_device(f0.ptr, f1.ptr, lo, scale, PASSES, R)
        assert bytes(after) == bytes(plain)
    finally:
        flow.close()


def test_a_sequence_under_a_random_mask(flow2d, ctx):
    """Three steps of the rotation sequence (4 degrees per step) with 30 % of the pixels excluded at random and min_pixels 20: every
    step's planes and records are the restated chain's, and the nodes the mask takes are the same in every step."""
    steps = 3
    scenes = rotation_scenes()[:steps]
    frames = [scenes[0].frame_0] + [sc.frame_1 for sc in scenes]
    mask = random_mask((H, W), 0.3, seed=12)
    r, _, s = PASSES[-1]
    nw, nh = grid(W, H, r, s)
    lo, scale = frame_range(frames[0], frames[1])
    u0, v0, _, _, _ = multipass_reference(frames[0], frames[1], lo, scale, list(PASSES), replace=True, validate_last=True)
    want = [subset_refine_masked_reference(frames[0], frames[1], u0, v0, None, mask, 20, r, s, R, max_shift=2.0)]
    for k in range(1, steps):
        nodes, state, _ = predict_passes([getattr(want[-1], n) for n in PLANES], want[-1].state, s, 2)
        taken = want[-1].state == MASKED
        assert (state[taken] != MASKED).any()  # the prediction refills masked nodes ...
        want.append(subset_refine_masked_reference(frames[0], frames[k + 1], nodes[0], nodes[1], nodes[2:], mask, 20, r, s, R, max_shift=4.0))
        assert np.array_equal(want[-1].state == MASKED, taken)  # ... and the refinement masks them again
    nv = usable_counts(mask, nw, nh, r, s, R)
    cy, cx = r + np.arange(nh) * s, r + np.arange(nw) * s
    assert np.array_equal(want[0].state == MASKED, (mask[np.ix_(cy, cx)] >= 0.5) | (nv < 20)) and 20 <= (want[0].state == MASKED).sum() <= 60
    names = flow2d.OpticalFlow.SUBSET_PLANES
    dev, pm = [ctx.plane(W, H, f) for f in frames], ctx.plane(W, H, mask)
    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        out = [{name: ctx.plane(W, H).fill_bytes(0x7F) for name in names} for _ in range(steps)]
        _, reports = flow.correlate_subset_sequence_device([q.ptr for q in dev], lo, scale, PASSES, R,
                                                           [{n: q.ptr for n, q in step.items()} for step in out], mask=pm.ptr, min_pixels=20)
        for k in range(steps):
            same_planes({n: q.download(nw, nh) for n, q in out[k].items()}, want[k], "step %d" % (k + 1))
            same_record(reports[k].subset, want[k], "step %d" % (k + 1))
            print("step %d:" % (k + 1), json.dumps(reports[k].summary(2)), "masked", reports[k].subset.masked)
        # the host-image form
        per_step, _, preports, _ = flow.correlate_subset_sequence(frames, PASSES, R, mask=mask, min_pixels=20)
        for k in range(steps):
            same_planes(per_step[k], want[k], "host images, step %d" % (k + 1))
            assert bytes(preports[k]) == bytes(reports[k])
        with pytest.raises(flow2d.Flow2DError):
            flow.correlate_subset_sequence(frames, PASSES, R, mask=mask, order=2)
    finally:
        flow.close()


def test_cli_subset_mask(flow2d, ctx, tmp_path):
    """--subset-mask FILE and --subset-mask-invert with the region image give the same files, those of OpticalFlow.correlate_subset
    with the mask; one "SubsetMask:" line; without the option no byte changes; order 2 and the options alone are usage errors."""
    scene, mask, _, _ = specimen_case("stretch")
    paths = {}
    region = np.where(mask == 0, F32(255), F32(0))  # non-zero = inside
    for name, image in (("f0", scene.frame_0), ("f1", scene.frame_1), ("mask", mask), ("region", region)):
        paths[name] = str(tmp_path / (name + ".raw"))
        image.astype(F32).tofile(paths[name])
    base = ["--correlation", "7", "--correlation-range", "6", "--subset-refine", str(R)]

    def run(options, out):
        out.mkdir()
        q = subprocess.run([flow2d.CLI_PATH, "--flo"] + options + [paths["f0"], paths["f1"], str(W), str(H), "t_", str(out) + "/"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        return q, {f.name: f.read_bytes() for f in out.iterdir()}

    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        nodes, _, rec, _ = flow.correlate_subset(scene.frame_0, scene.frame_1, PASSES, R, mask=mask)
        plain_nodes, _, _, _ = flow.correlate_subset(scene.frame_0, scene.frame_1, PASSES, R)
    finally:
        flow.close()
    nw, nh = grid(W, H, 7, 8)
    q1, files1 = run(base + ["--subset-mask", paths["mask"]], tmp_path / "masked")
    q2, files2 = run(base + ["--subset-mask", paths["region"], "--subset-mask-invert"], tmp_path / "inverted")
    assert q1.returncode == 0 and q2.returncode == 0, q1.stdout[-2000:] + q2.stdout[-2000:]
    assert files1 == files2 and len(files1) >= 8
    for name, plane in nodes.items():
        assert files1["t_%s-%d-%d.raw" % (FILES[name], nw, nh)] == plane.tobytes(), name
    for q in (q1, q2):
        line = [x for x in q.stdout.splitlines() if x.startswith("SubsetMask: ")]
        assert len(line) == 1 and json.loads(line[0][12:]) == {"masked": rec.masked, "min_pixels": 57}, q.stdout[-2000:]
    assert rec.masked == 55
    q3, files3 = run(base + ["--subset-mask", paths["mask"], "--subset-min-pixels", "150"], tmp_path / "more_pixels")
    line = [x for x in q3.stdout.splitlines() if x.startswith("SubsetMask: ")]
    assert q3.returncode == 0 and json.loads(line[0][12:])["min_pixels"] == 150 and json.loads(line[0][12:])["masked"] > 55
    # without the option: the run it always was
    q4, files4 = run(base, tmp_path / "plain")
    assert q4.returncode == 0 and "SubsetMask" not in q4.stdout and sorted(files4) == sorted(files1)
    for name, plane in plain_nodes.items():
        assert files4["t_%s-%d-%d.raw" % (FILES[name], nw, nh)] == plane.tobytes(), name
    for bad in (base + ["--subset-mask", paths["mask"], "--subset-order", "2"], base + ["--subset-mask-invert"], base + ["--subset-min-pixels", "57"],
                ["--correlation", "7", "--subset-mask", paths["mask"]], base + ["--subset-mask", paths["mask"], "--subset-min-pixels", "5"]):
        q = subprocess.run([flow2d.CLI_PATH] + bad + [paths["f0"], paths["f1"], str(W), str(H), "t_"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=60)
        assert q.returncode == 5, (bad, q.stdout[-500:])
    q = subprocess.run([flow2d.CLI_PATH] + base + ["--subset-mask", str(tmp_path / "missing.raw"), paths["f0"], paths["f1"], str(W), str(H), "t_"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert q.returncode == 2, q.stdout[-500:]
