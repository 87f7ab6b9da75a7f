"""The layers above flow2d_subset_refine_spline_2d and flow2d_subset_refine2_spline_2d on the device: OpticalFlow.refine_nodes_device,
correlate_subset_device and a three-step correlate_subset_sequence_device with interpolation="bspline" -- at order 1, at order 1 under
a mask and at order 2 -- against the chain assembled by hand from Context.bspline_prefilter, predict_nodes and the spline entry on
the same starts, byte for byte; the same call with the default afterwards gives the bytes it gave before; the setter on a real
object; and the CLI's --subset-interpolation."""
import json
import subprocess

import numpy as np
import pytest

from test_correlate_cpu import F32, U32, frame_range, grid
from test_gpu_multipass import POISON
from test_multipass_cpu import multipass_reference
from test_subset2_cpu import CURVATURES
from test_subset_cpu import Refined
from test_subset_masked_cpu import random_mask
from test_subset_sequence_cpu import ROTATION, rotation_scenes

pytestmark = pytest.mark.gpu
W, H, R = ROTATION["width"], ROTATION["height"], ROTATION["R"]
PASSES = ((7, 6, 8),)
STEPS = 3
FILES = dict(zip(Refined.NAMES, ("node-u", "node-v", "node-ux", "node-uy", "node-vx", "node-vy", "node-score", "node-state")))
VARIANTS = {"order 1": dict(order=1, mask=False), "order 1, masked": dict(order=1, mask=True), "order 2": dict(order=2, mask=False)}
_made = {}


def sequence_case():
    """Three steps of the rotation sequence, the range of the first pair and the restated chain's start of step 1 (search at d = 6,
    validation with replacement), made once."""
    if not _made:
        scenes = rotation_scenes()[:STEPS]
        frames = [scenes[0].frame_0] + [q.frame_1 for q in scenes]
        lo, scale = frame_range(frames[0], frames[1])
        u0, v0, _, _, _ = multipass_reference(frames[0], frames[1], lo, scale, list(PASSES), replace=True, validate_last=True)
        _made["case"] = (frames, lo, scale, u0, v0)
    return _made["case"]


def grids(planes, nw, nh):
    """The node grids of a dict of container planes as bits; nothing beyond a grid was written."""
    out = {}
    for name, q in planes.items():
        got = q.download().view(U32)
        assert (got[nh:] == POISON).all() and (got[:, nw:] == POISON).all(), name
        out[name] = got[:nh, :nw].copy()
    return out


def same(a, b, what):
    differ = {name: int((a[name] != b[name]).sum()) for name in a}
    print("%s: words that differ %s" % (what, differ))
    assert not any(differ.values()), "%s: %s" % (what, differ)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_the_host_calls_equal_the_chain_by_hand(flow2d, ctx, variant):
    order, masked = VARIANTS[variant]["order"], VARIANTS[variant]["mask"]
    frames, lo, scale, u0, v0 = sequence_case()
    r, _, s = PASSES[-1]
    nw, nh = grid(W, H, r, s)
    names = flow2d.OpticalFlow.SUBSET_PLANES if order == 1 else flow2d.OpticalFlow.SUBSET2_PLANES
    dev = [ctx.plane(W, H, f) for f in frames]
    pm = ctx.plane(W, H, random_mask((H, W), 0.3, seed=12)) if masked else None
    start = [ctx.plane(W, H, np.pad(q, ((0, H - nh), (0, W - nw)))) for q in (u0, v0)]
    new = lambda: ctx.plane(W, H).fill_bytes(0x7F)  # noqa: E731
    ptrs = lambda planes: {n: q.ptr for n, q in planes.items()}  # noqa: E731
    kw = dict(order=order, **(dict(mask=pm.ptr, min_pixels=20) if masked else {}))

    def by_hand(k, su, sv, gradients, max_shift, out):
        """Step k (frame k against frame 0) from the start (su, sv, gradients or None) into `out`; returns the record's bytes."""
        coeff = ctx.bspline_prefilter(dev[k], W, H)
        record = ctx.subset_records().fill_bytes(0x7F)
        if order == 1:
            ctx.subset_refine_spline(dev[0], coeff, W, H, su, sv, gradients, nw, nh, r, s, R, pm, 20 if masked else None, 20, 1e-3, max_shift, 0.5,
                                     out["u"], out["v"], [out[n] for n in names[2:6]], out["score"], out["state"], record)
        else:
            ctx.subset_refine2_spline(dev[0], coeff, W, H, su, sv, nw, nh, r, s, R, max_shift=max_shift, start_gradients=gradients, out_u=out["u"],
                                      out_v=out["v"], out_gradients=[out[n] for n in names[2:6]], out_curvatures=[out[n] for n in CURVATURES],
                                      out_score=out["score"], out_state=out["state"], record=record)
        ctx.synchronize()
        return record.download(16, 1).tobytes()

    flow = flow2d.OpticalFlow(W, H, flow2d.GREY, ctx=ctx)
    try:
        host = flow2d.host_lib()
        assert host.flow2d_host_set_subset_interpolation(flow.handle, 2) == 1 and host.flow2d_host_set_subset_interpolation(flow.handle, -1) == 1
        # ---- refine_nodes_device: the default before, the spline, the default afterwards
        hand = {n: new() for n in names}
        hand_record = by_hand(1, start[0], start[1], None, 2.0, hand)
        out = {n: new() for n in names}
        refine = lambda **more: flow.refine_nodes_device(dev[0].ptr, dev[1].ptr, start[0].ptr, start[1].ptr, r, s, R, dev_out=ptrs(out), **kw, **more)  # noqa: E731
        before_record, before = bytes(refine()), grids(out, nw, nh)
        rec = refine(interpolation="bspline")
        spline = grids(out, nw, nh)
        same(spline, grids(hand, nw, nh), "refine_nodes_device, %s" % variant)
        assert bytes(rec) == hand_record and rec.converged >= 20
        assert (spline["u"] != before["u"]).any()
        assert bytes(refine()) == before_record
        same(grids(out, nw, nh), before, "refine_nodes_device with the default afterwards, %s" % variant)
        # ---- correlate_subset_device: the same starts, found by the search
        chain = lambda **more: flow.correlate_subset_device(dev[0].ptr, dev[1].ptr, lo, scale, PASSES, R, dev_out=ptrs(out), **kw, **more)[1]  # noqa: E731
        chain_before_record, chain_before = bytes(chain()), grids(out, nw, nh)
        same(chain_before, before, "the chain's starts are the restated ones, %s" % variant)
        rec = chain(interpolation="bspline")
        same(grids(out, nw, nh), grids(hand, nw, nh), "correlate_subset_device, %s" % variant)
        assert bytes(rec) == hand_record
        assert bytes(chain()) == chain_before_record
        same(grids(out, nw, nh), before, "correlate_subset_device with the default afterwards, %s" % variant)
        # ---- three steps of correlate_subset_sequence_device: every step prefilters its own frame
        outs = [{n: new() for n in names} for _ in range(STEPS)]
        sequence = lambda **more: flow.correlate_subset_sequence_device([q.ptr for q in dev], lo, scale, PASSES, R, [ptrs(q) for q in outs],  # noqa: E731
                                                                        **kw, **more)[1]
        sequence_before_records = [bytes(q) for q in sequence()]
        sequence_before = [grids(q, nw, nh) for q in outs]
        steps = sequence(interpolation="bspline")
        hands, records = [hand], [hand_record]
        for k in range(1, STEPS):
            last = hands[-1]
            ping, pong = [new() for _ in range(7)], [new() for _ in range(7)]
            ctx.predict_nodes([last[n] for n in names[:6]], last["state"], nw, nh, s, 1, 1, ping[:6], ping[6], None)
            ctx.predict_nodes(ping[:6], ping[6], nw, nh, s, 1, 1, pong[:6], pong[6], None)
            hands.append({n: new() for n in names})
            records.append(by_hand(k + 1, pong[0], pong[1], pong[2:6], 4.0, hands[-1]))
        for k in range(STEPS):
            same(grids(outs[k], nw, nh), grids(hands[k], nw, nh), "sequence step %d, %s" % (k + 1, variant))
            assert bytes(steps[k].subset) == records[k], "record of step %d" % (k + 1)
            assert steps[k].subset.converged >= 10
        assert [bytes(q) for q in sequence()] == sequence_before_records
        for k in range(STEPS):
            same(grids(outs[k], nw, nh), sequence_before[k], "sequence step %d with the default afterwards, %s" % (k + 1, variant))
        # the host-image forms follow: the nodes of the device form
        nodes = flow.correlate_subset(frames[0], frames[1], PASSES, R, interpolation="bspline", order=order,
                                      **(dict(mask=random_mask((H, W), 0.3, seed=12), min_pixels=20) if masked else {}))[0]
        same({n: nodes[n].view(U32) for n in names}, grids(hand, nw, nh), "correlate_subset, %s" % variant)
        with pytest.raises(ValueError):
            refine(interpolation="quintic")
    finally:
        flow.close()


def test_cli_subset_interpolation(flow2d, ctx, tmp_path):
    """--subset-interpolation bspline gives the files of OpticalFlow.correlate_subset(interpolation="bspline") and one
    "SubsetInterpolation:" line; without the option the line is absent and no byte changes; catmull-rom spelled out gives the plain
    run's files; the option without --subset-refine and an unknown kind are usage errors."""
    frames, _, _, _, _ = sequence_case()
    paths = {}
    for name, image in (("f0", frames[0]), ("f1", frames[1])):
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
        nodes = flow.correlate_subset(frames[0], frames[1], PASSES, R, interpolation="bspline")[0]
        nodes2 = flow.correlate_subset(frames[0], frames[1], PASSES, R, interpolation="bspline", order=2)[0]
        plain = flow.correlate_subset(frames[0], frames[1], PASSES, R)[0]
    finally:
        flow.close()
    nw, nh = grid(W, H, 7, 8)
    lines = lambda q: [x for x in q.stdout.splitlines() if x.startswith("SubsetInterpolation: ")]  # noqa: E731
    q1, files1 = run(base + ["--subset-interpolation", "bspline"], tmp_path / "bspline")
    assert q1.returncode == 0, q1.stdout[-2000:]
    assert len(lines(q1)) == 1 and json.loads(lines(q1)[0][21:]) == {"interpolation": "bspline", "horizon": 16}
    for name, plane in nodes.items():
        assert files1["t_%s-%d-%d.raw" % (FILES[name], nw, nh)] == plane.tobytes(), name
    q2, files2 = run(base + ["--subset-interpolation", "bspline", "--subset-order", "2"], tmp_path / "bspline2")
    assert q2.returncode == 0 and len(lines(q2)) == 1, q2.stdout[-2000:]
    for name in Refined.NAMES:
        assert files2["t_%s-%d-%d.raw" % (FILES[name], nw, nh)] == nodes2[name].tobytes(), name
    q3, files3 = run(base, tmp_path / "plain")
    assert q3.returncode == 0 and "SubsetInterpolation" not in q3.stdout and sorted(files3) == sorted(files1)
    for name, plane in plain.items():
        assert files3["t_%s-%d-%d.raw" % (FILES[name], nw, nh)] == plane.tobytes(), name
    assert files3 != files1
    q4, files4 = run(base + ["--subset-interpolation", "catmull-rom"], tmp_path / "spelled_out")
    assert q4.returncode == 0 and files4 == files3 and json.loads(lines(q4)[0][21:]) == {"interpolation": "catmull-rom"}
    for bad in (["--correlation", "7", "--subset-interpolation", "bspline"], base + ["--subset-interpolation", "quintic"],
                base + ["--subset-interpolation"]):
        q = subprocess.run([flow2d.CLI_PATH] + bad + [paths["f0"], paths["f1"], str(W), str(H), "t_"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=60)
        assert q.returncode == 5, (bad, q.stdout[-500:])
