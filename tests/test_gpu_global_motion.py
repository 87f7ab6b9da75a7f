"""Global motion and stabilisation on the MI355X: flow2d_global_motion_2d against the numpy restatement of its definition
(tests/test_global_motion_cpu.py) within the tolerance measured there, identical bytes from repeated calls, a replayed graph and
an instance alone or in a lock-step batch; flow2d_global_flow_2d and flow2d_warp_global_2d bit for bit against their
restatements fed with the GPU's own record; the refusals on a real context; OpticalFlow.stabilise_sequence_device against its
parts, its device memory for a long and a short sequence, the CLI's --global-motion against the Python path and the results
table's GPU rows against its numpy rows."""
import ctypes
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_global_motion_cpu import (AFFINE, FITS, GPU_TOLERANCE, GPU_WEIGHT_RTOL, MASK_MODES, MODELS, SIMILARITY, SMALL_SHAPES,
                                    TRANSLATION, compose_motion, fit_case, global_flow_reference, global_motion_reference,
                                    warp_global_reference)
from test_gpu_batch_kernels import Tall, pitch_of, stride_of
from test_gpu_denoise import CLI_PARAMS, POISON, assert_same, run_cli, scenes_module
from test_oracle import rub_pair

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_record(got, want, what):
    print("%s: max |dp| %.3g (tolerance %.3g), weight_sum %.17g / %.17g" %
          (what, np.abs(got.parameters - want["p"]).max(), GPU_TOLERANCE, got.weight_sum, want["weight_sum"]))
    assert got.model_used == want["model_used"], what
    assert got.support == want["support"], what
    assert np.abs(got.parameters - want["p"]).max() <= GPU_TOLERANCE, what
    assert abs(got.weight_sum - want["weight_sum"]) <= GPU_WEIGHT_RTOL * abs(want["weight_sum"]), what
    assert list(got.reserved) == [0, 0, 0], what


@pytest.mark.parametrize("w,h", SMALL_SHAPES)
def test_fit_matches_the_definition(flow2d, ctx, w, h):
    u, v, masks = fit_case(w, h)
    pu, pv = ctx.plane(w, h, u), ctx.plane(w, h, v)
    pm = {mode: None if m is None else ctx.plane(w, h, m) for mode, m in masks.items()}
    for mode in MASK_MODES:
        for model in MODELS:
            for sigma, k in FITS:
                if w * h > 10000 and (mode, model) not in (("soft", AFFINE), ("none", SIMILARITY), ("binary", TRANSLATION)):
                    continue
                got = ctx.global_motion(pu, pv, w, h, model, sigma, k, pm[mode])[0]
                want = global_motion_reference(u, v, masks[mode], model, sigma, k)
                check_record(got, want, "%dx%d masks=%s model=%d sigma=%g K=%d" % (w, h, mode, model, sigma, k))


def test_fit_full_hd(flow2d, ctx):
    w, h = 1920, 1080
    u, v, masks = fit_case(w, h)
    pu, pv, pm = ctx.plane(w, h, u), ctx.plane(w, h, v), ctx.plane(w, h, masks["soft"])
    got = ctx.global_motion(pu, pv, w, h, AFFINE, 0.5, 5, pm)[0]
    check_record(got, global_motion_reference(u, v, masks["soft"], AFFINE, 0.5, 5), "1920x1080")
    assert got.model_used == AFFINE and 0 < got.support < w * h


def test_fit_finds_the_scene(flow2d, ctx):
    """The device fit on the scenes' fp32 ground truth: the affine scene's parameters, and two_layer's static background."""
    sc = scenes_module().make_scene("two_layer", 64, 64, seed=0)
    pu, pv = ctx.plane(64, 64, sc.gt_u), ctx.plane(64, 64, sc.gt_v)
    plain = ctx.global_motion(pu, pv, 64, 64, AFFINE, 0.5, 0)[0]
    robust = ctx.global_motion(pu, pv, 64, 64, AFFINE, 0.5, 5)[0]
    assert abs(plain.p[0]) > 0.25 and np.abs(robust.parameters).max() < 5e-3


def record_bytes(ctx, motion, instances=1):
    return [bytes(r) for r in ctx.read_motion(motion, instances)]


def test_repeated_calls_and_a_replayed_graph_give_the_same_bytes(flow2d, ctx):
    w, h = 640, 480
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    u, v, masks = fit_case(w, h)
    pu, pv, pm = ctx.plane(w, h, u), ctx.plane(w, h, v), ctx.plane(w, h, masks["soft"])
    first, second, replay = (ctx.motion_records() for _ in range(3))
    ctx.global_motion(pu, pv, w, h, AFFINE, 0.5, 5, pm, motion=first)     # (also allocates the context's workspace)
    ctx.global_motion(pu, pv, w, h, AFFINE, 0.5, 5, pm, motion=second)
    eager = record_bytes(ctx, first)
    assert eager == record_bytes(ctx, second)
    replay.fill_bytes(0)
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    try:
        ctx.global_motion(pu, pv, w, h, AFFINE, 0.5, 5, pm, motion=replay)
    finally:
        graph = vp()
        assert lib.flow2d_capture_end(ctx.handle, ctypes.byref(graph)) == 0
    try:
        ctx.synchronize()
        assert not replay.download().any()  # captured, not run
        for _ in range(2):
            replay.fill_bytes(0x7F)
            assert lib.flow2d_graph_launch(ctx.handle, graph) == 0
            ctx.synchronize()
            assert record_bytes(ctx, replay) == eager
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)
    check_record(ctx.read_motion(first)[0], global_motion_reference(u, v, masks["soft"], AFFINE, 0.5, 5), "640x480")


@pytest.mark.parametrize("kind", ["contiguous", "rows", "bytes"])
def test_lock_step_batch(flow2d, ctx, kind):
    """Three instances `stride` apart: record b has the bytes of the same planes fitted alone; the model planes, residuals,
    weights and warped frames of every instance are the restatement for its own record, and every other word of the output
    allocations is what it was."""
    w, h, cw, ch, count = 300, 70, 320, 80, 3
    stride = stride_of(kind, pitch_of(cw), ch)
    cases = [fit_case(w, h, seed=20 + b) for b in range(count)]
    frames = [np.random.default_rng(b).uniform(1, 255, (h, w)).astype(F32) for b in range(count)]
    fill = lambda arrays: Tall(ctx, cw, ch, count, stride).fill(arrays)  # noqa: E731
    tu, tv, tm, tf = fill([c[0] for c in cases]), fill([c[1] for c in cases]), fill([c[2]["soft"] for c in cases]), fill(frames)
    motion = ctx.motion_records(count)
    with ctx.set_batch(count, stride):
        ctx.global_motion(tu, tv, w, h, AFFINE, 0.5, 3, tm, instances=count, motion=motion)
    batch = ctx.read_motion(motion, count)
    for b, (u, v, masks) in enumerate(cases):
        alone = ctx.global_motion(ctx.plane(w, h, u), ctx.plane(w, h, v), w, h, AFFINE, 0.5, 3, ctx.plane(w, h, masks["soft"]))[0]
        assert bytes(alone) == bytes(batch[b]), "instance %d" % b
        check_record(batch[b], global_motion_reference(u, v, masks["soft"], AFFINE, 0.5, 3), "instance %d" % b)
    assert len({bytes(r) for r in batch}) == count
    for t in (tu, tv, tm):
        t.check(None, "fit: an input")
    # the per-pixel entries under the same batch, with gentle records so that the warp samples
    gentle = [flow2d.GlobalMotion.from_parameters([1.5 - b, 0.01 * b, -0.02, 0.75 * b, 0.015, -0.01]) for b in range(count)]
    ctx.upload_motion(gentle, motion)
    outs = [Tall(ctx, cw, ch, count, stride) for _ in range(7)]
    with ctx.set_batch(count, stride):
        ctx.global_flow(motion, w, h, tu, tv, tm, 0.5, *outs[:5])
        ctx.warp_global(motion, tf, w, h, outs[5], outs[6], fill=-3.0)
    ctx.synchronize()
    want = [global_flow_reference(g.parameters, (h, w), c[0], c[1], c[2]["soft"], 0.5) for g, c in zip(gentle, cases)]
    for o, name in zip(outs[:5], ("model_u", "model_v", "residual_u", "residual_v", "weight")):
        o.check([x[name] for x in want], "global_flow %s: %s" % (kind, name))
    warped = [warp_global_reference(g.parameters, f, -3.0) for g, f in zip(gentle, frames)]
    assert all(0 < x[1].mean() < 1 for x in warped)
    outs[5].check([x[0] for x in warped], "warp_global %s" % kind)
    outs[6].check([x[1] for x in warped], "warp_global %s: valid" % kind)
    for t in (tu, tv, tm, tf):
        t.check(None, "an input")
    # the batch switched off: instance 0 only
    outs[5].upload()
    ctx.warp_global(motion, tf, w, h, outs[5], fill=-3.0)
    ctx.synchronize()
    outs[5].check([x[0] for x in warped], "warp_global, batch switched off", upto=1)
    # a written plane must not meet a later instance of an input, nor the later records
    lib = flow2d.hip_lib()
    with ctx.set_batch(count, stride):
        assert lib.flow2d_warp_global_2d(ctx.handle, motion.ptr, tf.ptr, w, h, tf.pitch, ctypes.c_float(0), tf.ptr + 2 * stride,
                                         None) == 1
        assert lib.flow2d_global_motion_2d(ctx.handle, tu.ptr, tv.ptr, None, w, h, tu.pitch, AFFINE, 0.5, 1, tv.ptr + 2 * stride,
                                           outs[0].ptr, 4096) == 1


def poisoned(ctx, w, h, n):
    planes = [ctx.plane(w, h) for _ in range(n)]
    for p in planes:
        p.fill_bytes(0x7F)
    return planes


def untouched(plane):
    return (plane.download().view(np.uint32) == 0x7F7F7F7F).all()


@pytest.mark.parametrize("w,h", SMALL_SHAPES + [(1920, 1080)])
def test_global_flow_and_warp_match_the_definitions(flow2d, ctx, w, h):
    """The GPU's own record fed to the restatements: every plane bit for bit (there is no sum in them)."""
    u, v, masks = fit_case(w, h)
    frame = np.random.default_rng(w + h).uniform(1, 255, (h, w)).astype(F32)
    pu, pv, pm, pf = ctx.plane(w, h, u), ctx.plane(w, h, v), ctx.plane(w, h, masks["soft"]), ctx.plane(w, h, frame)
    motion = ctx.motion_records()
    ctx.global_motion(pu, pv, w, h, AFFINE, 0.5, 5, pm, motion=motion)
    rec = ctx.read_motion(motion)[0]
    names = ("model_u", "model_v", "residual_u", "residual_v", "weight")
    for sigma, mask in ((0.5, "soft"), (0.0, "none")):
        outs = poisoned(ctx, w, h, 5)
        ctx.global_flow(motion, w, h, pu, pv, pm if mask == "soft" else None, sigma, *outs)
        want = global_flow_reference(rec.parameters, (h, w), u, v, masks[mask], sigma)
        for o, name in zip(outs, names):
            assert_same(o.download(), want[name], "%dx%d sigma=%g: %s" % (w, h, sigma, name))
        for o in outs:
            o.free()
    if w * h > 1000:
        assert np.isnan(want["residual_u"]).any() and np.isfinite(want["residual_u"]).any() and (want["weight"] == 0).any()
    # outputs not asked for stay poisoned; the model alone needs no flow
    outs = poisoned(ctx, w, h, 5)
    ctx.global_flow(motion, w, h, model_u=outs[0], model_v=outs[1])
    ctx.global_flow(motion, w, h, pu, pv, None, 0.5, weight=outs[4])
    want = global_flow_reference(rec.parameters, (h, w), u, v, None, 0.5)
    for i in (0, 1, 4):
        assert_same(outs[i].download(), want[names[i]], names[i] + " alone")
    assert untouched(outs[2]) and untouched(outs[3])
    ctx.global_flow(motion, w, h, pu, pv, residual_u=outs[2], residual_v=outs[3])
    assert_same(outs[2].download(), want["residual_u"], "residual alone")
    # the warp: the fitted record (a translation of up to 20 px: part of the frame leaves), then a gentle one
    for p, fill in ((rec.parameters, -7.0), ([0.4, 0.01, -0.02, -0.3, 0.015, 0.005], float("nan"))):
        ctx.upload_motion([flow2d.GlobalMotion.from_parameters(p)], motion)
        out, valid, lone = poisoned(ctx, w, h, 3)
        ctx.warp_global(motion, pf, w, h, out, valid, fill=fill)
        ctx.warp_global(motion, pf, w, h, lone, fill=fill)
        want_out, want_valid = warp_global_reference(p, frame, fill)
        assert_same(out.download(), want_out, "%dx%d warp" % (w, h))
        assert_same(valid.download(), want_valid, "%dx%d warp: valid" % (w, h))
        assert_same(lone.download(), want_out, "%dx%d warp without valid" % (w, h))
    if w * h > 1000:
        assert 0 < want_valid.mean() < 1
    assert_same(pf.download(), frame, "the frame")


@pytest.mark.parametrize("p", [[np.nan, 0, 0, 0, 0, 0], [0, 0, 0, 0, np.nan, 0], [1e30, 0, 0, 0, 0, 0], [0, 0, 0, -1e30, 0, 0],
                               [0, 1e300, 0, 0, 0, 0], [np.inf, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, -1e30]])
def test_wild_records_fill_the_frame(flow2d, ctx, p):
    """NaN, infinite and huge parameters: every pixel gets `fill`, valid is 0, and nothing outside the plane is read (the planes
    of a context lie next to each other: a stray read would fault or show).  Even sizes: no pixel has a centred coordinate of 0,
    so a wild linear term moves every pixel."""
    w, h = 130, 76
    frame = np.random.default_rng(1).uniform(1, 255, (h, w)).astype(F32)
    pf = ctx.plane(w, h, frame)
    motion = ctx.upload_motion([flow2d.GlobalMotion.from_parameters(p)])
    out, valid = poisoned(ctx, w, h, 2)
    ctx.warp_global(motion, pf, w, h, out, valid, fill=-2.5)
    assert (out.download() == -2.5).all() and not valid.download().any()
    want_out, want_valid = warp_global_reference(p, frame, -2.5)
    assert (want_out == -2.5).all() and not want_valid.any()


def test_invalid_arguments_write_nothing(flow2d, ctx):
    w, h = 100, 40
    lib = flow2d.hip_lib()
    u, v, masks = fit_case(w, h)
    pu, pv, pm = ctx.plane(w, h, u), ctx.plane(w, h, v), ctx.plane(w, h, masks["binary"])
    motion = ctx.motion_records()
    need = lib.flow2d_global_motion_workspace_bytes(w, h, 1)
    ws = ctx.plane(max(need // 4, 4), 1)
    outs = poisoned(ctx, w, h, 5)
    motion.fill_bytes(0x7F)
    ws.fill_bytes(0x7F)
    d = dict(u=pu.ptr, v=pv.ptr, mask=pm.ptr, w=w, h=h, pitch=pu.pitch, model=AFFINE, sigma=0.5, k=5, motion=motion.ptr, ws=ws.ptr,
             ws_bytes=need)

    def fit(**kw):
        a = dict(d, **kw)
        return lib.flow2d_global_motion_2d(ctx.handle, a["u"], a["v"], a["mask"], a["w"], a["h"], a["pitch"], a["model"], a["sigma"],
                                           a["k"], a["motion"], a["ws"], a["ws_bytes"])

    bad = [dict(u=None), dict(v=None), dict(motion=None), dict(ws=None), dict(w=0), dict(h=0), dict(pitch=pu.pitch + 8),
           dict(pitch=16), dict(sigma=-0.5), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(k=-1), dict(k=17),
           dict(model=3), dict(model=-1), dict(motion=motion.ptr + 4), dict(ws=ws.ptr + 8), dict(ws_bytes=need - 1),
           dict(motion=pu.ptr), dict(motion=pm.ptr + pu.pitch), dict(ws=pv.ptr), dict(ws=motion.ptr, ws_bytes=need)]
    for kw in bad:
        assert fit(**kw) == 1, kw
    with ctx.set_batch(2, pu.pitch * h):
        assert fit() == 1  # a workspace for one instance under a batch of two
    ctx.synchronize()
    assert untouched(motion) and untouched(ws)
    assert fit() == 0
    ctx.synchronize()
    rec = ctx.read_motion(motion)[0]
    check_record(rec, global_motion_reference(u, v, masks["binary"], AFFINE, 0.5, 5), "after the refusals")
    vp = lambda q: q.ptr if q else None  # noqa: E731

    def flow(motion=motion, u=pu, v=pv, sigma=0.5, w=w, h=h, pitch=pu.pitch, o=outs):
        return lib.flow2d_global_flow_2d(ctx.handle, vp(motion), vp(u), vp(v), pm.ptr, w, h, pitch, sigma, *[vp(q) for q in o])

    assert flow(motion=None) == 1 and flow(u=None) == 1 and flow(u=None, v=None) == 1 and flow(o=[None] * 5) == 1
    assert flow(o=[outs[0], None] + outs[2:]) == 1 and flow(o=outs[:2] + [outs[2], None, outs[4]]) == 1
    assert flow(sigma=-1.0) == 1 and flow(sigma=float("nan")) == 1 and flow(w=0) == 1 and flow(h=0) == 1 and flow(pitch=16) == 1
    assert flow(o=[outs[0], outs[0]] + outs[2:]) == 1 and flow(o=[pu] + outs[1:]) == 1 and flow(o=outs[:4] + [pm]) == 1

    def warp(motion=motion, frame=pu, w=w, h=h, pitch=pu.pitch, out=outs[0], valid=outs[1]):
        return lib.flow2d_warp_global_2d(ctx.handle, vp(motion), vp(frame), w, h, pitch, ctypes.c_float(1.0), vp(out), vp(valid))

    assert warp(motion=None) == 1 and warp(frame=None) == 1 and warp(out=None) == 1 and warp(w=0) == 1 and warp(h=0) == 1
    assert warp(pitch=16) == 1 and warp(out=pu) == 1 and warp(valid=pu) == 1 and warp(valid=outs[0]) == 1
    ctx.synchronize()
    assert all(untouched(o) for o in outs)
    assert flow() == 0 and warp() == 0
    ctx.synchronize()
    assert not any(untouched(o) for o in outs)


# ---- the host layer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref,masks,model", [(0, False, AFFINE), (2, True, SIMILARITY), (4, False, TRANSLATION)])
def test_stabilise_sequence_equals_its_parts(flow2d, ctx, ref, masks, model):
    """OpticalFlow.stabilise_sequence_device equals compute_flow_bidirectional_device on the whole sequence, Context.global_motion
    on the flow towards the far side of the reference (with the occlusion mask of that flow when masks), compose_motion outwards
    from the reference and Context.warp_global: the frames bit for bit -- from the records the call returns --, the records
    within the tolerance of the fit.  The reference frame comes back bit for bit; the host-image form gives the same frames."""
    scene = {AFFINE: "affine", SIMILARITY: "rotation", TRANSLATION: "translation"}[model]  # a motion the model holds
    seq = scenes_module().make_sequence(scene, 5, 192, 160, seed=1)
    count, (h, w) = len(seq.frames), seq.frames[0].shape
    sigma, k, fill = 0.5, 3, -1.0
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        p = flow.params(*CLI_PARAMS)
        frames = [ctx.plane(w, h, a) for a in seq.frames]
        outs = poisoned(ctx, w, h, count)
        motions = flow.stabilise_sequence_device([q.ptr for q in frames], [o.ptr for o in outs], p, ref, model, sigma, k, masks, fill)
        got = [o.download() for o in outs]
        parts = [[ctx.plane(w, h) for _ in range(count - 1)] for _ in range(6)]
        flow.compute_flow_bidirectional_device([q.ptr for q in frames], *[[q.ptr for q in part] for part in parts[:4]], p,
                                               [q.ptr for q in parts[4]], [q.ptr for q in parts[5]])
        ctx.synchronize()
        us, vs, bus, bvs, occ_f, occ_b = parts
        steps = {}
        for j in range(count - 1):
            if j >= ref:   # M(j -> j + 1)
                steps[j + 1] = ctx.global_motion(us[j], vs[j], w, h, model, sigma, k, occ_f[j] if masks else None)[0]
            else:          # M(j + 1 -> j)
                steps[j] = ctx.global_motion(bus[j], bvs[j], w, h, model, sigma, k, occ_b[j] if masks else None)[0]
        want = {ref: np.zeros(6)}
        for j in range(ref + 1, count):
            want[j] = steps[j].parameters if j == ref + 1 else compose_motion(want[j - 1], steps[j].parameters)
        for j in range(ref - 1, -1, -1):
            want[j] = steps[j].parameters if j == ref - 1 else compose_motion(want[j + 1], steps[j].parameters)
        motion = ctx.motion_records()
        for j in range(count):
            assert np.abs(motions[j].parameters - want[j]).max() <= GPU_TOLERANCE, j
            assert motions[j].model_used == model
            if j == ref:
                assert_same(got[j], seq.frames[j], "the reference frame")
                assert not motions[j].parameters.any()
                continue
            assert motions[j].support == steps[j].support and motions[j].weight_sum == steps[j].weight_sum
            ctx.upload_motion([motions[j]], motion)
            out = ctx.plane(w, h)
            ctx.warp_global(motion, frames[j], w, h, out, fill=fill)
            assert_same(got[j], out.download(), "frame %d" % j)
            assert_same(got[j], warp_global_reference(motions[j].parameters, seq.frames[j], fill)[0], "frame %d, restatement" % j)
            assert_same(frames[j].download(), seq.frames[j], "input frame %d" % j)
            covered = got[j] != fill
            before = np.abs(seq.frames[j] - seq.frames[ref])[covered].mean()
            after = np.abs(got[j] - seq.frames[ref])[covered].mean()
            print("frame %d: mean |difference to the reference| %.3f -> %.3f over %.0f %%" % (j, before, after, 100 * covered.mean()))
            assert after < 0.5 * before
        if ref == 0:  # (how close the computed flow brings the first step to the scene's motion: tools/stabilisation_table.py)
            print("error of M(0 -> 1):", np.abs(motions[1].parameters - scene_motion(seq)))
        host, host_motions = flow.stabilise_sequence(seq.frames, p, ref, model, sigma, k, masks, fill)
        for j in range(count):
            assert_same(host[j], got[j], "host-image form, frame %d" % j)
            assert bytes(host_motions[j]) == bytes(motions[j])
        for bad in (dict(model=3), dict(sigma=-1.0), dict(iterations=17), dict(reference_index=count)):
            with pytest.raises(flow2d.Flow2DError):
                flow.stabilise_sequence(seq.frames, p, **bad)
        with pytest.raises(flow2d.Flow2DError):  # an output that is a frame
            flow.stabilise_sequence_device([q.ptr for q in frames], [frames[1].ptr] + [o.ptr for o in outs[1:]], p)
    finally:
        flow.close()


def scene_motion(seq):
    from test_global_motion_cpu import true_motion
    return true_motion(seq)


def test_estimate_global_motion(flow2d, ctx):
    """One pair: the record of the flow the object computes -- compute_flow's bits --, with and without the occlusion mask, and
    the residual planes of flow2d_global_flow_2d."""
    sc = scenes_module().make_scene("two_layer", 192, 160, seed=0)
    h, w = sc.shape
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        p = flow.params(*CLI_PARAMS)
        rec, (u, v), (ru, rv) = flow.estimate_global_motion(sc.frame_0, sc.frame_1, p, AFFINE, 0.5, 5, flow=True, residual=True)
        cu, cv, _ = flow.compute_flow(sc.frame_0, sc.frame_1, p)
        assert_same(u, cu, "the flow")
        assert_same(v, cv, "the flow")
        check_record(rec, global_motion_reference(u, v, None, AFFINE, 0.5, 5), "estimate_global_motion")
        want = global_flow_reference(rec.parameters, (h, w), u, v)
        assert_same(ru, want["residual_u"], "residual u")
        assert_same(rv, want["residual_v"], "residual v")
        assert np.abs(rec.parameters).max() < 0.1                       # the background stands still
        moving = sc.gt_u != 0
        print("max |p| %.4f, mean |residual u| on the square %.3f, on the background %.3f" %
              (np.abs(rec.parameters).max(), np.abs(ru[moving]).mean(), np.abs(ru[~moving]).mean()))
        assert np.abs(ru[moving]).mean() > np.abs(ru[~moving]).mean()   # what is left is on the square
        f0, f1 = ctx.plane(w, h, sc.frame_0), ctx.plane(w, h, sc.frame_1)
        dev = flow.estimate_global_motion_device(f0.ptr, f1.ptr, p, AFFINE, 0.5, 5)
        assert bytes(dev) == bytes(rec)
        masked = flow.estimate_global_motion_device(f0.ptr, f1.ptr, p, AFFINE, 0.5, 5, masks=True)
        parts = [[ctx.plane(w, h)] for _ in range(6)]
        flow.compute_flow_bidirectional_device([f0.ptr, f1.ptr], *[[q[0].ptr] for q in parts[:4]], p, [parts[4][0].ptr],
                                               [parts[5][0].ptr])
        ctx.synchronize()
        alone = ctx.global_motion(parts[0][0], parts[1][0], w, h, AFFINE, 0.5, 5, parts[4][0])[0]
        assert bytes(masked) == bytes(alone) and masked.support < rec.support
    finally:
        flow.close()


def test_device_memory_does_not_grow_with_the_sequence(flow2d, ctx):
    """Free device memory (mem_info) after a run over 4 frames, then over 12 frames, then over 4 again, in one object with the
    caller's planes allocated up front: the three readings are equal.  As in test_gpu_denoise: an object of its own runs the
    longest sequence first and is closed, and nothing is freed between the readings that are compared."""
    w = h = 128
    seq = scenes_module().make_sequence("affine", 12, w, h, seed=0)
    frames = [ctx.plane(w, h, a) for a in seq.frames]
    outs = [ctx.plane(w, h) for _ in range(12)]

    def run(flow, count):
        flow.stabilise_sequence_device([q.ptr for q in frames[:count]], [o.ptr for o in outs[:count]],
                                       flow.params(8, 0.7, 5, 5, 35.0, 0.001, 0.001, 5, 1.5), 1, AFFINE, 0.5, 2, True)
        ctx.synchronize()
        return ctx.mem_info()[0]

    warm = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        run(warm, 12)
    finally:
        warm.close()
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        ctx.synchronize()
        before = ctx.mem_info()[0]
        free = [run(flow, count) for count in (4, 12, 4)]
    finally:
        flow.close()
    print("free before %d, after 4 / 12 / 4 frames %s" % (before, free))
    assert free[0] == free[1] == free[2], (before, free)


def test_cli_global_motion(flow2d, ctx, tmp_path):
    """--global-motion prints the record of OpticalFlow.estimate_global_motion on the pair -- with --backward the masked one --,
    writes the residual flow (as .flo too with --flo) and leaves every other file as it was."""
    w, h = 584, 388
    plain = run_cli(flow2d, ["--flo"], tmp_path / "plain")
    r1, r2 = rub_pair()
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        p = flow.params(*CLI_PARAMS)
        for extra, masks, model, name in (([], False, SIMILARITY, "similarity"), (["--backward"], True, AFFINE, "affine")):
            out_dir = tmp_path / name
            data = os.path.join(ROOT, "tests", "data")
            cmd = [flow2d.CLI_PATH, "--global-motion", name, "--global-sigma", "0.75", "--global-iterations", "4", "--flo", "--u8"]
            cmd += extra + [os.path.join(data, "rub1.raw"), os.path.join(data, "rub2.raw"), "584", "388", "t_", str(out_dir) + "/"]
            out_dir.mkdir()
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            assert r.returncode == 0, r.stdout[-2000:]
            line = [q for q in r.stdout.splitlines() if q.startswith("Global motion: ")]
            assert len(line) == 1, r.stdout[-2000:]
            printed = json.loads(line[0][len("Global motion: "):])
            rec, (ru, rv) = flow.estimate_global_motion(r1, r2, p, model, 0.75, 4, masks, residual=True)
            assert printed["p"] == list(rec.p) and printed["model_used"] == rec.model_used == model and printed["model"] == model
            assert printed["weight_sum"] == rec.weight_sum and printed["support"] == rec.support
            files = {f: (out_dir / f).read_bytes() for f in os.listdir(out_dir)}
            new = {"t_residual-u-584-388.raw", "t_residual-v-584-388.raw", "t_residual.flo"}
            assert new <= set(files) and not new & set(plain)
            for f in plain:
                assert files[f] == plain[f], f
            assert files["t_residual-u-584-388.raw"] == ru.tobytes() and files["t_residual-v-584-388.raw"] == rv.tobytes()
            fu, fv = flow2d.read_flo(str(out_dir / "t_residual.flo"))
            assert_same(fu, ru, "residual.flo")
            assert_same(fv, rv, "residual.flo")
    finally:
        flow.close()


def test_table_gpu_rows_equal_numpy_rows(flow2d):
    """tools/stabilisation_table.py: with the true flows the GPU rows and the numpy rows are the same printed numbers."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        table = importlib.import_module("stabilisation_table")
    finally:
        sys.path.pop(0)
    names = ("rotation", "affine", "two_layer")
    gpu = table.true_rows(False, 96, 0, names, 4)
    cpu = table.true_rows(True, 96, 0, names, 4)
    assert len(gpu) == len(cpu) and len(gpu) >= len(names) * 3
    for g, c in zip(gpu, cpu):
        assert g["engine"] == "gpu" and c["engine"] == "numpy"
        assert table.format_row(g).replace("gpu  ", "numpy") == table.format_row(c), (g, c)
