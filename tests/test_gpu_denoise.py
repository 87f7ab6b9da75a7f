"""Temporal denoising on the MI355X: flow2d_denoise_2d and flow2d_compose_flow_2d bit for bit against the numpy restatements of
their definitions (tests/test_denoise_cpu.py) from 1x1 to 4096^2, lock-step batches with contiguous and padded strides and a
captured graph against direct calls, the degenerate calls, OpticalFlow.denoise_sequence_device against
compute_flow_bidirectional_device followed by Context.compose_flow and Context.denoise, the host-image form and the CLI's --denoise
against the device path, the device memory of a long and a short sequence, and the results table's GPU rows against its numpy
rows."""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from test_denoise_cpu import compose_reference, denoise_reference
from test_gpu_batch_kernels import Tall, drive, pitch_of, stride_of
from test_oracle import rub_pair

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_PARAMS = (50, 0.9, 40, 5, 35.0, 0.001, 0.001, 5, 1.5)  # the CLI's defaults (main.cpp)


def random_case(rng, w, h, n, edge_cases=True):
    """A centre and n neighbour frames in [1, 255]; per neighbour a flow of a translation up to +-20 px plus noise with 10 %
    wild vectors, and a mask -- 0 / 1 for even neighbours, uniform in [-0.5, 1.5] for odd ones; with edge_cases NaNs, vectors
    far out of the frame (+-1e6, +-3e38) and NaN masks.  Returns (centre, frames, us, vs, occs)."""
    centre = rng.uniform(1, 255, (h, w)).astype(F32)
    frames, us, vs, occs = [], [], [], []
    for k in range(n):
        frames.append(rng.uniform(1, 255, (h, w)).astype(F32))
        t = rng.uniform(-20, 20, 2)
        flow = [(t[i] + rng.normal(0, 0.5, (h, w))).astype(F32) for i in range(2)]
        for a in flow:
            wild = rng.random((h, w)) < 0.1
            a[wild] = rng.uniform(-20, 20, wild.sum())
            if edge_cases:
                pick = rng.random((h, w))
                a[pick < 0.01] = np.nan
                a[(pick >= 0.01) & (pick < 0.015)] = 1e6
                a[(pick >= 0.015) & (pick < 0.02)] = -1e6
                a[(pick >= 0.02) & (pick < 0.025)] = -3e38
                a[(pick >= 0.025) & (pick < 0.03)] = 3e38
        occ = (rng.random((h, w)) < 0.3).astype(F32) if k % 2 == 0 else rng.uniform(-0.5, 1.5, (h, w)).astype(F32)
        if edge_cases:
            occ[rng.random((h, w)) < 0.02] = np.nan
        us.append(flow[0])
        vs.append(flow[1])
        occs.append(occ)
    return centre, frames, us, vs, occs


def pick_masks(occs, mode):
    """all / none / mixed (every second entry absent)."""
    if mode == "none":
        return None
    return [o if (mode == "all" or k % 2 == 0) else None for k, o in enumerate(occs)]


def device_denoise(ctx, case, occs, sigma, with_sum=True):
    centre, frames, us, vs, _ = case
    h, w = centre.shape
    up = lambda q: [None if a is None else ctx.plane(w, h, a) for a in q]  # noqa: E731
    pc, pf, pu, pv = ctx.plane(w, h, centre), up(frames), up(us), up(vs)
    po = None if occs is None else up(occs)
    out, wsum = ctx.plane(w, h), ctx.plane(w, h)
    out.fill_bytes(0x7F)
    wsum.fill_bytes(0x7F)
    ctx.denoise(pc, pf, pu, pv, w, h, out, po, sigma, wsum if with_sum else None)
    ctx.synchronize()
    got = out.download(), wsum.download()
    for p in [pc, out, wsum] + pf + pu + pv + [q for q in (po or []) if q is not None]:
        p.free()
    return got


def assert_same(got, want, what):
    same = (np.asarray(got, F32).view(np.uint32) == np.asarray(want, F32).view(np.uint32))
    assert same.all(), "%s: %d of %d pixels differ" % (what, (~same).sum(), same.size)


POISON = np.full(1, 0x7F7F7F7F, np.uint32).view(F32)[0]


@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("w,h", [(1, 1), (1, 9), (9, 1), (17, 5), (67, 33), (256, 256)])
def test_denoise_matches_the_definition(flow2d, ctx, w, h, n):
    case = random_case(np.random.default_rng(w * 10007 + h * 13 + n), w, h, n)
    for mode in ("all", "none", "mixed"):
        for sigma in (0.0, 12.5):
            for with_sum in (True, False):
                if w * h > 10000 and (with_sum ^ (sigma == 0.0)) and mode != "all":
                    continue
                occs = pick_masks(case[4], mode)
                out, wsum = device_denoise(ctx, case, occs, sigma, with_sum)
                want, want_sum = denoise_reference(case[0], case[1], case[2], case[3], occs, sigma)
                what = "%dx%d N=%d masks=%s sigma=%g" % (w, h, n, mode, sigma)
                assert np.isfinite(want).all() and want_sum.min() >= 1 and want_sum.max() <= n + 1
                assert_same(out, want, what)
                if with_sum:
                    assert_same(wsum, want_sum, what + ": weight_sum")
                else:
                    assert (wsum.view(np.uint32) == 0x7F7F7F7F).all(), what + ": weight_sum was not asked for"


@pytest.mark.parametrize("w,h,n,sigma", [(1920, 1080, 3, 12.5), (4096, 4096, 2, 0.0), (4096, 4096, 1, 20.0)])
def test_denoise_large_frames(flow2d, ctx, w, h, n, sigma):
    case = random_case(np.random.default_rng(w + h + n), w, h, n)
    occs = pick_masks(case[4], "mixed" if n > 1 else "all")
    out, wsum = device_denoise(ctx, case, occs, sigma)
    want, want_sum = denoise_reference(case[0], case[1], case[2], case[3], occs, sigma)
    assert_same(out, want, "%dx%d" % (w, h))
    assert_same(wsum, want_sum, "%dx%d: weight_sum" % (w, h))


def compose_case(rng, w, h, edge_cases=True):
    _, _, flows, more, occs = random_case(rng, w, h, 2, edge_cases)
    small = lambda a: np.where(np.abs(a) < 1e5, a * F32(0.2), a).astype(F32)  # noqa: E731  most first steps stay inside
    return small(flows[0]), small(more[0]), flows[1], more[1], occs[0], occs[1]


def device_compose(ctx, case, masks=(True, True), with_mask=True):
    h, w = case[0].shape
    planes = [ctx.plane(w, h, a) for a in case[:4]]
    pm = [ctx.plane(w, h, a) if m else None for a, m in zip(case[4:], masks)]
    outs = [ctx.plane(w, h) for _ in range(3)]
    for o in outs:
        o.fill_bytes(0x7F)
    ctx.compose_flow(*planes, w, h, outs[0], outs[1], pm[0], pm[1], outs[2] if with_mask else None)
    ctx.synchronize()
    got = [o.download() for o in outs]
    for p in planes + outs + [q for q in pm if q]:
        p.free()
    return got


@pytest.mark.parametrize("w,h", [(1, 1), (1, 9), (9, 1), (17, 5), (67, 33), (256, 256), (1920, 1080), (4096, 4096)])
def test_compose_matches_the_definition(flow2d, ctx, w, h):
    case = compose_case(np.random.default_rng(w * 31 + h), w, h)
    combos = ((True, True), (False, False), (True, False), (False, True)) if w * h < 1e6 else ((True, True),)
    for masks in combos:
        want = compose_reference(*case[:4], case[4] if masks[0] else None, case[5] if masks[1] else None)
        got = device_compose(ctx, case, masks)
        for g, x, name in zip(got, want, ("u", "v", "mask")):
            assert_same(g, x, "%dx%d masks=%s: %s" % (w, h, masks, name))
    if w * h >= 1000:  # both branches are there
        assert np.isnan(want[0]).any() and np.isfinite(want[0]).any() and (want[2] == 0).any() and (want[2] == 1).any()
    if w * h < 1e6:
        got = device_compose(ctx, case, with_mask=False)
        assert_same(got[0], want[0], "no out_mask: u")
        assert (got[2].view(np.uint32) == 0x7F7F7F7F).all()
        # a zero first flow stays inside the frame at every size
        zero = np.zeros((h, w), F32)
        still = (zero, zero) + tuple(case[2:])
        want = compose_reference(*still)
        assert (want[2][np.isfinite(case[2]) & np.isfinite(want[0])] >= 0).all() and np.isfinite(want[0]).any()
        for g, x, name in zip(device_compose(ctx, still), want, ("u", "v", "mask")):
            assert_same(g, x, "%dx%d zero first flow: %s" % (w, h, name))


@pytest.mark.parametrize("sigma", [0.0, 7.5])
def test_degenerate_calls_return_the_centre(flow2d, ctx, sigma):
    """Every mask 1, every flow NaN, every flow leaving the frame: the centre frame bit for bit, weight sum 1."""
    w, h, n = 131, 77, 3
    rng = np.random.default_rng(3)
    centre, frames, us, vs, _ = random_case(rng, w, h, n, edge_cases=False)
    ones = [np.ones((h, w), F32)] * n
    nan = [np.full((h, w), np.nan, F32)] * n
    far = [np.full((h, w), 1e6, F32), np.full((h, w), -3e38, F32), np.full((h, w), np.inf, F32)]
    for a, b, occs in ((us, vs, ones), (nan, vs, None), (us, nan, None), (far, vs, None), (us, far, None)):
        out, wsum = device_denoise(ctx, (centre, frames, a, b, None), occs, sigma)
        assert_same(out, centre, "degenerate")
        assert_same(wsum, np.ones((h, w), F32), "degenerate: weight_sum")


@pytest.mark.parametrize("kind", ["contiguous", "rows", "bytes"])
def test_lock_step_batch(flow2d, ctx, kind):
    """Three instances, `stride` apart (contiguous, padding rows, 16 bytes off a pitch multiple), outputs poisoned: every
    instance's rectangle is the restatement for its own inputs, every other word of the allocations is what it was, the inputs
    are unchanged; the batch switched off, the same call touches instance 0 only."""
    w, h, cw, ch, count, n = 100, 70, 128, 80, 3, 3
    stride = stride_of(kind, pitch_of(cw), ch)
    rng = np.random.default_rng(11)
    cases = [random_case(rng, w, h, n) for _ in range(count)]
    fill = lambda arrays: Tall(ctx, cw, ch, count, stride).fill(arrays)  # noqa: E731
    centre = fill([c[0] for c in cases])
    frames, us, vs, occs = ([fill([c[part][k] for c in cases]) for k in range(n)] for part in (1, 2, 3, 4))
    out, wsum = Tall(ctx, cw, ch, count, stride), Tall(ctx, cw, ch, count, stride)
    masks = [occs[0], None, occs[2]]
    want = [denoise_reference(c[0], c[1], c[2], c[3], [c[4][0], None, c[4][2]], 9.0) for c in cases]
    drive(ctx, count, stride, lambda: ctx.denoise(centre, frames, us, vs, w, h, out, masks, 9.0, wsum),
          [(out, [x[0] for x in want]), (wsum, [x[1] for x in want])], [centre] + frames + us + vs + [occs[0], occs[2]],
          "denoise_2d %s" % kind)
    # the output must not meet a later instance of an input either
    lib = flow2d.hip_lib()
    arr = lambda q: (ctypes.c_void_p * n)(*[p.ptr if p else None for p in q])  # noqa: E731
    with ctx.set_batch(count, stride):
        assert lib.flow2d_denoise_2d(ctx.handle, centre.ptr, n, arr(frames), arr(us), arr(vs), arr(masks), w, h, centre.pitch,
                                     ctypes.c_float(9.0), vs[1].ptr + 2 * stride, None) == 1
    # composition: the flows of neighbours 0 and 1 chained, with their masks
    ccases = [compose_case(rng, w, h) for _ in range(count)]
    planes = [fill([c[i] for c in ccases]) for i in range(6)]
    outs = [Tall(ctx, cw, ch, count, stride) for _ in range(3)]
    cwant = [compose_reference(*c) for c in ccases]
    drive(ctx, count, stride, lambda: ctx.compose_flow(*planes[:4], w, h, outs[0], outs[1], planes[4], planes[5], outs[2]),
          [(outs[i], [x[i] for x in cwant]) for i in range(3)], planes, "compose_flow_2d %s" % kind)


def test_captured_graph_gives_the_same_frames(flow2d, ctx):
    w, h, n = 640, 480, 4
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    case = random_case(np.random.default_rng(5), w, h, n)
    eager, eager_sum = device_denoise(ctx, case, case[4], 6.0)
    ccase = compose_case(np.random.default_rng(6), w, h)
    ceager = device_compose(ctx, ccase)
    up = lambda q: [ctx.plane(w, h, a) for a in q]  # noqa: E731
    pc, pf, pu, pv, po, pcomp = ctx.plane(w, h, case[0]), up(case[1]), up(case[2]), up(case[3]), up(case[4]), up(ccase)
    outs = [ctx.plane(w, h) for _ in range(5)]
    for o in outs:
        o.fill_bytes(0)
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    try:
        ctx.denoise(pc, pf, pu, pv, w, h, outs[0], po, 6.0, outs[1])
        ctx.compose_flow(*pcomp[:4], w, h, outs[2], outs[3], pcomp[4], pcomp[5], outs[4])
    finally:
        graph = vp()
        assert lib.flow2d_capture_end(ctx.handle, ctypes.byref(graph)) == 0
    try:
        ctx.synchronize()
        assert not any(o.download().any() for o in outs)  # captured, not run
        for _ in range(2):
            for o in outs:
                o.fill_bytes(0x7F)
            assert lib.flow2d_graph_launch(ctx.handle, graph) == 0
            ctx.synchronize()
            for o, want in zip(outs, [eager, eager_sum] + ceager):
                assert_same(o.download(), want, "graph replay")
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)


def scenes_module():
    return importlib.import_module("cuda-flow2d_amd.scenes")


def fuse_from_parts(ctx, frames, parts, k, radius, sigma, masks):
    """Frame k fused the way DenoiseSequenceDevice documents it, from the planes of compute_flow_bidirectional_device:
    parts = (us, vs, back_us, back_vs, occ_fwd, occ_bwd), lists of Planes per pair."""
    h, w = frames[0].height, frames[0].width
    us, vs, bus, bvs, of, ob = parts
    count = len(frames)
    chain = {}
    temps = []
    for direction in (-1, 1):
        prev = None
        for d in range(1, radius + 1):
            j = k + direction * d
            if not 0 <= j < count:
                break
            step = (us[j - 1], vs[j - 1], of[j - 1]) if direction > 0 else (bus[j], bvs[j], ob[j])
            if d > 1:
                new = [ctx.plane(w, h) for _ in range(3)]
                temps += new
                ctx.compose_flow(prev[0], prev[1], step[0], step[1], w, h, new[0], new[1], prev[2] if masks else None,
                                 step[2] if masks else None, new[2] if masks else None)
                step = tuple(new)
            chain[j] = prev = step
    js = sorted(chain)
    out, wsum = ctx.plane(w, h), ctx.plane(w, h)
    ctx.denoise(frames[k], [frames[j] for j in js], [chain[j][0] for j in js], [chain[j][1] for j in js], w, h, out,
                [chain[j][2] for j in js] if masks else None, sigma, wsum)
    ctx.synchronize()
    got = out.download(), wsum.download()
    for p in temps + [out, wsum]:
        p.free()
    return got


@pytest.mark.parametrize("radius,sigma,masks", [(1, 0.0, True), (2, 20.0, True), (2, 0.0, False)])
def test_denoise_sequence_is_bidirectional_then_compose_then_denoise(flow2d, ctx, radius, sigma, masks):
    """OpticalFlow.denoise_sequence_device equals compute_flow_bidirectional_device on the whole sequence followed by
    Context.compose_flow and Context.denoise, bit for bit, for every frame -- the ends of the sequence, which have fewer
    neighbours, included -- and its weight sums too; the host-image form gives the same frames."""
    seq = scenes_module().make_sequence("two_layer", 6, 192, 160, seed=1)
    rng = np.random.default_rng(2)
    noised = (seq.frames + rng.normal(0, 4, seq.frames.shape)).astype(F32)
    count, (h, w) = len(noised), noised[0].shape
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        p = flow.params(*CLI_PARAMS)
        frames = [ctx.plane(w, h, a) for a in noised]
        outs, sums = ([ctx.plane(w, h) for _ in range(count)] for _ in range(2))
        for o in outs + sums:
            o.fill_bytes(0x7F)
        flow.denoise_sequence_device([q.ptr for q in frames], [o.ptr for o in outs], p, radius, sigma, masks,
                                     [s.ptr for s in sums])
        ctx.synchronize()
        got = [(o.download(), s.download()) for o, s in zip(outs, sums)]
        parts = [[ctx.plane(w, h) for _ in range(count - 1)] for _ in range(6)]
        flow.compute_flow_bidirectional_device([q.ptr for q in frames], *[[q.ptr for q in part] for part in parts[:4]], p,
                                               [q.ptr for q in parts[4]], [q.ptr for q in parts[5]])
        ctx.synchronize()
        for k in range(count):
            want, want_sum = fuse_from_parts(ctx, frames, parts, k, radius, sigma, masks)
            assert_same(got[k][0], want, "frame %d" % k)
            assert_same(got[k][1], want_sum, "frame %d: weight_sum" % k)
            assert want_sum.max() > 1 and want_sum.max() <= min(k, radius) + min(count - 1 - k, radius) + 1
        # without weight sums; the frames the caller handed in are unchanged
        for o in outs:
            o.fill_bytes(0x7F)
        flow.denoise_sequence_device([q.ptr for q in frames], [o.ptr for o in outs], p, radius, sigma, masks)
        ctx.synchronize()
        for k in range(count):
            assert_same(outs[k].download(), got[k][0], "frame %d, no weight sums" % k)
            assert_same(frames[k].download(), noised[k], "input frame %d" % k)
        host, host_sums = flow.denoise_sequence(noised, p, radius, sigma, masks, weight_sums=True)
        for k in range(count):
            assert_same(host[k], got[k][0], "host-image form, frame %d" % k)
            assert_same(host_sums[k], got[k][1], "host-image form, frame %d: weight_sum" % k)
        for bad in (dict(radius=0), dict(radius=5), dict(range_sigma=-1.0), dict(range_sigma=float("nan"))):
            with pytest.raises(flow2d.Flow2DError):
                flow.denoise_sequence(noised, p, **bad)
        with pytest.raises(flow2d.Flow2DError):
            flow.denoise_sequence(noised[:1], p)
        with pytest.raises(flow2d.Flow2DError):  # an output that is a frame
            flow.denoise_sequence_device([q.ptr for q in frames], [frames[1].ptr] + [o.ptr for o in outs[1:]], p)
    finally:
        flow.close()


def test_device_memory_does_not_grow_with_the_sequence(flow2d, ctx):
    """Free device memory (mem_info) after a run over 4 frames, then over 12 frames, then over 4 again, in one object with the
    caller's planes allocated up front: the three readings are equal -- what the object holds beyond the caller's planes is
    allocated by the first call and does not depend on the length of the sequence.
    Free memory is also moved by the HIP runtime itself: by what it sets up on first use (94 MB here), by pools of its own that
    grow in 10 MiB steps with the number of launches queued between two synchronisations, and by how it hands freed memory back
    (objects created and closed in turn read 136 / 28 / 122 / 122 MiB for 12 / 4 / 12 / 4 frames).  So an object of its own runs the
    longest sequence first and is closed, and nothing is freed between the readings that are compared."""
    w, h = 1024, 768
    seq = scenes_module().make_sequence("affine", 12, w, h, seed=0)
    frames = [ctx.plane(w, h, a) for a in seq.frames]
    outs = [ctx.plane(w, h) for _ in range(12)]

    def run(flow, count):
        flow.denoise_sequence_device([q.ptr for q in frames[:count]], [o.ptr for o in outs[:count]],
                                     flow.params(8, 0.7, 5, 5, 35.0, 0.001, 0.001, 5, 1.5), 1, 0.0, True)
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
    assert free[0] < before  # the ring and the chains are there


def run_cli(flow2d, args, out_dir, u8=True):
    out_dir.mkdir(exist_ok=True)
    data = os.path.join(ROOT, "tests", "data")
    cmd = [flow2d.CLI_PATH] + args + (["--u8"] if u8 else []) + [os.path.join(data, "rub1.raw"), os.path.join(data, "rub2.raw"),
                                                                "584", "388", "t_", str(out_dir) + "/"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:]
    return {f: (out_dir / f).read_bytes() for f in os.listdir(out_dir)}


def test_cli_denoise(flow2d, ctx, tmp_path):
    """--denoise SIGMA writes the two fused frames in the input's raw type and leaves every other file as it was; the frames
    are those of OpticalFlow.denoise_sequence on the pair (radius 1, masks on)."""
    w, h = 584, 388
    plain = run_cli(flow2d, [], tmp_path / "plain")
    den = run_cli(flow2d, ["--denoise", "12.5"], tmp_path / "den")
    new = {"t_denoised-1-584-388.raw", "t_denoised-2-584-388.raw"}
    assert not new & set(plain) and set(den) == set(plain) | new
    for f in plain:
        assert den[f] == plain[f], f
    r1, r2 = rub_pair()
    flow = flow2d.OpticalFlow(w, h, flow2d.GREY, ctx=ctx)
    try:
        want = flow.denoise_sequence(np.stack([r1, r2]), flow.params(*CLI_PARAMS), 1, 12.5, True)
    finally:
        flow.close()
    for k in (0, 1):
        got = np.frombuffer(den["t_denoised-%d-584-388.raw" % (k + 1)], np.uint8).reshape(h, w)
        assert np.array_equal(got, np.clip(want[k], 0, 255).astype(np.uint8)), k  # WriteRAWToFileU8: clamp, truncate
    assert np.abs(want[0] - r1).max() > 0.5  # something was fused


def test_table_gpu_rows_equal_numpy_rows(flow2d):
    """tools/denoising_table.py: with the true flows the GPU rows and the numpy rows are the same numbers."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        table = importlib.import_module("denoising_table")
    finally:
        sys.path.pop(0)
    names, noise = ("rotation", "two_layer"), (8.0,)
    gpu = table.true_rows(False, 128, 0, names, noise)
    cpu = table.true_rows(True, 128, 0, names, noise)
    assert len(gpu) == len(cpu) == 2 * 2 * 2 * 2
    for g, c in zip(gpu, cpu):
        assert g["engine"] == "gpu" and c["engine"] == "numpy"
        assert {k: v for k, v in g.items() if k != "engine"} == {k: v for k, v in c.items() if k != "engine"}, (g, c)
        assert g["rmse_after"] < g["rmse_before"]
    hidden = {(r["radius"], r["range_sigma"], r["masks"]): r["hidden_after"] for r in gpu if r["scene"] == "two_layer"}
    for radius in (1, 2):
        assert hidden[(radius, 0.0, True)] < hidden[(radius, 0.0, False)]


def test_planes_of_4_gib_and_more(flow2d, ctx):
    """Both kernels' 64-bit offset instantiations: a 40-pixel-wide frame in planes with a pitch of 1 MiB and 4200 rows, so a
    plane spans more than 4 GiB and the byte offsets of the rows from 4096 on do not fit 32 bits.  Bit for bit against the
    restatements, like every other size.  Then the same data in planes with a pitch of 255 616 floats, 4 294 348 800 bytes a plane:
    below 4 GiB, so both kernels take their 32-bit offsets, and from row 2101 on those have bit 31 set (2 148 196 864 at the start of
    row 2101; the frame's columns of row 2100 lie below 2^31).  The same bytes as the first run."""
    w, h = 40, 4200
    high = 255616
    assert (4 * high * h, 4 * high * 2101) == (4294348800, 2148196864) and 4 * high * h < 1 << 32 and 4 * high * 2100 + 4 * w < 1 << 31 <= 4 * high * 2101
    rng = np.random.default_rng(77)
    centre, frames, us, vs, occs = random_case(rng, w, h, 1)
    want, want_sum = denoise_reference(centre, frames, us, vs, occs, 12.5)
    case = compose_case(rng, w, h)
    cwant = compose_reference(*case)
    for line in (4096, 2101):
        assert (want_sum[line:] > 1).any()  # rows past the line gather
        assert np.isfinite(cwant[0][line:]).any()
        assert not np.array_equal(centre[line:], centre[:h - line]) and not np.array_equal(want[line:], want[:h - line])
    runs = []
    for wide in (262144, high):
        def plane(a=None):
            p = ctx.plane(wide, h)
            assert p.pitch == 4 * wide and (p.pitch * h >= 1 << 32) == (wide != high)
            return p.upload(a if a is not None else np.full((h, w), POISON, F32))

        pc, pf, pu, pv, po, out, wsum = plane(centre), plane(frames[0]), plane(us[0]), plane(vs[0]), plane(occs[0]), plane(), plane()
        ctx.denoise(pc, [pf], [pu], [pv], w, h, out, [po], 12.5, wsum)
        ctx.synchronize()
        got = [out.download(w, h), wsum.download(w, h)]
        for p in (pc, pf, out, wsum):
            p.free()
        # the composition: (pu, pv) scaled down as the first step, a second flow and both masks
        planes = [plane(a) for a in case]
        outs = [plane() for _ in range(3)]
        ctx.compose_flow(*planes[:4], w, h, outs[0], outs[1], planes[4], planes[5], outs[2])
        ctx.synchronize()
        got += [o.download(w, h) for o in outs]
        for p in planes + outs + [pu, pv, po]:
            p.free()
        runs.append(got)
    for got, kind in zip(runs, ("4 GiB planes", "planes just below 4 GiB")):
        assert_same(got[0], want, "denoise, %s" % kind)
        assert_same(got[1], want_sum, "denoise, %s: weight_sum" % kind)
        for g, x, name in zip(got[2:], cwant, ("u", "v", "mask")):
            assert_same(g, x, "compose, %s: %s" % (kind, name))
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes(), "the run on planes just below 4 GiB differs from the run on planes of 4 GiB"
