"""The 64-bit-offset instantiations behind flow2d::launch_by_span (csrc/plane_sample.hpp) and the generic median kernel behind
median.hip's offsets_fit, on planes that span 4 GiB and more: a frame of 100 x 4200 pixels in planes with a pitch of 1 MiB, as in
test_gpu_denoise.py::test_planes_of_4_gib_and_more, so the byte offset of row 4096 is 2^32 and a 32-bit intermediate anywhere wraps
row 4096 + k onto row k.  Only the frame's columns of a plane are ever touched (inputs uploaded, outputs poisoned there).

And the 32-bit forms of the same entries in the upper half of their range: the same frame in "high" planes with a pitch of 255 616
floats, 4 294 348 800 bytes a plane -- below 2^32, so every entry takes its `unsigned` instantiation and the medians their streaming
kernels -- where the byte offset of row 2101 is 2 148 196 864 >= 2^31: a signed intermediate addresses memory below the plane from
there on, and a shift or a mask that drops bit 31 reads row k for row 2101 + k.

Every entry is held to the restatement and the checker of its own GPU test, with that test's tolerances, and runs a second time on
high planes and a third time on the same data in planes with a pitch of 512 bytes (the 32-bit instantiation far below 2^31): the
three runs' outputs and records are the same bytes.  Before a device result is looked at, the inputs and the expected outputs are
shown to make a wrap visible at either line (4095 | 4096 of the tall planes, 2100 | 2101 of the high ones): the rows from the line
on differ from rows 0 .., the expected rows from the line on are live, what gathers does so across the line in both directions, and
what reduces to a record gives another record for the rows 0 .. 4095 alone."""
import numpy as np
import pytest

from test_bidirectional_cpu import consistency_reference
from test_correlate_cpu import F32, RECORD_DTYPE, U32, bits, correlate_reference, expand_reference, frame_range, grid, random_frames, scenes_module
from test_deformation_cpu import GREEN, PLANES as STRAIN_PLANES, SMALL, STATS_DTYPE, deformation_reference, masked_case
from test_flow_error_cpu import flow_error_reference
from test_global_motion_cpu import AFFINE, fit_case, global_flow_reference, global_motion_reference, warp_global_reference
from test_gpu_bidirectional import random_flows
from test_gpu_deformation import check_record as check_deformation_record, record_of as deformation_record_of
from test_gpu_denoise import assert_same
from test_gpu_flow_error import check_record as check_flow_error_record, random_case as flow_error_case
from test_gpu_global_motion import check_record as check_motion_record
from test_gpu_interpolation import random_case as interpolation_case, want_of as interpolation_want
from test_gpu_multipass import POISON
from test_gpu_prior import level_frames, restatement as prior_restatement, special_prior
from test_gpu_propagate import frames as propagate_frames, specials as propagate_specials
from test_gpu_subset import compare
from test_gpu_subset2 import OUT_NAMES as OUT_NAMES2, compare2
from test_gpu_subset_masked import same_bytes
from test_multipass_cpu import PASS_DTYPE, correlate_offset_reference
from test_propagate_cpu import RECORD_FIELDS as PROPAGATE_FIELDS, propagate_reference
from test_refine_cpu import RECORD_DTYPE as REFINE_DTYPE, random_case as refine_case, refine_reference
from test_subset2_cpu import all_orders2
from test_subset_cpu import all_orders
from test_subset_masked_cpu import default_min_pixels, random_mask, subset_refine_masked_reference
from test_subset_sequence_cpu import all_orders_from

pytestmark = pytest.mark.gpu

W, H = 100, 4200          # the frame: two 64-column tiles, 104 rows past the line
WIDE = 262144             # floats per row of a tall plane: a pitch of exactly 1 MiB
HIGH = 255616             # floats per row of a high plane: a pitch of 1 022 464 bytes, 4200 rows of it just below 4 GiB
NARROW = 128              # floats per row of an ordinary plane: a pitch of 512 bytes
PITCH = {"tall": WIDE, "high": HIGH, "ordinary": NARROW}
KINDS = ("tall", "high", "ordinary")
LINE = (1 << 32) // (4 * WIDE)  # 4096: the first row of a tall plane whose byte offset does not fit 32 bits
HIGH_LINE = -(-(1 << 31) // (4 * HIGH))  # 2101: the first row of a high plane whose byte offset has bit 31 set
LINES = (LINE, HIGH_LINE)
TALL_BYTES = 4 * WIDE * H
HIGH_BYTES = 4 * HIGH * H
assert (4 * HIGH, HIGH_BYTES, HIGH_LINE, 4 * HIGH * HIGH_LINE) == (1022464, 4294348800, 2101, 2148196864)
assert HIGH_BYTES < 1 << 32 and 4 * HIGH * (HIGH_LINE - 1) + 4 * W < 1 << 31 <= 4 * HIGH * HIGH_LINE  # (the frame's columns of row 2100 lie below 2^31)
# the node grid of the subset kernels: centres 10 + 16 j, so row 255 (cy = 4090) lies below the line and row 256 (cy = 4106) beyond it;
# rows 130 (cy = 2090) and 131 (cy = 2106) lie on either side of the high planes' line
GRID_R, GRID_S = 10, 16


# ---- planes ---------------------------------------------------------------------------------------------------------------------------
class Rig:
    """The planes of one run: tall (pitch 1 MiB), high (pitch 1 022 464 bytes) or ordinary (pitch 512 bytes).  `peak` tall or high
    planes are alive at most."""

    def __init__(self, ctx, kind, peak):
        self.ctx, self.kind, self.tall, self.held = ctx, kind, kind == "tall", []
        if kind != "ordinary":
            free, total = ctx.mem_info()
            need = peak * TALL_BYTES + (1 << 30)
            if need > free:
                pytest.fail("%d planes of %d bytes and 1 GiB of slack need %d bytes; the device has %d free of %d" % (peak, TALL_BYTES, need, free, total))

    def load(self, a, rows=H):
        """A plane of `rows` rows with `a` in its first columns; nothing else of it is touched."""
        if a is None:
            return None
        p = self.ctx.plane(PITCH[self.kind], rows)
        assert p.pitch == 4 * PITCH[self.kind]  # (the allocator leaves these pitches as they are: multiples of 256 bytes)
        if self.tall and rows == H:
            assert p.pitch * rows >= 1 << 32
        if self.kind == "high" and rows == H:
            assert 1 << 31 < p.pitch * (rows - 1) and p.pitch * rows == HIGH_BYTES < 1 << 32
        self.held.append(p)
        return p.upload(a)

    def out(self, w=W, rows=H, plane_rows=None):
        return self.load(np.full((rows, w), POISON, U32).view(F32), plane_rows or rows)

    def poison(self, planes, w=W, rows=H):
        for p in planes:
            p.upload(np.full((rows, w), POISON, U32).view(F32))

    def free(self, planes=None):
        for p in list(self.held if planes is None else planes):
            if p is not None:
                p.free()
                self.held.remove(p)
                self.ctx._planes.remove(p)


def on_both(ctx, peak, run):
    """run(rig) -> {name: array or bytes} on tall planes, then on high planes, then on ordinary ones: the same bytes.  Returns the tall
    run's result."""
    got = []
    for kind in KINDS:
        rig = Rig(ctx, kind, peak)
        try:
            got.append(run(rig))
            ctx.synchronize()
        finally:
            rig.free()
    assert got[0].keys() == got[1].keys() == got[2].keys()
    for name in got[0]:
        a, b, c = (g[name] if isinstance(g[name], bytes) else np.ascontiguousarray(g[name]).tobytes() for g in got)
        assert a == c, "%s: the run on planes of 4 GiB differs from the run on ordinary planes" % name
        assert b == c, "%s: the run on planes just below 4 GiB differs from the run on ordinary planes" % name
    return got[0]


def record_bytes(plane, count):
    return plane.download(count // 4, 1).tobytes()


# ---- what makes a wrap visible (the reference alone) --------------------------------------------------------------------------------
def wrapped_rows_differ(*arrays, h=H):
    """Rows 4096 .. of every input are not rows 0 .. again, and neither are rows 2101 .. ."""
    for a in arrays:
        if a is not None:
            for line in LINES:
                assert not np.array_equal(bits(a[line:h]), bits(a[:h - line]))


def live(*arrays, invalid=None):
    """The expected rows from 4096 on, and those from 2101 on: finite values, more than one of them, beyond `invalid` too, and not
    those of rows 0 .. ."""
    for a in arrays:
        a = np.asarray(a)
        for line in LINES:
            top = a[line:]
            values = top[np.isfinite(top)]
            if invalid is not None:
                values = values[values != invalid]
            assert values.size and np.unique(values).size > 1
            assert not np.array_equal(top.tobytes(), a[:a.shape[0] - line].tobytes())


def crosses_the_line(v, u=None, scale=1.0):
    """Some pixel below the line points (by its vertical component times `scale`) to a row of the frame from 4096 on, some pixel from
    4096 on to a row of the frame below 4095: a gather along these vectors reads across the line in both directions.  The same at
    the line 2100 | 2101."""
    ys, xs = np.mgrid[0:v.shape[0], 0:v.shape[1]]
    with np.errstate(invalid="ignore", over="ignore"):
        ty = ys + scale * v.astype(np.float64)
        tx = xs + scale * (u.astype(np.float64) if u is not None else 0.0)
        inside = (tx >= 0) & (tx <= v.shape[1] - 1) & (ty >= 0) & (ty <= v.shape[0] - 1)
        for line in LINES:
            assert (inside & (ys < line) & (ty >= line)).any() and (inside & (ys >= line) & (ty < line - 1)).any()


# ---- per-pixel entries ---------------------------------------------------------------------------------------------------------------
def test_consistency(flow2d, ctx):
    """flow2d_consistency_2d: consistency_kernel<size_t>.  Five tall planes."""
    flows = random_flows(np.random.default_rng(41), W, H)
    want = consistency_reference(*flows)
    wrapped_rows_differ(*flows)
    live(want)
    crosses_the_line(flows[1], flows[0])

    def run(rig):
        planes, out = [rig.load(a) for a in flows], rig.out()
        ctx.consistency(*planes, W, H, out)
        ctx.synchronize()
        return {"mask": out.download(W, H)}

    got = on_both(ctx, 5, run)["mask"]
    assert np.array_equal(got, want), "%d of %d pixels differ" % ((got != want).sum(), W * H)


def test_interpolate(flow2d, ctx):
    """flow2d_interpolate_2d with both masks and with none: interpolate_kernel<size_t> of either template.  Nine tall planes."""
    case = interpolation_case(np.random.default_rng(42), W, H)
    want = {masks: interpolation_want(case, 0.25, 2, masks=masks) for masks in ((True, True), (False, False))}
    wrapped_rows_differ(*case)
    live(*want.values())
    crosses_the_line(case[3], case[2], 0.25)
    crosses_the_line(case[5], case[4], 0.75)

    def run(rig):
        planes, out = [rig.load(a) for a in case], rig.out()
        got = {}
        for masks in want:
            rig.poison([out])
            ctx.interpolate(*planes[:6], W, H, 0.25, out, planes[6] if masks[0] else None, planes[7] if masks[1] else None, 2, 0.5)
            ctx.synchronize()
            got["masks=%s" % (masks,)] = out.download(W, H)
        return got

    got = on_both(ctx, 9, run)
    for masks in want:
        assert_same(got["masks=%s" % (masks,)], want[masks], "interpolate, 4 GiB planes, masks=%s" % (masks,))


@pytest.mark.parametrize("with_mask", [False, True])
def test_flow_error(flow2d, ctx, with_mask):
    """flow2d_flow_error_2d with and without the occlusion mask: flow_error_partials_kernel<size_t> of either template.  Seven tall
    planes.  (This kernel's per-lane offsets count floats, not bytes: at 4.1 GiB they stay below 2^32, so its `unsigned` instantiation
    would give these results too -- the test runs the 64-bit code and would see a 32-bit byte offset in it, while an offset in floats
    wraps only from 16 GiB on.)"""
    u, v, gu, gv, occ = flow_error_case(np.random.default_rng(43 + with_mask), W, H, with_mask)
    want, we, wa = flow_error_reference(u, v, gu, gv, occ)
    wrapped_rows_differ(u, v, gu, gv, occ)
    live(we)
    below = flow_error_reference(u[:LINE], v[:LINE], gu[:LINE], gv[:LINE], None if occ is None else occ[:LINE])[0]
    assert below["all"]["count"] != want["all"]["count"] and below["all"]["sum_epe"] != want["all"]["sum_epe"]

    held = []

    def run(rig):
        planes = [rig.load(a) for a in (u, v, gu, gv, occ)]
        epe, ae = rig.out(), rig.out()
        held.append(ctx.flow_error(*planes[:4], W, H, occlusion=planes[4], epe=epe, ae=ae)[0])
        return {"record": repr(held[-1]).encode(), "epe": epe.download(W, H), "ae": ae.download(W, H)}

    got = on_both(ctx, 7, run)
    e, a = got["epe"], got["ae"]
    assert np.array_equal(e, we, equal_nan=True), "%d EPE pixels differ" % (~((e == we) | (np.isnan(e) & np.isnan(we)))).sum()
    assert np.array_equal(np.isnan(a), np.isnan(wa))
    ok = ~np.isnan(wa)
    assert np.abs(a[ok] - wa[ok]).max(initial=0) <= 1e-4
    take = ~np.isnan(we)
    occluded = np.zeros_like(take) if occ is None else occ != 0
    check_flow_error_record(held[0], want, a, {"all": take, "noc": take & ~occluded, "occ": take & occluded})


def test_global_motion(flow2d, ctx):
    """flow2d_global_motion_2d, robust (sigma 0.5, two reweighted passes): motion_partials_kernel<size_t> without and with the previous
    pass's record.  Three tall planes.  (Offsets in floats, as in flow_error: see test_flow_error.)"""
    u, v, masks = fit_case(W, H)
    mask = masks["soft"]
    want = global_motion_reference(u, v, mask, AFFINE, 0.5, 2)
    wrapped_rows_differ(u, v, mask)
    below = global_motion_reference(u[:LINE], v[:LINE], mask[:LINE], AFFINE, 0.5, 2)
    assert below["support"] != want["support"] and below["weight_sum"] != want["weight_sum"]
    held = []

    def run(rig):
        pu, pv, pm = rig.load(u), rig.load(v), rig.load(mask)
        rec = ctx.global_motion(pu, pv, W, H, AFFINE, 0.5, 2, pm)[0]
        held.append(rec)
        return {"record": bytes(rec)}

    on_both(ctx, 3, run)
    check_motion_record(held[0], want, "100x4200, 4 GiB planes")


MOTION = [0.4, 0.01, -0.005, -0.3, 0.2, 0.0005]  # near the line the model's vertical component runs from -9 to +11 pixels across the columns


def test_global_flow(flow2d, ctx):
    """flow2d_global_flow_2d with every output: global_flow_kernel<size_t>.  Eight tall planes."""
    u, v, masks = fit_case(W, H)
    mask = masks["soft"]
    motion = ctx.upload_motion([flow2d.GlobalMotion.from_parameters(MOTION)])
    p = ctx.read_motion(motion)[0].parameters
    names = ("model_u", "model_v", "residual_u", "residual_v", "weight")
    want = global_flow_reference(p, (H, W), u, v, mask, 0.5)
    wrapped_rows_differ(u, v, mask)
    live(*[want[n] for n in names])

    def run(rig):
        pu, pv, pm = rig.load(u), rig.load(v), rig.load(mask)
        outs = [rig.out() for _ in names]
        ctx.global_flow(motion, W, H, pu, pv, pm, 0.5, *outs)
        ctx.synchronize()
        return {n: o.download(W, H) for n, o in zip(names, outs)}

    got = on_both(ctx, 8, run)
    for n in names:
        assert_same(got[n], want[n], "global_flow, 4 GiB planes: %s" % n)


def test_warp_global(flow2d, ctx):
    """flow2d_warp_global_2d with and without `valid`: warp_global_kernel<size_t>.  Four tall planes."""
    frame = np.random.default_rng(45).uniform(1, 255, (H, W)).astype(F32)
    motion = ctx.upload_motion([flow2d.GlobalMotion.from_parameters(MOTION)])
    p = ctx.read_motion(motion)[0].parameters
    want_out, want_valid = warp_global_reference(p, frame, -7.0)
    wrapped_rows_differ(frame)
    live(want_out, invalid=F32(-7.0))
    live(want_valid)
    model_v = global_flow_reference(p, (H, W))["model_v"]
    crosses_the_line(model_v, global_flow_reference(p, (H, W))["model_u"])

    def run(rig):
        pf, out, valid, lone = rig.load(frame), rig.out(), rig.out(), rig.out()
        ctx.warp_global(motion, pf, W, H, out, valid, fill=-7.0)
        ctx.warp_global(motion, pf, W, H, lone, fill=-7.0)
        ctx.synchronize()
        return {"out": out.download(W, H), "valid": valid.download(W, H), "lone": lone.download(W, H)}

    got = on_both(ctx, 4, run)
    assert_same(got["out"], want_out, "warp, 4 GiB planes")
    assert_same(got["valid"], want_valid, "warp, 4 GiB planes: valid")
    assert_same(got["lone"], want_out, "warp without valid, 4 GiB planes")


def test_deformation(flow2d, ctx):
    """flow2d_deformation_2d with its record (small strain) and without (Green-Lagrange): deformation_kernel<size_t> of either
    template.  Twelve tall planes."""
    u, v, mask = masked_case(W, H, soft=True)
    ref = {SMALL: deformation_reference(u, v, mask, SMALL), GREEN: deformation_reference(u, v, mask, GREEN)}
    wrapped_rows_differ(u, v, mask)
    for measure in ref:
        live(*[ref[measure][n] for n in STRAIN_PLANES])
    below = deformation_reference(u[:LINE], v[:LINE], mask[:LINE], SMALL)["stats"][0]
    assert below["valid"] != ref[SMALL]["stats"][0]["valid"] and below["e1"]["sum"] != ref[SMALL]["stats"][0]["e1"]["sum"]

    def run(rig):
        pu, pv, pm = rig.load(u), rig.load(v), rig.load(mask)
        outs = {n: rig.out() for n in STRAIN_PLANES}
        record = ctx.deformation_records().fill_bytes(0x7F)
        got = {}
        for measure, stats in ((SMALL, record), (GREEN, None)):
            rig.poison(outs.values())
            ctx.deformation(pu, pv, W, H, measure, mask=pm, planes=outs, stats=stats)
            ctx.synchronize()
            got.update({"%s %d" % (n, measure): o.download(W, H) for n, o in outs.items()})
        got["record"] = deformation_record_of(ctx, record).tobytes()
        return got

    got = on_both(ctx, 12, run)
    for measure in ref:
        for n in STRAIN_PLANES:
            assert np.array_equal(bits(got["%s %d" % (n, measure)]), bits(ref[measure][n])), "measure %d: %s" % (measure, n)
    check_deformation_record(np.frombuffer(got["record"], STATS_DTYPE)[0], ref[SMALL], "100x4200, 4 GiB planes")


@pytest.mark.parametrize("r,on,w", [(1, True, W), (3, True, 66), (1, False, W)])
def test_refine_flow(flow2d, ctx, r, on, w):
    """flow2d_refine_flow_2d: the `wide` launch of the radius units 1 and 3 with guide, mask and spatial weight, and of unit 1 with
    none of them.  Six tall planes; a window of radius r around the rows 4096 - r .. 4095 + r holds rows of both sides.  The radius 3
    runs at 66 columns: its restatement sorts 49 samples a pixel, 6.5 s at 100 columns."""
    u, v, guide, mask = refine_case(w, H)
    sg, ss = (30.0, 2.5) if on else (0.0, 0.0)
    wu, wv, record = refine_reference(u, v, guide if on else None, mask if on else None, r, sg, ss)
    wrapped_rows_differ(u, v, guide, mask)
    live(wu, wv)
    if r == 1:
        below = refine_reference(u[:LINE], v[:LINE], guide[:LINE] if on else None, mask[:LINE] if on else None, r, sg, ss)[2]
        assert below["pixels"] != record["pixels"] and below["changed"] != record["changed"]
    else:  # (not restated a second time: the counts are sums over the pixels, and the rows beyond the line add to every one asked for)
        changed = (bits(wu) != bits(u)) | (bits(wv) != bits(v))
        assert changed[LINE:].any() and not changed[LINE:].all() and record["changed"] == changed.sum() and record["filled"] > 0

    def run(rig):
        pu, pv = rig.load(u), rig.load(v)
        pg, pm = (rig.load(guide), rig.load(mask)) if on else (None, None)
        ou, ov = rig.out(w), rig.out(w)
        rec = ctx.refine_records().fill_bytes(0x7F)
        ctx.refine_flow(pu, pv, w, H, r, pg, pm, sg, ss, ou, ov, rec)
        ctx.synchronize()
        return {"u": ou.download(w, H), "v": ov.download(w, H), "record": record_bytes(rec, 32)}

    got = on_both(ctx, 6, run)
    for g, want, name in ((got["u"], wu, "u"), (got["v"], wv, "v")):
        same = bits(g) == bits(want)
        assert same.all(), "%s differs at %d pixels, first (y, x) = %s" % (name, (~same).sum(), np.argwhere(~same)[0])
    assert got["record"] == record.tobytes(), "record %s, want %s" % (np.frombuffer(got["record"], REFINE_DTYPE), record)


def test_prior_registration(flow2d, ctx):
    """flow2d_prior_registration_2d with a prior of 100 x 4200 and a level of 96 x 4000 in the same pitch: the level's planes stay below
    4 GiB and prior_bytes alone selects prior_registration_kernel<size_t>.  Two tall planes and five of 4000 rows.  The level's rows from
    3901 on are resampled from prior rows from 4096 on."""
    (in_w, in_h), (w, h) = (W, H), (96, 4000)
    pu, pv = special_prior(in_w, in_h, w, h, 46)
    pu[4150, 7], pv[4120, 50] = np.nan, np.inf  # counted only if the prior's rows beyond the line are read
    f0, f1 = level_frames(w, h, 46)
    want_u, want_v, want_out, count, hx, hy = prior_restatement(pu, pv, f0, f1, w, h)
    first = -((-LINE * h) // in_h)  # the first level row that reads prior rows from 4096 on only
    assert 4 * WIDE * h < 1 << 32 <= 4 * WIDE * in_h and first < h - 64
    wrapped_rows_differ(pu, pv)
    first_high = -((-HIGH_LINE * h) // in_h)  # the same for prior rows from 2101 on, the high planes' line
    for a in (want_u, want_v, want_out):
        for start in (first, first_high):
            top = a[start:]
            assert np.isfinite(top).all() and np.unique(top).size > 1 and not np.array_equal(top, a[:h - start])
    assert count >= 6 and count != prior_restatement(pu[:LINE], pv[:LINE], f0[:3900], f1[:3900], w, 3900)[3]
    held = []

    def run(rig):
        planes = [rig.load(pu), rig.load(pv), rig.load(f0, h), rig.load(f1, h)]
        outs = [rig.out(w, h) for _ in range(3)]
        held.append(ctx.prior_registration(planes[0], planes[1], in_w, in_h, outs[0], outs[1], planes[2], planes[3], w, h, float(hx), float(hy), outs[2]))
        return {"count": str(held[-1]).encode(), "out_u": outs[0].download(w, h), "out_v": outs[1].download(w, h), "output": outs[2].download(w, h)}

    got = on_both(ctx, 7, run)
    for name, want in (("out_u", want_u), ("out_v", want_v), ("output", want_out)):
        same = bits(got[name]) == bits(want)
        assert same.all(), "%s differs at %d places, first (y, x) = %s" % (name, (~same).sum(), np.argwhere(~same)[0])
    assert held[0] == count


def test_propagate_flow(flow2d, ctx):
    """flow2d_propagate_flow_2d with mask, frames and two fill passes: the splat, resolve and fill kernels' <size_t> instantiations.
    Seven tall planes; the workspace and the record are ordinary allocations."""
    u, v, mask = propagate_specials(W, H, 47)
    f0, f1 = propagate_frames(W, H, 48)
    kw = dict(u=u, v=v, mask=mask, frame_from=f0, frame_to=f1, photo_scale=3.0, fill_passes=2)
    want_u, want_v, want_rec = propagate_reference(**kw)
    wrapped_rows_differ(u, v, mask, f0, f1)
    live(want_u, want_v)
    crosses_the_line(v, u)
    assert want_rec["filled"] > 0
    below = propagate_reference(**{k: (a[:LINE] if isinstance(a, np.ndarray) else a) for k, a in kw.items()})[2]
    assert below["landed"] != want_rec["landed"] and below["filled"] != want_rec["filled"]
    held = []

    def run(rig):
        planes = [rig.load(a) for a in (u, v, mask, f0, f1)]
        ou, ov = rig.out(), rig.out()
        _, _, rec = ctx.propagate_flow(planes[0], planes[1], W, H, mask=planes[2], frame_from=planes[3], frame_to=planes[4], step=1.0,
                                       photo_scale=3.0, fill_passes=2, out_u=ou, out_v=ov)
        held.append(rec)
        return {"u": ou.download(W, H), "v": ov.download(W, H), "record": bytes(rec)}

    got = on_both(ctx, 7, run)
    for g, want, name in ((got["u"], want_u, "u"), (got["v"], want_v, "v")):
        same = bits(g) == bits(want)
        assert same.all(), "%s differs at %d places, first (y, x) = %s" % (name, (~same).sum(), np.argwhere(~same)[0])
    rec = held[0]
    assert {k: getattr(rec, k) for k in PROPAGATE_FIELDS} == want_rec and rec.reserved == 0
    assert rec.pixels == W * H == rec.unusable + rec.left + rec.landed


# ---- the generic median kernel behind offsets_fit ------------------------------------------------------------------------------------
def test_median(flow2d, ctx, oracle):
    """flow2d_median_2d for the windows 3, 5 and 7 and flow2d_add_median_2d_pair on planes of 4 GiB: median.hip's offsets_fit sends
    them to the generic kernel (a streaming kernel's 32-bit byte offsets would give rows 0 .. 103 from row 4096 on); the ordinary
    planes of the third run take the streaming kernels far below 2^31, and the high planes of the second run take them with byte
    offsets up to 2^32: a streaming kernel that dropped bit 31 would give rows 0 .. from row 2101 on.  Six tall planes; 66 columns and the pair form at window 5 alone keep the
    oracle's share of the time down."""
    w = 66
    rng = np.random.default_rng(49)
    u, v = (rng.normal(0, 1, (H, w)).astype(F32) for _ in range(2))
    du, dv = (rng.normal(0, 0.3, (H, w)).astype(F32) for _ in range(2))
    u[::3, ::5] = 0.0  # ties
    du[rng.random((H, w)) < 0.02] = np.nan
    wrapped_rows_differ(u, v, du, dv)
    want = {"median %d" % window: oracle.median(u, w, H, window) for window in (3, 5, 7)}
    want["add_median u"] = oracle.median(oracle.add(u, du, w, H), w, H, 5)
    want["add_median v"] = oracle.median(oracle.add(v, dv, w, H), w, H, 5)
    live(*want.values())

    def run(rig):
        pu, pdu, pv, pdv, ou, ov = [rig.load(a) for a in (u, du, v, dv)] + [rig.out(w), rig.out(w)]
        got = {}
        for window in (3, 5, 7):
            rig.poison([ou], w)
            ctx.median(pu, w, H, window, ou)
            ctx.synchronize()
            got["median %d" % window] = ou.download(w, H)
        rig.poison([ou, ov], w)
        ctx.add_median(pu, pdu, w, H, 5, ou, pv, pdv, ov)
        ctx.synchronize()
        got["add_median u"], got["add_median v"] = ou.download(w, H), ov.download(w, H)
        return got

    got = on_both(ctx, 6, run)
    for name, x in want.items():
        assert np.array_equal(bits(got[name]), bits(x)), name


# ---- the correlators ------------------------------------------------------------------------------------------------------------------
def node_poison(ctx, nw, nh, count):
    return [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F) for _ in range(count)]


def node_bits(planes, nw, nh):
    """The grids of node planes (None: absent) as bits; nothing beyond a grid was written."""
    out = []
    for q in planes:
        g = q.download().view(U32)
        assert (g[nh:] == POISON).all() and (g[:, nw:] == POISON).all(), "written beyond the grid"
        out.append(g[:nh, :nw])
    return out


def release(ctx, planes):
    for q in planes:
        q.free()
        ctx._planes.remove(q)


def straddling_and_beyond(cy, reach, line=LINE):
    """Of the node rows with centres `cy` and rows cy - reach .. cy + reach: (those below the line that reach rows from `line` on,
    those from the line on that reach rows below it, those wholly beyond it)."""
    down = (cy < line) & (cy + reach >= line)
    up = (cy >= line) & (cy - reach < line)
    return down, up, cy - reach >= line


def test_correlate_and_expand(flow2d, ctx):
    """flow2d_correlate_2d on tall frames, then flow2d_expand_nodes_2d of its nodes into tall dense planes: correlate_kernel<size_t> and
    expand_kernel<size_t>.  Grid (15, s 16) with range 3: the window of node row 255 is rows 4080 .. 4110, the search of row 256
    starts at row 4093.  Four tall planes; the node planes are ordinary."""
    r, d, s = 15, 3, 16
    f0, f1 = random_frames(W, H, seed=50, shift=(2, -1))
    lo, scale = frame_range(f0, f1)
    wu, wv, ws, record, _ = correlate_reference(f0, f1, lo, scale, r, d, s)
    eu, ev = expand_reference(wu, wv, r, s, W, H)
    nw, nh = grid(W, H, r, s)
    cy = r + np.arange(nh) * s
    wrapped_rows_differ(f0, f1)
    for line in LINES:
        for rows in straddling_and_beyond(cy, r + d, line):
            assert rows.any() and np.isfinite(wu[rows]).all() and np.unique(wu[rows]).size > 1
    live(eu, ev)
    assert correlate_reference(f0[:LINE], f1[:LINE], lo, scale, r, d, s)[3].tobytes() != record.tobytes()

    def run(rig):
        p0, p1, du, dv = rig.load(f0), rig.load(f1), rig.out(), rig.out()
        nodes, rec = node_poison(ctx, nw, nh, 3), ctx.correlation_records().fill_bytes(0x7F)
        ctx.correlate(p0, p1, W, H, lo, scale, r, d, s, -1.0, nodes[0], nodes[1], nodes[2], rec)
        ctx.expand_nodes(nodes[0], nodes[1], nw, nh, r, s, du, dv, W, H)
        ctx.synchronize()
        gu, gv, gs = node_bits(nodes, nw, nh)
        got = {"u": gu, "v": gv, "score": gs, "record": record_bytes(rec, 32), "expanded u": bits(du.download(W, H)), "expanded v": bits(dv.download(W, H))}
        release(ctx, nodes + [rec])
        return got

    got = on_both(ctx, 4, run)
    for name, want in (("u", wu), ("v", wv), ("score", ws), ("expanded u", eu), ("expanded v", ev)):
        same = got[name] == bits(want)
        assert same.all(), "%s differs at %d places, first (y, x) = %s" % (name, (~same).sum(), np.argwhere(~same)[0])
    assert got["record"] == record.tobytes(), "record %s, want %s" % (np.frombuffer(got["record"], RECORD_DTYPE), record)


def test_expand_nodes_into_tall_planes(flow2d, ctx):
    """flow2d_expand_nodes_2d where the dense planes alone are tall: a node field with invalid nodes, grid (10, s 64).  Two tall planes."""
    r, s = 10, 64
    nw, nh = grid(W, H, r, s)
    rng = np.random.default_rng(51)
    nu, nv = (rng.normal(0, 3, (nh, nw)).astype(F32) for _ in range(2))
    nu[3, 0], nv[nh - 2, 1], nu[nh - 1, :] = np.nan, np.inf, np.nan
    eu, ev = expand_reference(nu, nv, r, s, W, H)
    assert nh == 66 and r + (nh - 2) * s >= LINE and r + 32 * s < HIGH_LINE <= r + 33 * s
    live(eu, ev)

    def run(rig):
        du, dv = rig.out(), rig.out()
        nodes = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F).upload(a) for a in (nu, nv)]
        ctx.expand_nodes(nodes[0], nodes[1], nw, nh, r, s, du, dv, W, H)
        ctx.synchronize()
        got = {"u": bits(du.download(W, H)), "v": bits(dv.download(W, H))}
        release(ctx, nodes)
        return got

    got = on_both(ctx, 2, run)
    for name, want in (("u", eu), ("v", ev)):
        same = got[name] == bits(want)
        assert same.all(), "%s differs at %d places, first (y, x) = %s" % (name, (~same).sum(), np.argwhere(~same)[0])


def test_correlate_offset(flow2d, ctx):
    """flow2d_correlate_offset_2d with a dense predictor: correlate_offset_kernel<size_t>.  Grid (10, s 64), range 3: node row 63 (rows
    4032 .. 4052) is sent 50 rows down, across the line; row 64 (rows 4096 .. 4116) six rows up, across it; row 65 lies beyond.  At
    the high planes' line node row 32 (rows 2048 .. 2068) is sent 50 rows down, row 33 (rows 2112 .. 2132) twenty rows up, and row 34
    lies beyond.  Four tall planes."""
    r, d, s = 10, 3, 64
    f0, f1 = random_frames(W, H, seed=52, shift=(2, -1))
    lo, scale = frame_range(f0, f1)
    nw, nh = grid(W, H, r, s)
    cy = r + np.arange(nh) * s
    rng = np.random.default_rng(53)
    pu, pv = (rng.uniform(-3, 3, (H, W)).astype(F32) for _ in range(2))
    pv[cy[63] - 2:cy[63] + 3], pv[cy[64] - 2:cy[64] + 3] = 50.0, -6.0
    pv[cy[32] - 2:cy[32] + 3], pv[cy[33] - 2:cy[33] + 3] = 50.0, -20.0
    wu, wv, ws, record = correlate_offset_reference(f0, f1, lo, scale, r, d, s, -1.0, pu, pv)
    wrapped_rows_differ(f0, f1, pu, pv)
    assert cy[63] < LINE <= cy[63] + r + 50 - d and cy[64] - r - 6 - d < LINE <= cy[64] and cy[65] - r - 3 - d >= LINE
    assert cy[32] < HIGH_LINE <= cy[32] + r + 50 - d and cy[33] - r - 20 - d < HIGH_LINE <= cy[33] - r and cy[34] - r - 3 - d >= HIGH_LINE
    for j in (63, 64, 65):
        assert np.isfinite(wu[j]).all() and np.isfinite(wv[j]).all() and not np.array_equal(wv[j], wv[j - 63])
    for j in (32, 33, 34):
        assert np.isfinite(wu[j]).all() and np.isfinite(wv[j]).all() and not np.array_equal(wv[j], wv[j - 32])
    below = correlate_offset_reference(f0[:LINE], f1[:LINE], lo, scale, r, d, s, -1.0, pu[:LINE], pv[:LINE])[3]
    assert below.tobytes() != record.tobytes()

    def run(rig):
        planes = [rig.load(a) for a in (f0, f1, pu, pv)]
        nodes, rec = node_poison(ctx, nw, nh, 3), ctx.pass_records().fill_bytes(0x7F)
        ctx.correlate_offset(planes[0], planes[1], W, H, lo, scale, r, d, s, -1.0, (planes[2], planes[3]), nodes[0], nodes[1], nodes[2], rec)
        ctx.synchronize()
        gu, gv, gs = node_bits(nodes, nw, nh)
        got = {"u": gu, "v": gv, "score": gs, "record": record_bytes(rec, 64)}
        release(ctx, nodes + [rec])
        return got

    got = on_both(ctx, 4, run)
    for name, want in (("u", wu), ("v", wv), ("score", ws)):
        same = got[name] == bits(want)
        assert same.all(), "%s differs at %d places, first (y, x) = %s" % (name, (~same).sum(), np.argwhere(~same)[0])
    assert got["record"] == record.tobytes(), "record %s, want %s" % (np.frombuffer(got["record"], PASS_DTYPE), record)


# ---- the subset refinements -----------------------------------------------------------------------------------------------------------
_speckle = []
LIVE_ROWS = [0, 1, 100, 130, 131, 132, 254, 255, 256, 257, 258]  # the node rows that have a start; every other node is SUBSET_NO_INPUT


def speckle_case():
    """The translated speckle pattern at 100 x 4200 and the start of the grid (10, s 16), 5 x 262 nodes: the truth (2.3, -1.4) rounded
    to whole pixels in the node rows LIVE_ROWS, NaN in every other, which keeps the restatement to fifty-five nodes.  Made once."""
    if not _speckle:
        scene = scenes_module().make_speckle_scene("translation", W, H, seed=3)
        nw, nh = grid(W, H, GRID_R, GRID_S)
        u0, v0 = np.full((nh, nw), np.nan, F32), np.full((nh, nw), np.nan, F32)
        u0[LIVE_ROWS, :], v0[LIVE_ROWS, :] = 2.0, -1.0
        _speckle.append((scene.frame_0, scene.frame_1, u0, v0))
    return _speckle[0]


def subsets_show_a_wrap(want, R, f0, f1, reference_below):
    """The node rows 255 (cy = 4090) and 256 (cy = 4106): at R = 15 both subsets hold rows of both sides of the line, at R = 5 row 255
    reaches row 4096 with its gradient stencil; rows 257 and 258 lie wholly beyond the line.  All of them hold refined nodes, and the
    rows 0 .. 4095 alone give another record.  The node rows 130 (cy = 2090), 131 (cy = 2106) and 132 are the same to the line
    2100 | 2101 of the high planes: at R = 15 the subsets of rows 130 and 131 hold rows of both sides, at R = 5 row 131 reaches down
    to row 2100 and row 130 lies below the line; row 132 lies wholly beyond."""
    nh = want.state.shape[0]
    cy = GRID_R + np.arange(nh) * GRID_S
    down, up, beyond = straddling_and_beyond(cy, R + 1)
    assert down[255] and (up[256] or R < 15) and beyond[257] and beyond[258] and cy[258] + R + 2 < H
    down, up, beyond = straddling_and_beyond(cy, R + 1, HIGH_LINE)
    assert (down[130] or R < 15) and up[131] and beyond[132] and not beyond[131]
    for j in (130, 131, 132, 255, 256, 257, 258):
        assert (want.state[j] >= 1).any(), "no node of row %d converged" % j
    assert not np.array_equal(want.u[131:133], want.u[0:2]) and np.unique(want.u[131:133][want.state[131:133] >= 1]).size > 1
    assert not np.array_equal(want.u[256:259], want.u[0:3]) and np.unique(want.u[256:259][want.state[256:259] >= 1]).size > 1
    wrapped_rows_differ(f0, f1)
    assert reference_below.record.tobytes() != want.record.tobytes()


def below_the_line(a):
    """The node rows whose grid the frame's rows 0 .. 4095 alone have."""
    return a[:grid(W, LINE, GRID_R, GRID_S)[1]]


def subset_outputs(ctx, nw, nh, count):
    return node_poison(ctx, nw, nh, count), ctx.subset_records().fill_bytes(0x7F)


@pytest.mark.parametrize("R", [15, 5])
def test_subset_refine(flow2d, ctx, R):
    """flow2d_subset_refine_2d: subset_refine_kernel<size_t> at two waves per workgroup and sixteen pixels per lane (R = 15) and at four
    waves (R = 5).  Two tall planes."""
    f0, f1, u0, v0 = speckle_case()
    nh, nw = u0.shape
    want, spread = all_orders(f0, f1, u0, v0, GRID_R, GRID_S, R)
    subsets_show_a_wrap(want, R, f0, f1, all_orders(f0[:LINE], f1[:LINE], below_the_line(u0), below_the_line(v0), GRID_R, GRID_S, R)[0])

    def run(rig):
        p0, p1 = rig.load(f0), rig.load(f1)
        start = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F).upload(a) for a in (u0, v0)]
        outs, rec = subset_outputs(ctx, nw, nh, 8)
        ctx.subset_refine(p0, p1, W, H, start[0], start[1], nw, nh, GRID_R, GRID_S, R, 20, 1e-3, 2.0, 0.5, outs[0], outs[1], outs[2:6], outs[6], outs[7], rec)
        ctx.synchronize()
        got = dict(zip(("u", "v", "ux", "uy", "vx", "vy", "score", "state"), node_bits(outs, nw, nh)), record=record_bytes(rec, 64))
        release(ctx, start + outs + [rec])
        return got

    got = on_both(ctx, 2, run)
    compare(([got[n] for n in ("u", "v", "ux", "uy", "vx", "vy", "score", "state")], got["record"]), want, spread, "100x4200, R = %d, 4 GiB planes" % R)


def test_subset_refine_from(flow2d, ctx):
    """flow2d_subset_refine_from_2d with start gradients: subset_refine_kernel<size_t, SubsetStart>, R = 15.  Two tall planes."""
    R = 15
    f0, f1, u0, v0 = speckle_case()
    nh, nw = u0.shape
    rng = np.random.default_rng(54)
    start = [u0, v0] + [rng.uniform(-0.01, 0.01, (nh, nw)).astype(F32) for _ in range(4)]
    want, spread = all_orders_from(f0, f1, u0, v0, start[2:], GRID_R, GRID_S, R)
    subsets_show_a_wrap(want, R, f0, f1, all_orders_from(f0[:LINE], f1[:LINE], below_the_line(u0), below_the_line(v0),
                                                         [below_the_line(q) for q in start[2:]], GRID_R, GRID_S, R)[0])

    def run(rig):
        p0, p1 = rig.load(f0), rig.load(f1)
        held = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F).upload(a) for a in start]
        outs, rec = subset_outputs(ctx, nw, nh, 8)
        ctx.subset_refine_from(p0, p1, W, H, held[0], held[1], held[2:], nw, nh, GRID_R, GRID_S, R, 20, 1e-3, 4.0, 0.5, outs[0], outs[1], outs[2:6],
                               outs[6], outs[7], rec)
        ctx.synchronize()
        got = dict(zip(("u", "v", "ux", "uy", "vx", "vy", "score", "state"), node_bits(outs, nw, nh)), record=record_bytes(rec, 64))
        release(ctx, held + outs + [rec])
        return got

    got = on_both(ctx, 2, run)
    compare(([got[n] for n in ("u", "v", "ux", "uy", "vx", "vy", "score", "state")], got["record"]), want, spread, "100x4200 from a start, R = 15, 4 GiB planes")


def test_subset_refine2(flow2d, ctx):
    """flow2d_subset_refine2_2d: subset_refine2_kernel<size_t>, R = 15.  Two tall planes."""
    R = 15
    f0, f1, u0, v0 = speckle_case()
    nh, nw = u0.shape
    want, spread = all_orders2(f0, f1, u0, v0, GRID_R, GRID_S, R)
    subsets_show_a_wrap(want, R, f0, f1, all_orders2(f0[:LINE], f1[:LINE], below_the_line(u0), below_the_line(v0), GRID_R, GRID_S, R)[0])

    def run(rig):
        p0, p1 = rig.load(f0), rig.load(f1)
        start = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F).upload(a) for a in (u0, v0)]
        outs, rec = subset_outputs(ctx, nw, nh, 14)
        ctx.subset_refine2(p0, p1, W, H, start[0], start[1], nw, nh, GRID_R, GRID_S, R, 20, 1e-3, 2.0, 0.5, 0.05, None, None, outs[0], outs[1],
                           outs[2:6], outs[6:12], outs[12], outs[13], rec)
        ctx.synchronize()
        got = dict(zip(OUT_NAMES2, node_bits(outs, nw, nh)), record=record_bytes(rec, 64))
        release(ctx, start + outs + [rec])
        return got

    got = on_both(ctx, 2, run)
    compare2(({n: got[n] for n in OUT_NAMES2}, got["record"]), want, spread, "100x4200 second order, R = 15, 4 GiB planes")


def test_subset_refine_masked(flow2d, ctx):
    """flow2d_subset_refine_masked_2d with a tall mask that excludes a tenth of the pixels on both sides of the line:
    subset_refine_masked_kernel<size_t>, R = 15.  Three tall planes; every byte is the restatement's, as in test_gpu_subset_masked.py."""
    R = 15
    f0, f1, u0, v0 = speckle_case()
    nh, nw = u0.shape
    mask = random_mask(f0.shape, 0.1, seed=55)
    min_pixels = default_min_pixels(R)
    want = subset_refine_masked_reference(f0, f1, u0, v0, None, mask, min_pixels, GRID_R, GRID_S, R)
    below = subset_refine_masked_reference(f0[:LINE], f1[:LINE], below_the_line(u0), below_the_line(v0), None, mask[:LINE], min_pixels, GRID_R, GRID_S, R)
    subsets_show_a_wrap(want, R, f0, f1, below)
    wrapped_rows_differ(mask)
    assert (mask[LINE - 16:LINE] == 1).any() and (mask[LINE:LINE + 16] == 1).any()
    assert (mask[HIGH_LINE - 16:HIGH_LINE] == 1).any() and (mask[HIGH_LINE:HIGH_LINE + 16] == 1).any()

    def run(rig):
        p0, p1, pm = rig.load(f0), rig.load(f1), rig.load(mask)
        start = [ctx.plane(nw + 5, nh + 3).fill_bytes(0x7F).upload(a) for a in (u0, v0)]
        outs, rec = subset_outputs(ctx, nw, nh, 8)
        ctx.subset_refine_masked(p0, p1, W, H, start[0], start[1], None, nw, nh, GRID_R, GRID_S, R, pm, min_pixels, 20, 1e-3, 4.0, 0.5, outs[0],
                                 outs[1], outs[2:6], outs[6], outs[7], rec)
        ctx.synchronize()
        got = dict(zip(("u", "v", "ux", "uy", "vx", "vy", "score", "state"), node_bits(outs, nw, nh)), record=record_bytes(rec, 64))
        release(ctx, start + outs + [rec])
        return got

    got = on_both(ctx, 3, run)
    same_bytes(([got[n] for n in ("u", "v", "ux", "uy", "vx", "vy", "score", "state")], got["record"]), want, "100x4200 masked, R = 15, 4 GiB planes")
