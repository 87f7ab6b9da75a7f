"""The 32-bit-offset kernels in the upper half of their range, and the solver on either side of the 4 GiB line.

The strip solver (csrc/solve_fused_kernel.hpp), the streaming medians (csrc/median.hip) and the `unsigned` instantiation of every
kernel behind flow2d::launch_by_span (csrc/plane_sample.hpp) address a plane as a scalar base plus one unsigned 32-bit per-lane byte
offset, which their launchers (fused_addressable, offsets_fit, launch_by_span) allow for any plane with height * pitch_bytes < 2^32.
From byte 2^31 of a plane on three mistakes would pass every test on small planes: a signed intermediate (addresses memory below the
plane), a shift or mask that drops bit 31, and a sum that wraps before it is widened (both read row k for row 2048 + k).

Here the frame is 100 x 4095 in planes with a pitch of 1 MiB ("high" planes): height * pitch = 2^32 - 2^20, the rows from 2048 on
have bit 31 set in their byte offsets and the last row starts 1 MiB below 2^32.  Only the frame's columns of a plane are touched
(inputs uploaded, outputs poisoned there; tests/test_gpu_wide_planes.py's Rig), and no host array has a container's size.  Every
result is compared bit for bit with the CPU oracle and with the same call on planes with a pitch of 512 bytes; before a device
result is looked at, the inputs and the oracle's results are shown to differ between the rows from the line on and the rows they
would alias, and the oracle's rows from the line on to be finite and varied.  (LogDerivatives: the oracle is handed the device's
logarithms, oracle.device_logs, as in tests/test_gpu_log_derivatives.py, and is then held to every bit as well.)  The solver's
inputs are the finite random fields of tests/test_gpu_fused.py; the medians' have ties and NaNs as in test_gpu_wide_planes.py.

  test_strips_on_high_planes              flow2d_solve_level, FUSED, on the pipeline build and on the packed build (Build.served
                                          of tests/test_gpu_fused.py is the proof of which ran): Grey, Gradient, LogDerivatives at
                                          3 x 5, Grey at inner 2, red-black SOR (omega 1.5, inner 2), a half-size base flow
  test_tiles_and_sweeps_on_high_planes    TILED and PER_SWEEP requested on the same planes
  test_sweeps_beyond_the_line             100 x 4200 at a pitch of 1 MiB (4.1 GiB), AUTO: the per-sweep kernels, Grey and Gradient
  test_group_whose_span_passes_4_gib      three instances of 100 x 1390, 1400 MiB apart in one allocation of 4200 MiB a plane: the
                                          strips and flow2d_add_median_2d_pair; the second instance's base has bit 31 set, the
                                          batch span is beyond 4 GiB, each instance's plane is not
  test_pyramid_entries                    flow2d_gaussian_blur (streaming), flow2d_registration_2d, flow2d_upsample_registration_2d
                                          and its _half form, flow2d_add_2d_pair, flow2d_compute_phi_ksi, flow2d_resample_x_pair,
                                          flow2d_resample_y_pair on high planes (100 x 4095) and on planes of 4.1 GiB (100 x 4200)
The line itself (fused_addressable at height x pitch = 2^32) is tests/test_planning_cus_cpu.py's, on the host.

flow2d_upsample_registration_half_2d takes exactly doubled levels only and refuses 100 x 4095 with FLOW2D_ERR_UNSUPPORTED: the test
asserts the status and that nothing was written, and runs the entry at 100 x 4094 in the same planes instead.

Where a 32-bit byte offset is formed (read before the first run; every one is unsigned from its first multiplication on and is
widened to 64 bits, by the static_cast of plane_load / plane_store or by the pointer addition of load_at / store_at, after its last
32-bit addition):

  file                        function                                           offset type
  solve_fused_kernel.hpp      row_offset, uv_row_offset, strip_step `off`        unsigned (int row, pitch, column cast first)
  solve_fused_kernel.hpp      run_strip / strip_step uv_off += uv_step[]         unsigned + unsigned, below the plane's bytes
  solve_fused_kernel.hpp      run_strip `os` (CONT), blockIdx.z instance offset  size_t (in floats)
  median.hip                  base_byte_offset, load_row / 3 / 7 `line`, `at`    unsigned (row clamped to [0, h) before the cast)
  median.hip                  median3/5/7_step `at`, `at + pitch * 4u`           unsigned; second row only where ya + 1 < y1 <= h
  median.hip                  Source::at (generic kernel, exact_median)          size_t (in floats)
  plane_sample.hpp            pixel_offset<Offset>, make_tap                     Offset(y) * Offset(pitch) + Offset(x), then * 4
  consistency.hip             consistency_kernel `c`                             Offset, in floats (below 2^30 here)
  flow_error.hip              flow_error_partials_kernel `c`                     Offset, in floats
  global_motion.hip           motion_partials_kernel `c`; the other two kernels  Offset, in floats; pixel_offset<Offset>
  interpolate.hip, denoise.hip, deformation.hip, propagate.hip, prior.hip        pixel_offset<Offset> / make_tap<Offset>, clamped x, y
  correlate.hip, correlate_offset.hip, correlate_masked.hip                      pixel_offset<Offset>; frame 1 only where 0 <= g < w, h
  subset_sample.hpp, subset_node.hpp, subset_refine*.hip                         sample_at<Offset> -> pixel_offset<Offset>, clamped
  refine_kernel.hpp           refine_kernel `o`                                  pixel_offset<Offset> of clamped (xc, yc)
  bspline_prefilter.hip       stage load, store_at                               pixel_offset<Offset> of reflected indices
  solve.hip, solve_tile.hip, solve_small.hip, pyramid_ops.hip                    size_t throughout
No place was found signed, or widened too early or too late.

Not covered: offsets within a few KiB of 2^32, where an immediate folded into a `saddr` access could carry -- that takes a frame
about as wide as its pitch, a gigapixel through the CPU oracle; the closest this file gets is 1 MiB.  The node-grid kernels (their
grids are bounded by node_count_ok), tracking and segmentation (size_t slots, refused from 2^31 pixels on) are out of scope."""
import ctypes

import numpy as np
import pytest

from conftest import in_container, level_fields
from test_gpu_fused import Build
from test_gpu_wide_planes import F32, POISON, U32, WIDE, Rig, bits

pytestmark = pytest.mark.gpu

W, H = 100, 4095                  # the frame of the high planes: two strips of the solver, two 64-column tiles
TALL_H = 4200                     # the frame of the planes beyond the line
PITCH_BYTES = 4 * WIDE            # 1 MiB
HALF = (1 << 31) // PITCH_BYTES   # 2048: the first row whose byte offset has bit 31 set
LINE = (1 << 32) // PITCH_BYTES   # 4096: the first row whose byte offset does not fit 32 bits
assert H * PITCH_BYTES == (1 << 32) - (1 << 20) and (H - 1) * PITCH_BYTES == (1 << 32) - (1 << 21)
GREY, GRADIENT, LOG = 0, 1, 3
AUTO, PER_SWEEP, FUSED, TILED = 0, 1, 2, 4
UNSUPPORTED = 5
ALPHA, EPS, OUTER = 35.0, 0.001, 3
ONE = F32(1.0)


# ---- helpers --------------------------------------------------------------------------------------------------------------------------
def rig_of(ctx, wide, peak):
    """The planes of one run: a pitch of 1 MiB (`peak` of them alive at most) or of 512 bytes."""
    return Rig(ctx, "tall" if wide else "ordinary", peak)


def shows_a_wrap(line, inputs, wants):
    """The reference alone: the rows from `line` on are not the rows 0 .. again, in the inputs and in what is expected, and the
    expected rows from `line` on are finite and varied."""
    for a in inputs:
        assert a.shape[0] > line and not np.array_equal(bits(a[line:]), bits(a[:a.shape[0] - line]))
    for a in wants:
        top = a[line:]
        assert top.size and np.isfinite(top).all() and np.unique(top).size > min(1000, top.size // 4)
        assert not np.array_equal(bits(top), bits(a[:a.shape[0] - line]))


def same(got, want, what):
    d = bits(got) != bits(np.ascontiguousarray(want, F32))
    if d.any():
        rows = np.flatnonzero(d.any(axis=1))
        pytest.fail("%s: %d of %d pixels differ, in %d rows from row %d to row %d, first (y, x) = %s" %
                    (what, d.sum(), d.size, rows.size, rows[0], rows[-1], np.argwhere(d)[0]))


def same_runs(runs, what):
    """{name: array} of the run on planes with a pitch of 1 MiB and of the run on ordinary planes: the same bytes."""
    assert runs[0].keys() == runs[1].keys()
    for name in runs[0]:
        same(runs[0][name], runs[1][name], "%s, %s: pitch 1 MiB against pitch 512" % (what, name))


def replicate(half, w, h):
    return np.repeat(np.repeat(half, 2, axis=0), 2, axis=1)[:h, :w]


_fields, _wanted = {}, {}


def fields(oracle, w, h, seed):
    """level_fields, made once per size and seed and read-only"""
    key = (w, h, seed)
    if key not in _fields:
        _fields[key] = level_fields(oracle, w, h, seed)
        for a in _fields[key]:
            a.setflags(write=False)
    return _fields[key]


# name: (data term, inner, hx, hy, omega, base_flow_shift, launches of the packed build per outer iteration)
SOLVES = {
    "grey 3 x 5": (GREY, 5, ONE, ONE, 0.0, 0, 1),
    "gradient 3 x 5": (GRADIENT, 5, F32(1.25), F32(1.1), 0.0, 0, 1),
    "log-derivatives 3 x 5": (LOG, 5, ONE, ONE, 0.0, 0, 0),  # (no packed build of this term: the pipeline's, on any context)
    "grey 3 x 2": (GREY, 2, ONE, ONE, 0.0, 0, 1),
    "grey sor 1.5, 3 x 2": (GREY, 2, ONE, ONE, 1.5, 0, 1),
    "gradient 3 x 5, half-size base": (GRADIENT, 5, ONE, ONE, 0.0, 1, 1),
}


def solve_inputs(oracle, name, w, h, seed=11):
    """(f0, f1, u, v as the oracle takes them, u and v as the device takes them)"""
    constancy, _, _, _, _, shift, _ = SOLVES[name]
    f0, f1, u, v, _, _ = fields(oracle, w, h, seed)
    f0, f1 = np.roll(f0, seed, axis=0), np.roll(f1, seed, axis=0)  # (level_fields' first frame is the same for every seed)
    if constancy == LOG:
        f0, f1 = np.abs(f0), np.abs(f1)
    if shift:
        u_half, v_half = (np.ascontiguousarray(a[:(h + 1) // 2, :(w + 1) // 2]) for a in (u, v))
        return f0, f1, replicate(u_half, w, h), replicate(v_half, w, h), u_half, v_half
    return f0, f1, u, v, u, v


def wanted(ctx, oracle, name, w, h, seed=11):
    """The oracle's (du, dv) of a case of SOLVES, computed once."""
    key = (name, w, h, seed)
    if key not in _wanted:
        constancy, inner, hx, hy, omega, _, _ = SOLVES[name]
        f0, f1, u, v, _, _ = solve_inputs(oracle, name, w, h, seed)
        if omega:
            _wanted[key] = oracle.solve_level_sor(f0, f1, u, v, w, h, hx, hy, ALPHA, EPS, EPS, OUTER, inner, omega, constancy)[:2]
        elif constancy == LOG:
            with oracle.device_logs(ctx):
                _wanted[key] = oracle.solve_level(f0, f1, u, v, w, h, hx, hy, ALPHA, EPS, EPS, OUTER, inner, constancy)[:2]
        else:
            _wanted[key] = oracle.solve_level(f0, f1, u, v, w, h, hx, hy, ALPHA, EPS, EPS, OUTER, inner, constancy)[:2]
    return _wanted[key]


class SolvePlanes:
    """The ten planes of flow2d_solve_level in a rig, allocated once and filled per case."""

    def __init__(self, rig, w, h):
        self.rig, self.w, self.h = rig, w, h
        self.inputs = [rig.out(w, h) for _ in range(4)]
        self.written = [rig.out(w, h) for _ in range(6)]

    def solve(self, ctx, arrays, name, algorithm):
        constancy, inner, hx, hy, omega, shift, _ = SOLVES[name]
        self.rig.poison(self.inputs + self.written, self.w, self.h)
        for p, a in zip(self.inputs, arrays):
            p.upload(a)
        rdu, rdv = ctx.solve_level(*self.inputs, *self.written, self.w, self.h, hx, hy, ALPHA, EPS, EPS, OUTER, inner, constancy, algorithm,
                                   container_height=self.h, sor_omega=omega, base_flow_shift=shift)
        ctx.synchronize()
        return {"du": rdu.download(self.w, self.h), "dv": rdv.download(self.w, self.h)}


def check_solves(ctx, oracle, names, w, h, line, algorithm, build=None, ask=None):
    """Every case of `names` on planes with a pitch of 1 MiB and on ordinary ones: the oracle's bits on both."""
    arrays = {name: solve_inputs(oracle, name, w, h) for name in names}
    for name in names:  # the reference alone, before any device result
        f0, f1, _, _, u, v = arrays[name]
        shows_a_wrap(line, (f0, f1), wanted(ctx, oracle, name, w, h))
        shows_a_wrap(line >> SOLVES[name][5], (u, v), ())
    runs = {name: [] for name in names}
    for wide in (True, False):
        rig = rig_of(ctx, wide, 10)
        try:
            planes = SolvePlanes(rig, w, h)
            if wide:
                assert planes.inputs[0].pitch == PITCH_BYTES
            if build:
                build.served(0)
            for name in names:
                if ask:
                    ask(name, planes.inputs[0].pitch)
                runs[name].append(planes.solve(ctx, arrays[name][:2] + arrays[name][4:], name, algorithm))
                if build:
                    build.served(OUTER * SOLVES[name][6])
        finally:
            rig.free()
    for name in names:
        odu, odv = wanted(ctx, oracle, name, w, h)
        for run, kind in zip(runs[name], ("pitch 1 MiB", "pitch 512")):
            same(run["du"], odu, "%s, %s: du against the oracle" % (name, kind))
            same(run["dv"], odv, "%s, %s: dv against the oracle" % (name, kind))
        same_runs(runs[name], name)


# ---- the solver -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build_name", ["pipeline", "packed"])
def test_strips_on_high_planes(flow2d, ctx, oracle, build_name):
    """flow2d_solve_level with the strips on 100 x 4095 at a pitch of 1 MiB: every plane_load and plane_store of the rows from 2048 on
    has bit 31 set in its offset, up to 2^32 - 2^20 + 400.  The half-size base flow is there for uv_row_offset.  Ten high planes."""
    build = Build(flow2d, ctx, build_name)

    def ask(name, pitch):
        constancy, inner, hx, hy, omega, shift, _ = SOLVES[name]
        p = flow2d.SolveParams(W, H, pitch, H, hx, hy, ALPHA, EPS, EPS, OUTER, inner, constancy, FUSED, omega, shift)
        takes = flow2d.hip_lib().flow2d_solve_level_takes_half_base(ctx.handle, ctypes.byref(p))
        assert takes == 1, (name, pitch)  # (whatever the case's own shift: the level is the strips' and within their offsets)

    try:
        check_solves(ctx, oracle, list(SOLVES), W, H, HALF, FUSED, build, ask)
    finally:
        ctx.set_lone(False)


def test_tiles_and_sweeps_on_high_planes(flow2d, ctx, oracle):
    """TILED and PER_SWEEP requested on the planes of the strips' test: size_t offsets by reading, which this keeps so.  Ten high
    planes."""
    for algorithm, name in ((TILED, "grey 3 x 5"), (PER_SWEEP, "gradient 3 x 5")):
        assert flow2d.hip_lib().flow2d_solver_algorithm_for(algorithm, W, H, PITCH_BYTES, OUTER, 5, SOLVES[name][0]) == algorithm
        check_solves(ctx, oracle, [name], W, H, HALF, algorithm)


def test_sweeps_beyond_the_line(flow2d, ctx, oracle):
    """100 x 4200 at a pitch of 1 MiB under AUTO: 4.1 GiB a plane, beyond the strips' offsets, so the per-sweep kernels run it (the
    comment above fused_addressable's use in csrc/solve_level.hip promises that); the ordinary planes of the second run are the
    strips'.  Row 4096 + k would alias row k.  Ten planes of 4.1 GiB."""
    pick = flow2d.hip_lib().flow2d_solver_algorithm_for
    names = ["grey 3 x 5", "gradient 3 x 5"]
    for name in names:
        assert pick(AUTO, W, TALL_H, PITCH_BYTES, OUTER, 5, SOLVES[name][0]) == PER_SWEEP
        assert pick(AUTO, W, TALL_H, 512, OUTER, 5, SOLVES[name][0]) == FUSED
    check_solves(ctx, oracle, names, W, TALL_H, LINE, AUTO)


# ---- a lock-step group ----------------------------------------------------------------------------------------------------------------
def test_group_whose_span_passes_4_gib(flow2d, ctx, oracle):
    """Three instances of 100 x 1390, 1400 rows of 1 MiB apart, in one allocation of 4200 MiB a plane: the instances start at 0,
    1400 MiB and 2800 MiB (bit 31 set), the batch span passes 4 GiB and each instance's plane does not.  The strips and the
    streaming median with addend must decide for 32-bit offsets by the instance's plane and take them against the instance's base:
    each instance equals the oracle and its frame run alone on ordinary planes, and every row outside the instances' frames stays
    poisoned.  Ten planes of 4200 MiB."""
    w, h, G, stride_rows, rows, cols = W, 1390, 3, 1400, 4200, 128
    name = "gradient 3 x 5"
    constancy, inner, hx, hy, _, _, _ = SOLVES[name]
    assert stride_rows * PITCH_BYTES == 1400 << 20 and 2 * stride_rows * PITCH_BYTES >= 1 << 31 and h * PITCH_BYTES < 1 << 32
    assert (2 * stride_rows + h) * PITCH_BYTES > 1 << 32 and rows == G * stride_rows
    assert flow2d.hip_lib().flow2d_solver_algorithm_for(FUSED, w, h, PITCH_BYTES, OUTER, inner, constancy) == FUSED
    group = [solve_inputs(oracle, name, w, h, seed=70 + b)[:4] for b in range(G)]
    want = [wanted(ctx, oracle, name, w, h, seed=70 + b) for b in range(G)]
    rng = np.random.default_rng(71)
    adds = []
    for b in range(G):
        du, dv = (rng.normal(0, 0.3, (h, w)).astype(F32) for _ in range(2))
        du[rng.random((h, w)) < 0.02] = np.nan
        dv[::3, ::5] = 0.0
        adds.append((du, dv))
    medians = [(oracle.median(oracle.add(f[2], a[0], w, h), w, h, 5), oracle.median(oracle.add(f[3], a[1], w, h), w, h, 5)) for f, a in zip(group, adds)]
    for b in range(1, G):  # what another instance's base, or a wrapped one, would give is something else
        for k in range(4):
            assert not np.array_equal(bits(group[b][k]), bits(group[0][k]))
        assert not np.array_equal(bits(want[b][0]), bits(want[0][0])) and not np.array_equal(bits(medians[b][0]), bits(medians[0][0]))
        assert np.isfinite(want[b][0]).all() and np.unique(want[b][0]).size > 1000

    def stack(arrays):
        full = np.full((rows, cols), POISON, U32)
        for b, a in enumerate(arrays):
            full[b * stride_rows:b * stride_rows + h, :w] = bits(a)
        return full.view(F32)

    def untouched(plane, what):
        """the frames of a written plane as bits, after a look at everything beside them"""
        got = bits(plane.download(cols, rows))
        outside = np.ones(got.shape, bool)
        for b in range(G):
            outside[b * stride_rows:b * stride_rows + h, :w] = False
        assert (got[outside] == POISON).all(), "%s: %d words outside the instances' frames were written" % (what, (got[outside] != POISON).sum())
        return [got[b * stride_rows:b * stride_rows + h, :w] for b in range(G)]

    rig = rig_of(ctx, True, 10)
    try:
        d = [rig.load(stack([f[k] for f in group]), rows) for k in range(4)]
        written = [rig.load(stack([]), rows) for _ in range(6)]
        assert d[0].pitch == PITCH_BYTES and d[0].pitch * rows > 1 << 32
        with ctx.set_batch(G, stride_rows * PITCH_BYTES):
            rdu, rdv = ctx.solve_level(*d, *written, w, h, hx, hy, ALPHA, EPS, EPS, OUTER, inner, constancy, FUSED, container_height=h)
        ctx.synchronize()
        got = {p: untouched(p, "solve_level") for p in written}
        solved = got[rdu], got[rdv]
        for plane, arrays in zip(d, zip(*group)):
            assert np.array_equal(bits(plane.download(cols, rows)), bits(stack(arrays))), "an input was written"
        # the median of (u + du, v + dv): the flow planes as they are, the addends in the frames' planes, two poisoned outputs
        d[0].upload(stack([a[0] for a in adds]))
        d[1].upload(stack([a[1] for a in adds]))
        for p in written[:2]:
            p.upload(stack([]))
        with ctx.set_batch(G, stride_rows * PITCH_BYTES):
            ctx.add_median(d[2], d[0], w, h, 5, written[0], d[3], d[1], written[1])
        ctx.synchronize()
        filtered = untouched(written[0], "add_median a"), untouched(written[1], "add_median b")
    finally:
        rig.free()
    for b in range(G):
        for k, n in enumerate(("du", "dv")):
            same(solved[k][b].view(F32), want[b][k], "instance %d: %s against the oracle" % (b, n))
            same(filtered[k][b].view(F32), medians[b][k], "instance %d: median of %s against the oracle" % (b, n))
    # every frame alone, on ordinary planes and without a batch
    rig = rig_of(ctx, False, 10)
    try:
        planes = SolvePlanes(rig, w, h)
        for b in range(G):
            alone = planes.solve(ctx, group[b], name, FUSED)
            same(solved[0][b].view(F32), alone["du"], "instance %d: du against the frame alone" % b)
            same(solved[1][b].view(F32), alone["dv"], "instance %d: dv against the frame alone" % b)
            rig.poison(planes.written[:2], w, h)
            src = [planes.inputs[k].upload(group[b][2 + k]) for k in range(2)]
            add = [planes.written[2 + k].upload(adds[b][k]) for k in range(2)]
            ctx.add_median(src[0], add[0], w, h, 5, planes.written[0], src[1], add[1], planes.written[1])
            ctx.synchronize()
            for k in range(2):
                same(filtered[k][b].view(F32), planes.written[k].download(w, h), "instance %d: median %d against the frame alone" % (b, k))
    finally:
        rig.free()


# ---- the per-level pyramid entries ------------------------------------------------------------------------------------------------------
def resampled(oracle, a, iw, ih, w, h):
    return np.ascontiguousarray(oracle.resample(in_container(a, w, h), iw, ih, w, h)[:h, :w])


@pytest.mark.parametrize("h,line", [(H, HALF), (TALL_H, LINE)], ids=["high", "tall"])
def test_pyramid_entries(flow2d, ctx, oracle, h, line):
    """The per-level entries of the pyramid on 100 x 4095 (byte offsets up to 2^32 - 2^20) and on 100 x 4200 (4.1 GiB), at a pitch of
    1 MiB: size_t offsets by reading, which this keeps so.  Against the oracle and against the run on ordinary planes, bit for bit.
    Thirteen planes."""
    w = W
    hx, hy = F32(1.25), F32(1.1)
    f0, f1, u, v, du, dv = fields(oracle, w, h, 13)
    u, v = (u * F32(3)).astype(F32), (v * F32(3)).astype(F32)
    sigma = 1.5
    taps, radius = flow2d.gaussian_kernel(sigma)
    assert 1 <= radius <= 6  # the streaming form
    iw, ih = w // 2, h // 2
    rng = np.random.default_rng(14)
    u_in, v_in = (rng.normal(0, 2, (ih, iw)).astype(F32) for _ in range(2))
    ow, oh = 77, h * 4 // 5
    want = {"blur": oracle.convolution(f0, w, h, sigma), "warp": oracle.registration(f0, f1, u, v, w, h, hx, hy)}
    want["up u"], want["up v"] = resampled(oracle, u_in, iw, ih, w, h), resampled(oracle, v_in, iw, ih, w, h)
    want["up warp"] = oracle.registration(f0, f1, want["up u"], want["up v"], w, h, hx, hy)
    want["u + du"], want["v + dv"] = oracle.add(u, du, w, h), oracle.add(v, dv, w, h)
    want["phi"], want["ksi"] = oracle.compute_phi_ksi(f0, f1, u, v, du, dv, w, h, hx, hy, EPS, EPS)
    shows_a_wrap(line, (f0, f1, u, v, du, dv), want.values())
    for k, a in enumerate((f0, f1)):
        want["x %d" % k] = np.ascontiguousarray(oracle.resample_x(a, ow, h, w)[:h, :ow])
        want["y %d" % k] = np.ascontiguousarray(oracle.resample_y(a, w, oh, h)[:oh, :w])
        shows_a_wrap(line, (), (want["x %d" % k],))
        shows_a_wrap(-(-line * oh // h), (), (want["y %d" % k],))  # (the output rows that read input rows from the line on)
    even = h if h % 2 == 0 else h - 1  # flow2d_upsample_registration_half_2d takes exactly doubled levels only
    if even != h:
        half_in = u_in[:even // 2], v_in[:even // 2]
        want["even up u"], want["even up v"] = (resampled(oracle, a, iw, even // 2, w, even) for a in half_in)
        want["even up warp"] = oracle.registration(f0[:even], f1[:even], want["even up u"], want["even up v"], w, even, hx, hy)
        shows_a_wrap(line, (), (want["even up u"], want["even up warp"]))

    def poisoned(plane, out_w, out_h, what):
        """the first out_w x out_h words of an output whose frame was poisoned, after a look at the rest of the frame"""
        got = bits(plane.download(w, h))
        assert (got[out_h:] == POISON).all() and (got[:, out_w:] == POISON).all(), "%s: written beyond %d x %d" % (what, out_w, out_h)
        return got[:out_h, :out_w].view(F32)

    def run(rig):
        p0, p1, pu, pv, pdu, pdv = (rig.load(a, h) for a in (f0, f1, u, v, du, dv))
        pui, pvi = rig.load(u_in, h), rig.load(v_in, h)
        outs = [rig.out(w, h) for _ in range(3)]
        sums = [rig.load(u, h), rig.load(v, h)]
        got = {}
        ctx.gaussian_blur(outs[0], p0, w, h, taps, radius)
        ctx.registration(p0, p1, pu, pv, w, h, hx, hy, outs[1])
        ctx.synchronize()
        got["blur"], got["warp"] = outs[0].download(w, h), outs[1].download(w, h)
        rig.poison(outs, w, h)
        ctx.upsample_registration(pui, pvi, iw, ih, outs[0], outs[1], p0, p1, w, h, hx, hy, outs[2])
        ctx.synchronize()
        got["up u"], got["up v"], got["up warp"] = (o.download(w, h) for o in outs)
        rig.poison(outs, w, h)
        if even == h:
            ctx.upsample_registration_half(pui, pvi, iw, ih, outs[0], outs[1], p0, p1, w, h, hx, hy, outs[2])
            ctx.synchronize()
            got["half u"], got["half v"] = poisoned(outs[0], iw, ih, "half u"), poisoned(outs[1], iw, ih, "half v")
            got["half warp"] = outs[2].download(w, h)
        else:
            with pytest.raises(flow2d.Flow2DError) as e:
                ctx.upsample_registration_half(pui, pvi, iw, ih, outs[0], outs[1], p0, p1, w, h, hx, hy, outs[2])
            assert e.value.status == UNSUPPORTED
            ctx.synchronize()
            for o in outs:
                assert (bits(o.download(w, h)) == POISON).all(), "a refused call wrote"
            ctx.upsample_registration(pui, pvi, iw, even // 2, outs[0], outs[1], p0, p1, w, even, hx, hy, outs[2])
            ctx.synchronize()
            got["even up u"], got["even up v"], got["even up warp"] = (poisoned(o, w, even, "even up") for o in outs)
            rig.poison(outs, w, h)
            ctx.upsample_registration_half(pui, pvi, iw, even // 2, outs[0], outs[1], p0, p1, w, even, hx, hy, outs[2])
            ctx.synchronize()
            got["half u"], got["half v"] = poisoned(outs[0], iw, even // 2, "half u"), poisoned(outs[1], iw, even // 2, "half v")
            got["half warp"] = poisoned(outs[2], w, even, "half warp")
        ctx.add_pair(sums[0], pdu, sums[1], pdv, w, h)
        rig.poison(outs, w, h)
        ctx.compute_phi_ksi(p0, p1, pu, pv, pdu, pdv, w, h, hx, hy, EPS, EPS, outs[0], outs[1])
        ctx.synchronize()
        got["u + du"], got["v + dv"] = sums[0].download(w, h), sums[1].download(w, h)
        got["phi"], got["ksi"] = outs[0].download(w, h), outs[1].download(w, h)
        rig.poison(outs, w, h)
        ctx.resample_x_pair(p0, outs[0], p1, outs[1], ow, h, w)
        ctx.synchronize()
        got["x 0"], got["x 1"] = poisoned(outs[0], ow, h, "x 0"), poisoned(outs[1], ow, h, "x 1")
        rig.poison(outs, w, h)
        ctx.resample_y_pair(p0, outs[0], p1, outs[1], w, oh, h)
        ctx.synchronize()
        got["y 0"], got["y 1"] = poisoned(outs[0], w, oh, "y 0"), poisoned(outs[1], w, oh, "y 1")
        for plane, a in zip((p0, p1, pu, pv, pdu, pdv), (f0, f1, u, v, du, dv)):
            assert np.array_equal(bits(plane.download(w, h)), bits(a)), "an input was written"
        return got

    runs = []
    for wide in (True, False):
        rig = rig_of(ctx, wide, 13)
        try:
            runs.append(run(rig))
        finally:
            rig.free()
    up = "even up" if even != h else "up"
    for got, kind in zip(runs, ("pitch 1 MiB", "pitch 512")):
        for name, x in want.items():
            same(got[name], x, "%s, %s against the oracle" % (name, kind))
        # the half-size form: the same warped frame, and the flow once per 2 x 2 block
        same(got["half warp"], want[up + " warp"], "half warp, %s" % kind)
        same(replicate(got["half u"], w, even), want[up + " u"], "half u, %s" % kind)
        same(replicate(got["half v"], w, even), want[up + " v"], "half v, %s" % kind)
    same_runs(runs, "pyramid entries at %d rows" % h)
