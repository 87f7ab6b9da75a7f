"""The packed build of the fused strip kernel (the six objects fused_launch_g{0,1,2}_p{0,1}_k of csrc/Makefile: packed fp32
multiplies, fmas and adds, no priority filter), which a lone context (flow2d_context_set_lone, the default of OpticalFlow and of the
command line) takes for every strip launch of at most one workgroup per CU.  It is another instruction stream than the pipeline's
build and must give the same bits: every case here runs flow2d_solve_level with the strips on a lone context, compares all 32 bits
of every pixel with the CPU oracle, and asserts from flow2d_fused_packed_launches that the packed build -- not the pipeline's, which
would pass the comparison just as well -- served exactly the launches it must have.  A case whose plan outgrows the packed build
fails; it is not skipped.

Which of the packed build's 42 kernels (object x Jacobi sweeps 1..5, object x red-black stages 2 and 4) a test reaches:
  test_every_jacobi_kernel_of_the_packed_build      all 30 Jacobi kernels, each on a level of one block column (every wave a border
                                                    wave) and on one with strips that touch no border
  test_every_sor_kernel_of_the_packed_build         all 12 red-black kernels, omega 1.0 and 1.9
  the guard and plan tests of test_gpu_fused.py     collected here a second time with the packed build (`build` below): g0 / g1,
                                                    sweeps 3 and 5, with the operands that trip every guard and the plain pass
  test_half_size_base_flow_on_the_packed_build      g0 / g1 / g2, both spacings, sweeps 1, 2, 4, 5 with base_flow_shift = 1
  test_lock_step_group_shares_one_packed_launch     g0_p0 / g1_p0, sweeps 5, three instances in grid.z
What the packed build does not hold -- and the counter must show as not served -- is in test_what_the_packed_build_leaves_*."""
import numpy as np
import pytest

import test_gpu_fused as pipeline_tests
from conftest import in_container, level_fields
from test_gpu_fused import (  # noqa: F401  (collected here as well: the same functions, the `build` fixture of this file)
    Build, bits, test_a_diffusion_front_trips_the_guard_only_where_it_is,
    test_a_spacing_outside_the_guarded_range_takes_the_plain_divisions, test_denominators_outside_the_proven_range_fall_back,
    test_negative_zero_in_the_flow_falls_back, test_ordinary_operands_do_not_fall_back,
    test_overflowing_results_match_the_per_sweep_kernels, test_robustifier_arguments_outside_the_proven_range_fall_back,
    test_spacings_that_are_no_powers_of_two, test_tiny_differences_over_a_non_power_of_two_spacing_fall_back,
    test_tiny_numerators_fall_back_to_the_plain_division, test_zero_regularisers_match_the_per_sweep_kernels)

pytestmark = pytest.mark.gpu

F32 = np.float32
POISON = 0x7F7F7F7F
FUSED = 2
GREY, GRADIENT, GRADIENT_UNTILED, LOG_DERIVATIVES = 0, 1, 2, 3
# a power-of-two spacing (the *_p1_k objects) and the spacing of a level 1.25 x 1.1 times smaller than its container (*_p0_k: the
# divisions by 2h and 4h go through the three-step division)
SPACINGS = {"pow2": (F32(1.0), F32(1.0)), "other": (F32(1.25), F32(1.1))}


@pytest.fixture(params=["packed"])
def build(request, flow2d, ctx):
    """The context of the test marked lone, and the counter of packed launches as it stands (`ctx` is a fresh context per test:
    the mark does not leak).  The tests imported from test_gpu_fused.py get this one in place of that file's."""
    return Build(flow2d, ctx, request.param)


_fields = {}


def fields(oracle, w, h, seed):
    """level_fields, made once per size and seed (read-only: a test that changes a plane copies it)"""
    key = (w, h, seed)
    if key not in _fields:
        _fields[key] = level_fields(oracle, w, h, seed)[:4]
        for a in _fields[key]:
            a.setflags(write=False)
    return _fields[key]


def live_blocks(order):
    return order[order[:, 0] >= 0]


def assert_fits_the_packed_build(ctx, w, h, stages, instances=1):
    """at most one workgroup per CU (256 of them): what launch_fused_outer asks of a launch of the packed build"""
    blocks = len(live_blocks(ctx.fused_block_order(w, h, stages, instances))) * instances
    assert blocks <= 256, "%d x %d, %d stages, %d instance(s): %d blocks" % (w, h, stages, instances, blocks)


def first_launch_stages(inner, sor=False):
    """Stages of the launch that starts an outer iteration -- the one launch of it the packed build can serve: the library cuts
    more than five sweeps (two red-black iterations: four half-sweep stages) into equal launches, the longer ones first."""
    per_launch = 2 if sor else 5
    launches = max(1, -(-inner // per_launch))
    first = inner // launches + (1 if inner % launches else 0)
    return 2 * first if sor else first


def strips(ctx, planes, w, h, cw, ch, hx, hy, alpha, outer, inner, constancy, omega=0.0, shift=0):
    """flow2d_solve_level with the strips on planes[0..3] (device) into poisoned planes; the increment as 32-bit words"""
    scratch = [ctx.plane(cw, ch).fill_bytes(0x7F) for _ in range(6)]
    rdu, rdv = ctx.solve_level(*planes, *scratch, w, h, hx, hy, alpha, 0.001, 0.001, outer, inner, constancy, FUSED,
                               sor_omega=omega, base_flow_shift=shift)
    got = bits(rdu.download(w, h)), bits(rdv.download(w, h))
    for p in scratch:
        p.free()
    return got


def upload(ctx, arrays, cw, ch):
    return [ctx.plane(cw, ch, in_container(a, cw, ch)) for a in arrays]


# ---- every instantiation ------------------------------------------------------------------------------------------------------

# 100 x 70 in a 128 x 80 container: one block column, every wave runs the border body, ragged last strip columns.
# 640 x 520 (in a 800 x 572 container for the second spacing): three or four block columns, a border-aware or uniform plan of
# 178 ... 240 blocks with strips that touch no border, for every sweep count 1 ... 5 (checked below from the plan itself).
@pytest.mark.parametrize("inner", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("spacing", ["pow2", "other"])
@pytest.mark.parametrize("constancy", [GREY, GRADIENT, GRADIENT_UNTILED])
@pytest.mark.parametrize("w,h", [(100, 70), (640, 520)])
def test_every_jacobi_kernel_of_the_packed_build(ctx, oracle, build, w, h, constancy, spacing, inner):
    """Two outer iterations, so that the second one reads an increment that is not zero."""
    hx, hy = SPACINGS[spacing]
    cw, ch = (128, 80) if (w, h) == (100, 70) else ((640, 520) if spacing == "pow2" else (800, 572))
    outer = 2
    order = live_blocks(ctx.fused_block_order(w, h, inner, 1))
    assert len(order) <= 256, len(order)
    columns = int(order[:, 0].max()) + 1
    if (w, h) == (100, 70):
        assert columns == 1
    else:  # a strip whose rows, with their halo, keep off the first and the last row, in a block column that is neither first nor last
        assert columns >= 3
        assert any(0 < bx < columns - 1 and y0 > inner + 2 and y1 + inner + 5 < h for bx, _, y0, y1 in order.tolist()), order
    f0, f1, u, v = fields(oracle, w, h, 7)
    du, dv = strips(ctx, upload(ctx, (f0, f1, u, v), cw, ch), w, h, cw, ch, hx, hy, 3.5, outer, inner, constancy)
    odu, odv, _, _ = oracle.solve_level(f0, f1, u, v, w, h, hx, hy, 3.5, 0.001, 0.001, outer, inner, constancy)
    assert np.array_equal(du, bits(odu)) and np.array_equal(dv, bits(odv))
    build.served(outer)


def sor_case(ctx, oracle, build, w, h, constancy, spacing, iterations, omega):
    if constancy == GRADIENT:
        w, h = (w + 15) // 16 * 16, (h + 7) // 8 * 8  # the reference's tile rule is defined on multiples of 16 x 8
    hx, hy = SPACINGS[spacing]
    outer = 2
    assert_fits_the_packed_build(ctx, w, h, first_launch_stages(iterations, sor=True))
    f0, f1, u, v = fields(oracle, w, h, 77)
    du, dv = strips(ctx, upload(ctx, (f0, f1, u, v), w, h), w, h, w, h, hx, hy, 35.0, outer, iterations, constancy, omega=omega)
    odu, odv = oracle.solve_level_sor(f0, f1, u, v, w, h, hx, hy, 35.0, 0.001, 0.001, outer, iterations, omega, constancy)
    assert np.array_equal(du, bits(odu)) and np.array_equal(dv, bits(odv))
    build.served(outer)


@pytest.mark.parametrize("omega", [1.0, 1.9])
@pytest.mark.parametrize("iterations", [1, 2])  # one launch of two and of four half-sweep stages
@pytest.mark.parametrize("spacing", ["pow2", "other"])
@pytest.mark.parametrize("constancy", [GREY, GRADIENT, GRADIENT_UNTILED])
@pytest.mark.parametrize("w,h", [(200, 136), (330, 250)])
def test_every_sor_kernel_of_the_packed_build(ctx, oracle, build, w, h, constancy, spacing, iterations, omega):
    """Red-black SOR as the stages of the strip kernel, on the levels of test_sor_in_the_strip_kernel."""
    sor_case(ctx, oracle, build, w, h, constancy, spacing, iterations, omega)


@pytest.mark.parametrize("spacing", ["pow2", "other"])
@pytest.mark.parametrize("constancy", [GREY, GRADIENT, GRADIENT_UNTILED])
def test_sor_of_five_iterations_starts_on_the_packed_build(ctx, oracle, build, constancy, spacing):
    """Five iterations are launches of 2 + 2 + 1: the first is the packed build's, the two that continue it are the pipeline's (the
    packed build holds no kernels for continued sweeps) -- one packed launch per outer iteration, and the oracle's bits."""
    sor_case(ctx, oracle, build, 200, 136, constancy, spacing, 5, 1.9)


# ---- the base flow at half the level's size ----------------------------------------------------------------------------------------

def replicate(half, w, h):
    return np.repeat(np.repeat(half, 2, axis=0), 2, axis=1)[:h, :w]


def half_base_case(ctx, oracle, build, f0, f1, u_half, v_half, w, h, spacing, outer, inner, constancy):
    """The expectation of test_shifted_base_gives_the_bits_of_the_replicated_base -- the strips fed the replicated base at full
    size, here on the pipeline's build -- and the oracle's level for those planes, against the packed build reading the half-size
    base with base_flow_shift = 1."""
    u, v = replicate(u_half, w, h), replicate(v_half, w, h)
    frames = [ctx.plane(w, h, a) for a in (f0, f1)]
    ctx.set_lone(False)
    full = [ctx.plane(w, h).fill_bytes(0x7F).upload(a) for a in (u, v)]
    want = strips(ctx, frames + full, w, h, w, h, spacing, spacing, 35.0, outer, inner, constancy)
    build.served(0)
    ctx.set_lone(True)
    assert_fits_the_packed_build(ctx, w, h, first_launch_stages(inner))
    half = [ctx.plane(w, h).fill_bytes(0x7F).upload(a) for a in (u_half, v_half)]
    got = strips(ctx, frames + half, w, h, w, h, spacing, spacing, 35.0, outer, inner, constancy, shift=1)
    build.served(outer)
    for p in frames + full + half:
        p.free()
    assert not (want[0] == POISON).any()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (spacing, inner)
    odu, odv, _, _ = oracle.solve_level(f0, f1, u, v, w, h, spacing, spacing, 35.0, 0.001, 0.001, outer, inner, constancy)
    assert np.array_equal(got[0], bits(odu)) and np.array_equal(got[1], bits(odv)), (spacing, inner)


@pytest.mark.parametrize("constancy", [GREY, GRADIENT, GRADIENT_UNTILED])  # (the LogDerivatives term has no packed build)
@pytest.mark.parametrize("w,h", [(128, 96), (320, 208)])
def test_half_size_base_flow_on_the_packed_build(ctx, oracle, build, w, h, constancy):
    """The cases of test_shifted_base_gives_the_bits_of_the_replicated_base: sweeps 1, 2, 5 and 7 (a launch of four sweeps, which
    the packed build serves, and one of three that continues it, which it does not), outer 3, both kinds of spacing."""
    f0, f1, u, v = fields(oracle, w, h, 61)
    u_half, v_half = u[:h // 2, :w // 2].copy(), v[:h // 2, :w // 2].copy()
    before = ctx.fused_fallbacks()
    for spacing in (1.0, 1.37):
        for inner in (1, 2, 5, 7):
            half_base_case(ctx, oracle, build, f0, f1, u_half, v_half, w, h, F32(spacing), 3, inner, constancy)
    assert ctx.fused_fallbacks() == before  # (ordinary operands: every wave took the guarded short forms)


def test_half_size_base_flow_with_a_negative_zero_on_the_packed_build(ctx, oracle, build):
    """test_shifted_base_with_a_negative_zero_takes_the_fallback_pass: flat frames and a base flow of -0, every numerator a -0 --
    the guard sees them through the shifted loads of the packed build too, and the plain pass gives the oracle's signed zeros."""
    w, h = 320, 208
    f0 = np.full((h, w), 80.0, F32)
    u_half, v_half = np.full((h // 2, w // 2), -0.0, F32), np.zeros((h // 2, w // 2), F32)
    before = ctx.fused_fallbacks()
    half_base_case(ctx, oracle, build, f0, f0.copy(), u_half, v_half, w, h, F32(1.0), 3, 5, GREY)
    assert ctx.fused_fallbacks() >= before + 2  # both runs tripped


# ---- a lock-step group -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("constancy", [GREY, GRADIENT])
def test_lock_step_group_shares_one_packed_launch(ctx, oracle, build, constancy):
    """Three pairs one below the other, four padding rows between them, in one launch per outer iteration (grid.z = 3): 50 blocks
    per instance, 150 in all.  Every instance has the oracle's level of its own planes; the counter counts launches, not instances."""
    w, h, G, pad, outer, inner = 300, 200, 3, 4, 2, 5
    assert_fits_the_packed_build(ctx, w, h, inner, G)
    hx, hy = SPACINGS["other"]
    stride_rows = h + pad
    group = [fields(oracle, w, h, 70 + b) for b in range(G)]

    def stack(arrays):
        full = np.full((stride_rows * G, w), POISON, np.uint32)
        for b, a in enumerate(arrays):
            full[b * stride_rows:b * stride_rows + h] = bits(a)
        return ctx.plane(w, stride_rows * G).upload(full.view(F32))

    d = [stack([f[k] for f in group]) for k in range(4)]
    scratch = [stack([]) for _ in range(6)]
    with ctx.set_batch(G, stride_rows * d[0].pitch):
        rdu, rdv = ctx.solve_level(*d, *scratch, w, h, hx, hy, 35.0, 0.001, 0.001, outer, inner, constancy, FUSED, container_height=h)
    ctx.synchronize()
    build.served(outer)
    du, dv = bits(rdu.download()), bits(rdv.download())
    for b, (f0, f1, u, v) in enumerate(group):
        odu, odv, _, _ = oracle.solve_level(f0, f1, u, v, w, h, hx, hy, 35.0, 0.001, 0.001, outer, inner, constancy)
        rows = slice(b * stride_rows, b * stride_rows + h)
        assert np.array_equal(du[rows], bits(odu)) and np.array_equal(dv[rows], bits(odv)), b
        assert (du[b * stride_rows + h:(b + 1) * stride_rows] == POISON).all(), b  # the padding rows are nobody's


# ---- the plans of test_gpu_fused.py that fit ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("constancy", [0, 1])
@pytest.mark.parametrize("w,h,cw,ch", pipeline_tests.BORDER_AWARE_LEVELS_OF_THE_PACKED_BUILD)
def test_border_aware_strip_plan_covers_every_pixel(ctx, oracle, build, w, h, cw, ch, constancy):
    """test_gpu_fused.py's test of that name on the levels whose plans hold at most one workgroup per CU"""
    pipeline_tests.test_border_aware_strip_plan_covers_every_pixel(ctx, oracle, build, w, h, cw, ch, constancy)


# ---- what the packed build leaves to the pipeline's ---------------------------------------------------------------------------------

def test_what_the_packed_build_leaves_the_log_derivatives_term(ctx, oracle, build):
    """No packed objects for solve_2d_log: a lone context runs the pipeline's.  (The oracle's logarithm is the C library's, the
    kernel's is not: this term is held to the reference's kernel elsewhere; here the lone context must repeat the other's bits.)"""
    w, h = 640, 520
    assert_fits_the_packed_build(ctx, w, h, 5)
    f0, f1, u, v = fields(oracle, w, h, 7)
    planes = upload(ctx, (np.abs(f0), np.abs(f1), u, v), w, h)
    lone = strips(ctx, planes, w, h, w, h, F32(1.0), F32(1.0), 35.0, 2, 5, LOG_DERIVATIVES)
    build.served(0)
    ctx.set_lone(False)
    other = strips(ctx, planes, w, h, w, h, F32(1.0), F32(1.0), 35.0, 2, 5, LOG_DERIVATIVES)
    build.served(0)
    assert not (lone[0] == POISON).any()
    assert np.array_equal(lone[0], other[0]) and np.array_equal(lone[1], other[1])


@pytest.mark.parametrize("constancy", [GREY, GRADIENT_UNTILED])
def test_what_the_packed_build_leaves_continued_sweeps(ctx, oracle, build, constancy):
    """Eight sweeps are two launches of four: the packed build serves the first of every outer iteration only."""
    w, h, outer = 640, 520, 2
    assert_fits_the_packed_build(ctx, w, h, first_launch_stages(8))
    f0, f1, u, v = fields(oracle, w, h, 7)
    du, dv = strips(ctx, upload(ctx, (f0, f1, u, v), w, h), w, h, w, h, F32(1.0), F32(1.0), 35.0, outer, 8, constancy)
    odu, odv, _, _ = oracle.solve_level(f0, f1, u, v, w, h, F32(1.0), F32(1.0), 35.0, 0.001, 0.001, outer, 8, constancy)
    assert np.array_equal(du, bits(odu)) and np.array_equal(dv, bits(odv))
    build.served(outer)


def test_what_the_packed_build_leaves_a_launch_that_fills_the_chip(ctx, oracle, build):
    """2048 x 2048 is planned as more blocks than CUs: two waves per SIMD, the pipeline build's case, lone context or not."""
    w, h = 2048, 2048
    assert len(live_blocks(ctx.fused_block_order(w, h, 5, 1))) > 256
    f0, f1, u, v = fields(oracle, w, h, 7)
    du, dv = strips(ctx, upload(ctx, (f0, f1, u, v), w, h), w, h, w, h, F32(1.0), F32(1.0), 35.0, 1, 5, GREY)
    odu, odv, _, _ = oracle.solve_level(f0, f1, u, v, w, h, F32(1.0), F32(1.0), 35.0, 0.001, 0.001, 1, 5, GREY)
    assert np.array_equal(du, bits(odu)) and np.array_equal(dv, bits(odv))
    build.served(0)


def test_what_the_packed_build_leaves_a_context_that_is_not_lone(ctx, oracle, build):
    w, h = 640, 520
    assert_fits_the_packed_build(ctx, w, h, 5)
    ctx.set_lone(False)
    f0, f1, u, v = fields(oracle, w, h, 7)
    du, dv = strips(ctx, upload(ctx, (f0, f1, u, v), w, h), w, h, w, h, F32(1.0), F32(1.0), 35.0, 2, 5, GREY)
    odu, odv, _, _ = oracle.solve_level(f0, f1, u, v, w, h, F32(1.0), F32(1.0), 35.0, 0.001, 0.001, 2, 5, GREY)
    assert np.array_equal(du, bits(odu)) and np.array_equal(dv, bits(odv))
    build.served(0)
