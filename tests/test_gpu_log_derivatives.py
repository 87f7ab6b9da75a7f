"""DataConstancy::LogDerivatives (solve_2d_log, constancy 3) against the CPU oracle, word for word.

The kernels take logf from the device library, the oracle from the CPU's libm; the two differ in the last place.  Here the
oracle is handed the DEVICE's logarithms (oracle.device_logs: flow2d_log_frame_2d, the function every kernel of the term calls,
behind oracle_set_log_source), so all that is left of a comparison is what a kernel can get wrong: the neighbour rule of the
reference's 16 x 8 blocks (also where the image ends inside a block), the guards of the strip kernel, the continuation
launches, the pyramid around them.  Everything is compared as uint32 words; where the inputs make NaNs, the NaN positions
must coincide and every other word be equal.

  entry            test_log_frame_*               the entry itself: specials exact, 3 ulp, refusals, the recorded fixture
  pin              test_checker_is_pinned_*       product == reference kernel == oracle under device_logs, on the 16 x 8 grid
  per-sweep tiles  test_sweep_off_the_block_grid
  level loop       test_solve_level*, test_single_workgroup
  strip guards     test_strip_guard_*
  special pixels   test_special_pixels
  pipelines        test_compute_flow
(The streaming form: tests/test_gpu_kernels.py::test_sweep_streaming_strips; batches and groups: test_gpu_batch_kernels.py,
test_gpu_flow.py.)
"""
import os

import numpy as np
import pytest

from conftest import in_container, level_fields
from test_gpu_kernels import SIZES

pytestmark = pytest.mark.gpu
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOG = 3
ALPHA = 0.001  # log derivatives are about 1 / I of the grey ones: an alpha of that scale keeps the data term in play
POISON = 0x7F7F7F7F


@pytest.fixture(scope="module")
def RK():
    from oracle import ref_kernels
    if not ref_kernels.available():
        # as in test_gpu_reference.py: a skip would let the pin of the checker disappear without anybody noticing
        pytest.fail("oracle/_ref holds no reference kernels: build them with `make -C oracle ref` where the reference's sources "
                    "are (python -c 'import __graft_entry__ as g; g.build()') and ship oracle/_ref with the snapshot")
    return ref_kernels


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def differing(got, want):
    """Number of words that differ; where `want` is NaN any NaN serves (payloads are not part of the contract)."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape
    nan = np.isnan(want)
    return int((np.isnan(got) != nan).sum() + (words(got)[~nan] != words(want)[~nan]).sum())


def up(ctx, a, cw, ch, fill=0.0):
    return ctx.plane(cw, ch, in_container(a, cw, ch, fill))


def poison_outside(plane, w, h, rows=True):
    full = words(plane.download())
    return np.all(full[:, w:] == POISON) and (not rows or np.all(full[h:, :] == POISON))


# ---- a. the entry ----------------------------------------------------------------------------------------------------------------
def entry_inputs():
    """100 x 70: uniform [0, 255]; rows of denormals, of values near 0, near -1, from 2^24 to 3e38; the specials."""
    w, h = 100, 70
    rng = np.random.default_rng(3)
    a = rng.uniform(0, 255, (h, w)).astype(np.float32)
    den = rng.integers(1, 0x007FFFFF, (5, w)).astype(np.uint32) | (rng.integers(0, 2, (5, w)).astype(np.uint32) << 31)
    a[0:5] = den.view(np.float32)
    a[5:8] = rng.uniform(-1e-3, 1e-3, (3, w)).astype(np.float32)
    a[8:10] = (rng.uniform(-1, 1, (2, w)) * np.exp2(rng.uniform(-60, -20, (2, w)))).astype(np.float32)
    a[10:13] = (-1.0 + rng.uniform(0, 1e-3, (3, w))).astype(np.float32)
    a[13] = np.float32(-1.0) + np.arange(1, w + 1, dtype=np.float32) * np.float32(2.0 ** -24)  # the floats just above -1
    a[14] = np.nextafter(np.float32(-1.0), np.float32(-2.0))  # just below -1: a negative sum
    a[15:20] = np.exp2(rng.uniform(24, 127.9, (5, w))).astype(np.float32)
    a[19, -1] = np.float32(3e38)
    a[20, :12] = [-1.0, -1.5, -3.0, -1e30, -np.inf, 0.0, -0.0, np.inf, np.nan, -2.0, 1e-45, -1e-45]
    return a


def test_log_frame_values(ctx, flow2d):
    """flow2d_log_frame_2d on a 100 x 70 plane in a 128 x 80 container.  Specials are exact: I = -1 -> -inf, I < -1 -> NaN,
    +-0 and everything that vanishes beside 1 -> +0, +inf -> +inf, NaN -> NaN.  Every other value lies within 3 ulp (the OpenCL
    full-profile bound the device library's logf is written to) of log in float64 of the float32 sum I + 1.0f.
    Measured on the MI355X: largest error 1.83 ulp."""
    w, h, cw, ch = 100, 70, 128, 80
    a = entry_inputs()
    src, dst = up(ctx, a, cw, ch, 5.0), ctx.plane(cw, ch).fill_bytes(0x7f)
    ctx.log_frame(src, dst, w, h)
    got = dst.download(w, h)
    assert poison_outside(dst, w, h)
    assert np.array_equal(words(src.download(w, h)), words(a))  # the input is left alone
    s = (a + np.float32(1.0)).astype(np.float32)
    with np.errstate(all="ignore"):
        nan, ninf, pinf, one = np.isnan(s) | (s < 0), s == 0, s == np.inf, s == 1
        assert nan.sum() >= 6 + w and ninf.sum() >= 1 and pinf.sum() >= 1 and one.sum() >= 5 * w
        assert np.array_equal(np.isnan(got), nan)
        assert np.all(words(got)[ninf] == 0xFF800000) and np.all(words(got)[pinf] == 0x7F800000) and np.all(words(got)[one] == 0)
        rest = ~(nan | ninf | pinf | one)
        ref = np.log(s[rest].astype(np.float64))
        ulp = np.spacing(np.abs(ref.astype(np.float32))).astype(np.float64)
        err = np.abs(got[rest].astype(np.float64) - ref) / ulp
    print("flow2d_log_frame_2d: largest error %.3f ulp over %d values" % (float(err.max()), int(rest.sum())))
    assert rest.sum() > 6000 and float(err.max()) <= 3.0


def test_log_frame_refusals(ctx, flow2d):
    """Null pointers, overlapping planes, pitches that are no multiple of 16 bytes or shorter than a row: INVALID_ARGUMENT, and
    a refused call writes nothing."""
    w, h, cw, ch = 100, 70, 128, 80
    src, dst = up(ctx, entry_inputs(), cw, ch, 5.0), ctx.plane(cw, ch).fill_bytes(0x7f)
    before = words(src.download()).copy()
    call = flow2d.hip_lib().flow2d_log_frame_2d
    bad = [(None, dst.ptr, w, h, src.pitch), (src.ptr, None, w, h, src.pitch), (src.ptr, src.ptr, w, h, src.pitch),
           (src.ptr, src.ptr + 10 * src.pitch, w, h, src.pitch),      # the output starts inside the input
           (src.ptr + 10 * src.pitch, src.ptr, w, h - 10, src.pitch),  # the input starts inside the output
           (src.ptr, dst.ptr, w, h, src.pitch + 4), (src.ptr, dst.ptr, w, h, 4 * w - 16), (src.ptr, dst.ptr, 0, h, src.pitch),
           (src.ptr, dst.ptr, w, 0, src.pitch), (src.ptr, dst.ptr + 4, w, h, src.pitch)]
    for args in bad:
        assert call(ctx.handle, *args) == 1, args
    assert call(None, src.ptr, dst.ptr, w, h, src.pitch) == 1
    ctx.synchronize()
    assert np.all(words(dst.download()) == POISON) and np.array_equal(words(src.download()), before)
    with pytest.raises(flow2d.Flow2DError) as e:
        ctx.log_frame(src, src, w, h)
    assert e.value.status == 1


def test_log_frame_fixture_is_what_the_device_returns(ctx):
    """tests/golden/device_log_golden.npz (tests/golden/make_device_log_golden.py) holds flow2d_log_frame_2d of the two 96 x 64
    frames of ref_kernels_golden.npz; tests/test_oracle.py feeds them to the oracle on the CPU.  If this fails, the device
    library's logf has changed: record the fixture again and see whether the reference's recorded outputs still follow."""
    g = np.load(os.path.join(GOLDEN_DIR, "ref_kernels_golden.npz"))
    d = np.load(os.path.join(GOLDEN_DIR, "device_log_golden.npz"))
    for name in ("f0", "f1"):
        frame = g["tile_in_" + name]
        h, w = frame.shape
        dst = ctx.plane(w, h)
        ctx.log_frame(ctx.plane(w, h, frame), dst, w, h)
        assert differing(dst.download(), d["log_" + name]) == 0, name


# ---- b. the pin of the new checker -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,cw,ch", [(96, 64, 96, 64), (160, 72, 192, 80)])
def test_checker_is_pinned_to_the_reference_kernel(ctx, flow2d, oracle, RK, w, h, cw, ch):
    """On the reference's 16 x 8 grid three parties must agree: the product's solve_2d_log, the reference's own kernel and the
    oracle fed by flow2d_log_frame_2d -- one sweep and a 3 x 5 level.  (If this fails while test_gpu_reference.py passes, the
    entry's logarithm is not the kernels'.)"""
    f0, f1, u, v, du, dv = level_fields(oracle, w, h, 52)
    hx, hy = np.float32(1.25), np.float32(1.1)
    d = [up(ctx, a, cw, ch, 3.0) for a in (f0, f1, u, v, du, dv)]
    phi, ksi, tdu, tdv = (ctx.plane(cw, ch).fill_bytes(0x7f) for _ in range(4))
    ctx.compute_phi_ksi(*d, w, h, hx, hy, 0.001, 0.001, phi, ksi)
    ctx.solve_sweep(*d, phi, ksi, w, h, hx, hy, 35.0, tdu, tdv, LOG)
    with RK.RefKernels(cw, ch) as R:
        rphi, rksi = R.phi_ksi(f0, f1, u, v, du, dv, hx, hy, 0.001, 0.001)
        rdu, rdv = R.sweep(RK.LOG_DERIVATIVES, f0, f1, u, v, du, dv, rphi, rksi, hx, hy, 35.0)
        wdu, wdv, _, _, _ = R.solve(f0, f1, u, v, hx, hy, RK.LOG_DERIVATIVES, 3, 5, ALPHA, 0.001, 0.001)
    with oracle.device_logs(ctx):
        odu, odv = oracle.solve_sweep(f0, f1, u, v, du, dv, rphi, rksi, w, h, hx, hy, 35.0, LOG)
        ldu, ldv, _, _ = oracle.solve_level(f0, f1, u, v, w, h, hx, hy, ALPHA, 0.001, 0.001, 3, 5, LOG)
    counts = [differing(tdu.download(w, h), rdu), differing(tdv.download(w, h), rdv), differing(odu, rdu), differing(odv, rdv),
              differing(ldu, wdu), differing(ldv, wdv)]
    assert float(np.abs(wdu).max()) > 1e-3
    for algorithm in (1, 2, 0):
        pdu, pdv, p1, p2, p3, p4 = (ctx.plane(cw, ch).fill_bytes(0x7f) for _ in range(6))
        res = ctx.solve_level(*d[:4], pdu, pdv, p1, p2, p3, p4, w, h, hx, hy, ALPHA, 0.001, 0.001, 3, 5, LOG, algorithm)
        counts += [differing(res[0].download(w, h), wdu), differing(res[1].download(w, h), wdv)]
    print("words that differ (product / oracle against the reference kernel):", counts)
    assert counts == [0] * len(counts)


# ---- c. the per-sweep tile form off the grid ---------------------------------------------------------------------------------------
OFF_GRID = SIZES + [(17, 9, 40, 30), (15, 7, 40, 30), (16, 8, 40, 30), (33, 17, 40, 30), (1, 1, 40, 30), (2, 3, 40, 30)]


@pytest.mark.parametrize("hx,hy", [(1.0, 1.0), (1.25, 1.1)])
@pytest.mark.parametrize("w,h,cw,ch", OFF_GRID)
def test_sweep_off_the_block_grid(ctx, flow2d, oracle, w, h, cw, ch, hx, hy):
    """sweep_log_kernel where the image ends inside a 16 x 8 block, one pixel past a block edge and one short of it: two sweeps
    in a row (the second reads what the first wrote) equal the oracle's, nothing outside the level is written.  A level of one
    pixel has no neighbour to take (the reference's index leaves the plane there): the entry refuses it and writes nothing."""
    f0, f1, u, v, du, dv = level_fields(oracle, w, h, 5)
    d = [up(ctx, a, cw, ch, 3.0) for a in (f0, f1, u, v, du, dv)]
    phi, ksi, tdu, tdv = (ctx.plane(cw, ch).fill_bytes(0x7f) for _ in range(4))
    if w < 2 or h < 2:
        ophi, oksi = oracle.compute_phi_ksi(f0, f1, u, v, du, dv, w, h, hx, hy, 0.001, 0.001)
        phi.upload(ophi), ksi.upload(oksi)
        with pytest.raises(flow2d.Flow2DError) as e:
            ctx.solve_sweep(*d, phi, ksi, w, h, hx, hy, ALPHA, tdu, tdv, LOG)
        assert e.value.status == 1
        ctx.synchronize()
        assert np.all(words(tdu.download()) == POISON) and np.all(words(tdv.download()) == POISON)
        return
    ctx.compute_phi_ksi(*d, w, h, hx, hy, 0.001, 0.001, phi, ksi)
    ophi, oksi = oracle.compute_phi_ksi(f0, f1, u, v, du, dv, w, h, hx, hy, 0.001, 0.001)
    assert differing(phi.download(w, h), ophi) == 0 and differing(ksi.download(w, h), oksi) == 0
    for alpha in (ALPHA, 35.0):
        d[4].upload(in_container(du, cw, ch, 3.0)), d[5].upload(in_container(dv, cw, ch, 3.0))
        tdu.fill_bytes(0x7f), tdv.fill_bytes(0x7f)
        ctx.solve_sweep(*d, phi, ksi, w, h, hx, hy, alpha, tdu, tdv, LOG)
        with oracle.device_logs(ctx):
            odu, odv = oracle.solve_sweep(f0, f1, u, v, du, dv, ophi, oksi, w, h, hx, hy, alpha, LOG)
            odu2, odv2 = oracle.solve_sweep(f0, f1, u, v, odu, odv, ophi, oksi, w, h, hx, hy, alpha, LOG)
        assert differing(tdu.download(w, h), odu) == 0 and differing(tdv.download(w, h), odv) == 0, alpha
        assert poison_outside(tdu, w, h) and poison_outside(tdv, w, h)
        ctx.solve_sweep(d[0], d[1], d[2], d[3], tdu, tdv, phi, ksi, w, h, hx, hy, alpha, d[4], d[5], LOG)
        assert differing(d[4].download(w, h), odu2) == 0 and differing(d[5].download(w, h), odv2) == 0, (alpha, "second sweep")
        full = d[4].download()
        assert np.all(full[h:, :] == 3.0) and np.all(full[:, w:] == 3.0)


# ---- e. the level loop -------------------------------------------------------------------------------------------------------------
_levels = {}


def oracle_level(ctx, oracle, w, h, cw, ch, seed, outer, inner):
    """The oracle's level under device_logs, computed once per case and shared by the algorithms."""
    key = (w, h, cw, ch, seed, outer, inner)
    if key not in _levels:
        f0, f1, u, v, _, _ = level_fields(oracle, w, h, seed)
        with oracle.device_logs(ctx):
            _levels[key] = oracle.solve_level(f0, f1, u, v, w, h, np.float32(cw / w), np.float32(ch / h), ALPHA, 0.001, 0.001, outer,
                                              inner, LOG)[:2]
    return _levels[key]


def product_level(ctx, oracle, w, h, cw, ch, seed, outer, inner, algorithm):
    f0, f1, u, v, _, _ = level_fields(oracle, w, h, seed)
    d = [up(ctx, a, cw, ch) for a in (f0, f1, u, v)]
    planes = [ctx.plane(cw, ch).fill_bytes(0x7f) for _ in range(6)]
    rdu, rdv = ctx.solve_level(*d, *planes, w, h, np.float32(cw / w), np.float32(ch / h), ALPHA, 0.001, 0.001, outer, inner, LOG,
                               algorithm)
    return rdu, rdv, planes


def check_level(ctx, oracle, w, h, cw, ch, seed, outer, inner, algorithm):
    rdu, rdv, planes = product_level(ctx, oracle, w, h, cw, ch, seed, outer, inner, algorithm)
    odu, odv = oracle_level(ctx, oracle, w, h, cw, ch, seed, outer, inner)
    if outer * inner > 0:
        assert float(np.abs(odu).max()) > 1e-4  # the data term acts: not a field smoothed to nothing
    assert differing(rdu.download(w, h), odu) == 0 and differing(rdv.download(w, h), odv) == 0
    for p in planes:  # (du / dv are zeroed over the level's width down the container, like the reference's; the columns beside stay)
        assert poison_outside(p, w, h, rows=False)
    return rdu, planes


@pytest.mark.parametrize("algorithm", [1, 2, 0])
@pytest.mark.parametrize("outer,inner", [(2, 3), (3, 2), (1, 5), (2, 1), (1, 4)])
@pytest.mark.parametrize("w,h,cw,ch", [(100, 70, 128, 80), (53, 65, 64, 80), (300, 150, 320, 160), (640, 520, 640, 520),
                                        (401, 333, 416, 340)])
def test_solve_level(ctx, oracle, w, h, cw, ch, outer, inner, algorithm):
    """The level loop in Log mode off the block grid: per-sweep launches (sweep_log_kernel), the fused strip kernel and AUTO's
    choice (strips, or the whole level in one workgroup)."""
    check_level(ctx, oracle, w, h, cw, ch, 7, outer, inner, algorithm)


@pytest.mark.parametrize("algorithm", [2, 0])
@pytest.mark.parametrize("outer,inner", [(1, 6), (2, 7), (3, 8), (1, 10), (4, 11), (1, 16)])
@pytest.mark.parametrize("w,h,cw,ch", [(100, 70, 128, 80), (640, 520, 640, 520)])
def test_solve_level_more_than_five_sweeps(ctx, oracle, w, h, cw, ch, outer, inner, algorithm):
    """More sweeps per outer iteration than one strip launch holds: the continuation launches of the Log instances."""
    check_level(ctx, oracle, w, h, cw, ch, 17, outer, inner, algorithm)


@pytest.mark.parametrize("outer,inner", [(2, 3), (3, 5), (1, 7), (2, 0), (0, 3)])
@pytest.mark.parametrize("w,h", [(5, 4), (16, 8), (64, 16), (33, 17), (64, 32), (40, 33), (64, 64), (52, 61), (2, 2)])
def test_single_workgroup(ctx, flow2d, oracle, w, h, outer, inner):
    """small_level_kernel with log = 1: the whole level in one workgroup."""
    rdu, planes = check_level(ctx, oracle, w, h, 64, 64, 9, outer, inner, flow2d.SOLVER_SINGLE_WORKGROUP)
    assert rdu is planes[0]


@pytest.mark.parametrize("algorithm", [1, 2, 0])
@pytest.mark.parametrize("case", ["zero frames", "constant frames", "alpha 0", "epsilon 0", "huge values"])
def test_solve_level_degenerate_inputs(ctx, oracle, case, algorithm):
    """The cases of test_gpu_kernels.py::test_solve_level_degenerate_inputs with the log-derivative term: zeros, infinities and NaNs
    come out where the oracle's IEEE arithmetic puts them."""
    w, h, cw, ch = 150, 90, 160, 96
    f0, f1, u, v, _, _ = level_fields(oracle, w, h, 23)
    alpha, eps = ALPHA, 0.001
    if case == "zero frames":
        f0, f1 = np.zeros_like(f0), np.zeros_like(f1)
    elif case == "constant frames":
        f0, f1 = np.full_like(f0, 17.0), np.full_like(f1, 17.0)
    elif case == "alpha 0":
        alpha = 0.0
    elif case == "epsilon 0":
        eps = 0.0
        u, v = np.zeros_like(u), np.zeros_like(v)
    else:
        f0, f1 = f0 * np.float32(1e18), f1 * np.float32(1e18)
    hx, hy = np.float32(cw / w), np.float32(ch / h)
    d = [up(ctx, a, cw, ch) for a in (f0, f1, u, v)]
    planes = [ctx.plane(cw, ch).fill_bytes(0x7f) for _ in range(6)]
    rdu, rdv = ctx.solve_level(*d, *planes, w, h, hx, hy, alpha, eps, eps, 2, 3, LOG, algorithm)
    with oracle.device_logs(ctx), np.errstate(all="ignore"):
        odu, odv, _, _ = oracle.solve_level(f0, f1, u, v, w, h, hx, hy, alpha, eps, eps, 2, 3, LOG)
    assert differing(rdu.download(w, h), odu) == 0 and differing(rdv.download(w, h), odv) == 0


# ---- g. pixels only the logarithm cares about ------------------------------------------------------------------------------------
SPECIALS = [-1.0, -3.0, 0.0, 1e30, np.inf, np.nan]


def special_frames(oracle, w, h):
    """Frame 0 with isolated special pixels in the four corners, on both sides of 16 x 8 block edges and in the interior;
    frame 1 with 8 x 8 blocks of them in the bottom right corner, across a block corner and inside one block."""
    f0, f1, u, v, _, _ = level_fields(oracle, w, h, 23)
    f0, f1 = f0.copy(), f1.copy()
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1),                      # corners
             (7, 15), (8, 16), (7, 31), (8, 32), (15, 16), (16, 15), (23, 31), (24, 32),  # block edges, both sides
             (3, 5), (11, 21), (19, 9), (20, 26), (27, 37), (29, 3)]              # inside blocks
    for k, (y, x) in enumerate(spots):
        f0[y % h, x % w] = SPECIALS[k % 6]
    tile = np.array(SPECIALS * 11, np.float32)[:64].reshape(8, 8)
    for y, x in ((h - 8, w - 8), (12, 28), (16, 16)):  # corner of the image; across the corner of four blocks; one whole block row
        f1[y:y + 8, x:x + 8] = tile
    return f0, f1, u, v


@pytest.mark.parametrize("w,h,cw,ch,algorithm", [(150, 90, 160, 96, 1), (150, 90, 160, 96, 2), (150, 90, 160, 96, 0), (40, 33, 64, 64, 3)])
def test_special_pixels(ctx, oracle, w, h, cw, ch, algorithm):
    """I = -1 (log -> -inf), I < -1 (NaN), 0, 1e30, +inf and NaN in the frames: the same pixels NaN as in the oracle, every other
    word equal, for the per-sweep kernels, the strips, AUTO and the single-workgroup kernel."""
    f0, f1, u, v = special_frames(oracle, w, h)
    hx, hy = np.float32(cw / w), np.float32(ch / h)
    d = [up(ctx, a, cw, ch) for a in (f0, f1, u, v)]
    planes = [ctx.plane(cw, ch).fill_bytes(0x7f) for _ in range(6)]
    rdu, rdv = ctx.solve_level(*d, *planes, w, h, hx, hy, ALPHA, 0.001, 0.001, 2, 3, LOG, algorithm)
    with oracle.device_logs(ctx), np.errstate(all="ignore"):
        odu, odv, _, _ = oracle.solve_level(f0, f1, u, v, w, h, hx, hy, ALPHA, 0.001, 0.001, 2, 3, LOG)
    assert 0 < np.isnan(odu).sum() < odu.size  # the specials did something, and left some of the level alone
    assert differing(rdu.download(w, h), odu) == 0 and differing(rdv.download(w, h), odv) == 0


# ---- h. pipelines ------------------------------------------------------------------------------------------------------------------
_pairs = {}


def pipeline_pair(oracle, w, h):
    if (w, h) not in _pairs:
        _pairs[(w, h)] = oracle.synthetic_pair(w, h, 1.5, -0.75, seed=1, noise=True)
    return _pairs[(w, h)]


@pytest.mark.parametrize("alpha", [0.0005, 0.02])
@pytest.mark.parametrize("w,h,levels,scale", [(256, 128, 4, 0.5), (333, 207, 5, 0.75), (100, 70, 4, 0.8)])
def test_compute_flow(ctx, flow2d, oracle, RK, w, h, levels, scale, alpha):
    """OpticalFlow2D::ComputeFlow in Log mode against the oracle's pyramid under device_logs, every pixel: on the block grid
    at every level (256 x 128, where the reference's kernels pin both) and with every level off it."""
    f0, f1 = pipeline_pair(oracle, w, h)
    p = (levels, scale, 3, 5, alpha, 0.001, 0.001, 5, 1.5)
    flow = flow2d.OpticalFlow(w, h, LOG)
    try:
        u, v, _ = flow.compute_flow(f0, f1, flow.params(*p))
    finally:
        flow.close()
    with oracle.device_logs(ctx):
        ou, ov, _ = oracle.compute_flow(f0, f1, *p, LOG)
    assert float(np.abs(ou).max()) > 0.01
    assert differing(u, ou) == 0 and differing(v, ov) == 0
    if (w, h) == (256, 128):
        with RK.RefKernels(w, h) as R:
            ru, rv, _, _ = R.compute_flow(f0, f1, *p, constancy=RK.LOG_DERIVATIVES)
        assert differing(ou, ru) == 0 and differing(ov, rv) == 0


# ---- f. the strip kernel's guards in Log mode --------------------------------------------------------------------------------------
# The constructions of tests/test_gpu_fused.py.  In each of them the operand that trips the guard sits in the flow, in alpha,
# in the regularisers or in the spacing -- none of which the logarithm touches -- or (the robustifier's 1e18 frames) in phi / ksi,
# which every data term forms from the frames as they are (compute_phi_ksi has no Log form).  So the Log twins keep the Grey
# tests' frames: their expm1 would not even exist, e^x leaves float32 above x = 88.7 and those frames reach 218.
# Left out: test_a_diffusion_front_trips_the_guard_only_where_it_is.  Its bump in the flow (rows 300-302, columns 500-502) spreads
# one pixel per sweep in Grey mode and decays below 2^-80 on the way.  solve_2d_log takes a block's own edge pixel for the flow
# neighbours, so the increment never leaves the 16 x 8 block of the bump (rows 296-303, columns 496-511): after the test's 8 x 5
# sweeps the oracle's smallest non-zero |du| is 1.07e-14 -- ten orders of magnitude above the guard's 2^-80 = 8.3e-25: no front,
# and no fallback to count.
def strips_vs_oracle(ctx, oracle, f0, f1, u, v, w, h, hx, hy, alpha, outer, inner, e_smooth=0.001, e_data=0.001, algorithm=2):
    d = [up(ctx, a, w, h) for a in (f0, f1, u, v)]
    planes = [ctx.plane(w, h).fill_bytes(0x7f) for _ in range(6)]
    before, plain = ctx.fused_fallbacks(), ctx.fused_plain_waves()
    rdu, rdv = ctx.solve_level(*d, *planes, w, h, hx, hy, alpha, e_smooth, e_data, outer, inner, LOG, algorithm)
    got = rdu.download(w, h), rdv.download(w, h)
    moved = ctx.fused_fallbacks() - before, ctx.fused_plain_waves() - plain
    with oracle.device_logs(ctx), np.errstate(all="ignore"):
        odu, odv, _, _ = oracle.solve_level(f0, f1, u, v, w, h, hx, hy, alpha, e_smooth, e_data, outer, inner, LOG)
    return differing(got[0], odu) + differing(got[1], odv), moved[0], moved[1], odu


ONE = np.float32(1.0)


def test_strip_guard_ordinary_operands(ctx, oracle):
    f0, f1, u, v, _, _ = level_fields(oracle, 640, 520, 11)
    assert strips_vs_oracle(ctx, oracle, f0, f1, u, v, 640, 520, ONE, ONE, 35.0, 3, 5)[:2] == (0, 0)


@pytest.mark.parametrize("inner", [5, 3])
def test_strip_guard_tiny_numerators(ctx, oracle, inner):
    """Flat frames, a flow of magnitude 1e-30 (test_tiny_numerators_fall_back_to_the_plain_division): falls back, oracle's words."""
    w, h = 640, 260
    rng = np.random.default_rng(5)
    f0 = np.full((h, w), 100.0, np.float32)
    u = (rng.normal(0, 1, (h, w)) * 1e-30).astype(np.float32)
    v = (rng.normal(0, 1, (h, w)) * 1e-30).astype(np.float32)
    diff, fell, _, odu = strips_vs_oracle(ctx, oracle, f0, f0.copy(), u, v, w, h, ONE, ONE, 35.0, 2, inner)
    assert 0 < float(np.abs(odu).max()) < 1e-25
    assert diff == 0 and fell > 0


def test_strip_guard_denominators_outside_the_range(ctx, oracle):
    f0, f1, u, v, _, _ = level_fields(oracle, 640, 200, 21)
    diff, fell, _, _ = strips_vs_oracle(ctx, oracle, f0, f1, u, v, 640, 200, ONE, ONE, 1e22, 2, 5)
    assert diff == 0 and fell > 0


@pytest.mark.parametrize("alpha,fuses", [(1e-29, True), (1e-31, False), (0.0, True), (3e-36, False)])
def test_strip_guard_weights_the_strips_cannot_halve(ctx, flow2d, oracle, alpha, fuses):
    w, h = 1300, 300
    f0, f1, u, v, _, _ = level_fields(oracle, w, h, 27)
    assert strips_vs_oracle(ctx, oracle, f0, f1, u, v, w, h, ONE, ONE, alpha, 2, 5, algorithm=0)[0] == 0
    if fuses:
        assert strips_vs_oracle(ctx, oracle, f0, f1, u, v, w, h, ONE, ONE, alpha, 2, 5)[0] == 0
    else:
        with pytest.raises(flow2d.Flow2DError) as e:
            strips_vs_oracle(ctx, oracle, f0, f1, u, v, w, h, ONE, ONE, alpha, 2, 5)
        assert e.value.status == 5


def test_strip_guard_overflowing_results(ctx, oracle):
    """An infinite patch in the flow (test_overflowing_results_match_the_per_sweep_kernels): here against the oracle itself."""
    w, h = 640, 200
    f0, f1, u, v, _, _ = level_fields(oracle, w, h, 23)
    u = u.copy()
    u[50:60, 100:400] = np.inf
    diff, fell, _, odu = strips_vs_oracle(ctx, oracle, f0, f1, u, v, w, h, ONE, ONE, 35.0, 2, 5)
    assert not np.isfinite(odu).all()
    assert diff == 0 and fell > 0


def test_strip_guard_negative_zero_in_the_flow(ctx, oracle):
    w, h = 640, 200
    f0 = np.full((h, w), 80.0, np.float32)
    u, v = np.full((h, w), -0.0, np.float32), np.zeros((h, w), np.float32)
    diff, fell, _, _ = strips_vs_oracle(ctx, oracle, f0, f0.copy(), u, v, w, h, ONE, ONE, 35.0, 2, 5)
    assert diff == 0 and fell > 0


@pytest.mark.parametrize("e_smooth,e_data,scale,trips", [(1e-8, 1e-8, 1.0, False), (1e-20, 0.001, 1.0, True), (0.001, 1e-20, 1.0, True),
                                                         (0.001, 0.001, 1e16, True)])
def test_strip_guard_robustifier_arguments(ctx, oracle, e_smooth, e_data, scale, trips):
    w, h = 640, 200
    f0, f1, u, v, _, _ = level_fields(oracle, w, h, 41)
    f0, f1 = (f0 * np.float32(scale)).astype(np.float32), (f1 * np.float32(scale)).astype(np.float32)
    u, v = u.copy(), v.copy()
    u[40:120, 100:500] = 0.25
    v[40:120, 100:500] = -0.5
    f1[60:100, 200:400] = f0[60:100, 200:400]
    diff, fell, _, _ = strips_vs_oracle(ctx, oracle, f0, f1, u, v, w, h, ONE, ONE, 35.0, 2, 5, e_smooth=e_smooth, e_data=e_data)
    assert diff == 0
    if trips:
        assert fell > 0


@pytest.mark.parametrize("hx,hy", [(1.1, 0.9), (3.7, 1.0), (0.013, 0.02)])
def test_strip_guard_spacings_that_are_no_powers_of_two(ctx, oracle, hx, hy):
    f0, f1, u, v, _, _ = level_fields(oracle, 640, 264, 51)
    diff, fell, _, _ = strips_vs_oracle(ctx, oracle, f0, f1, u, v, 640, 264, np.float32(hx), np.float32(hy), 35.0, 2, 5)
    assert diff == 0
    if hx >= 1.0:
        assert fell == 0


def test_strip_guard_tiny_differences_over_a_spacing(ctx, oracle):
    w, h = 640, 200
    rng = np.random.default_rng(7)
    f0, f1, _, _, _, _ = level_fields(oracle, w, h, 53)
    u = (rng.normal(0, 1, (h, w)) * 1e-30).astype(np.float32)
    v = (rng.normal(0, 1, (h, w)) * 1e-30).astype(np.float32)
    diff, fell, _, _ = strips_vs_oracle(ctx, oracle, f0, f1, u, v, w, h, np.float32(1.1), np.float32(1.1), 35.0, 1, 5)
    assert diff == 0 and fell > 0


def test_strip_guard_spacing_outside_the_guarded_range(ctx, oracle):
    f0, f1, u, v, _, _ = level_fields(oracle, 640, 200, 55)
    diff, fell, plain, _ = strips_vs_oracle(ctx, oracle, f0, f1, u, v, 640, 200, np.float32(3.0 * 2.0 ** 40), np.float32(1.1), 35.0, 1, 5)
    assert diff == 0 and plain > 0 and fell == 0
