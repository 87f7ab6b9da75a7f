"""flow2d_deformation_2d restated in numpy from the text of include/flow2d_c_abi.h (np.float32 operations in the stated order),
with its statistics, and what can be checked without a device: the restatement against numpy.gradient, exact linear fields, a
3-4-5 rotation, the masking (no output depends on a vector that is not ok) and the entry's host-side refusals."""
import ctypes

import numpy as np
import pytest

F32 = np.float32
U32 = np.uint32
SMALL, GREEN = 0, 1  # flow2d_strain_measure
PLANES = ("divergence", "vorticity", "dilatation", "exx", "eyy", "exy", "e1", "e2", "max_shear")
STAT_NAMES = ("divergence", "vorticity", "dilatation", "e1", "e2", "max_shear")
MOMENTS_DTYPE = np.dtype([("sum", "<f8"), ("sum_sq", "<f8"), ("min", "<f4"), ("max", "<f4")])
STATS_DTYPE = np.dtype([("valid", "<u8"), ("invalid", "<u8")] + [(n, MOMENTS_DTYPE) for n in STAT_NAMES] + [("reserved", "<u8", 12)])
assert STATS_DTYPE.itemsize == 256
NAN = F32(np.nan)
assert NAN.view(U32) == 0x7FC00000
HALF = F32(0.5)


def vectors_ok(u, v, mask):
    """ok(q) of the definition for every pixel of the frame."""
    with np.errstate(invalid="ignore"):
        ok = (np.abs(u) <= F32(1e9)) & (np.abs(v) <= F32(1e9))
        if mask is not None:
            m = np.array(mask, F32)
            m[~(m <= 1)] = 1
            m[~(m >= 0)] = 0
            ok &= m < HALF
    return ok


def masked_difference(f, ok, axis):
    """(difference, has one) along `axis`: central where both neighbours are ok, one-sided where one is."""
    f = np.moveaxis(f, axis, 1)
    ok = np.moveaxis(ok, axis, 1)
    n = f.shape[1]
    lo_ok = np.zeros_like(ok)
    hi_ok = np.zeros_like(ok)
    lo_ok[:, 1:] = ok[:, :-1]
    hi_ok[:, :-1] = ok[:, 1:]
    lo = f[:, np.maximum(np.arange(n) - 1, 0)]
    hi = f[:, np.minimum(np.arange(n) + 1, n - 1)]
    with np.errstate(all="ignore"):
        both, forward, backward = (hi - lo) * HALF, hi - f, f - lo
    d = np.where(lo_ok, np.where(hi_ok, both, backward), np.where(hi_ok, forward, NAN)).astype(F32)
    return np.moveaxis(d, 1, axis), np.moveaxis(lo_ok | hi_ok, 1, axis)


def deformation_reference(u, v, mask=None, measure=SMALL):
    """{plane name: [h, w] float32} for the nine planes, "gradient" (a, b, c, d before the NaN fill), "valid" and "stats" (one
    STATS_DTYPE record), with "abs_sum" / "abs_sum_sq": the sums of |term| of the record's double sums."""
    u, v = np.ascontiguousarray(u, F32), np.ascontiguousarray(v, F32)
    ok = vectors_ok(u, v, mask)
    a, has_x = masked_difference(u, ok, 1)
    c, _ = masked_difference(v, ok, 1)
    b, has_y = masked_difference(u, ok, 0)
    d, _ = masked_difference(v, ok, 0)
    valid = ok & has_x & has_y
    with np.errstate(all="ignore"):
        q = {"divergence": a + d, "vorticity": c - b, "dilatation": (a + d) + (a * d - b * c)}
        if measure == SMALL:
            exx, eyy, exy = a, d, HALF * (b + c)
        else:
            assert measure == GREEN
            exx = a + HALF * (a * a + c * c)
            eyy = d + HALF * (b * b + d * d)
            exy = HALF * ((b + c) + (a * b + c * d))
        mean, half = HALF * (exx + eyy), HALF * (exx - eyy)
        shear = np.sqrt(half * half + exy * exy)
        q.update(exx=exx, eyy=eyy, exy=exy, e1=mean + shear, e2=mean - shear, max_shear=shear)
    out = {}
    for name in PLANES:
        assert q[name].dtype == F32
        out[name] = np.where(valid, q[name], NAN).astype(F32)
    stats = np.zeros(1, STATS_DTYPE)
    n = int(valid.sum())
    stats["valid"], stats["invalid"] = n, valid.size - n
    out["abs_sum"], out["abs_sum_sq"] = {}, {}
    for name in STAT_NAMES:
        x = out[name][valid].astype(np.float64)  # raster order
        stats[name]["sum"], stats[name]["sum_sq"] = x.sum(), (x * x).sum()
        if n:
            stats[name]["min"], stats[name]["max"] = x.min(), x.max()
        out["abs_sum"][name], out["abs_sum_sq"][name] = float(np.abs(x).sum()), float((x * x).sum())
    out.update(gradient=(a, b, c, d), valid=valid, stats=stats)
    return out


def random_flow(rng, w, h, scale=3.0):
    return (rng.standard_normal((h, w)) * scale).astype(F32), (rng.standard_normal((h, w)) * scale).astype(F32)


def masked_case(w, h, seed=7, soft=False):
    """A flow with a sprinkle of NaN and infinite vectors and a random mask of about 30 % (binary, or soft: values in [0, 1]
    with NaN, negative and > 1 entries, 30 % of them >= 0.5)."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    u, v = random_flow(rng, w, h)
    wild = rng.random((h, w))
    u[wild < 0.02] = np.nan
    v[(wild >= 0.02) & (wild < 0.04)] = np.inf
    u[(wild >= 0.04) & (wild < 0.05)] = -np.inf
    v[(wild >= 0.05) & (wild < 0.06)] = F32(2e9)
    r = rng.random((h, w))
    if not soft:
        mask = (r < 0.3).astype(F32)
    else:
        mask = np.where(r < 0.3, 0.5 + 0.5 * rng.random((h, w)), 0.4999 * rng.random((h, w))).astype(F32)
        odd = rng.random((h, w))
        mask[odd < 0.03] = np.nan   # clamps to 1: left out
        mask[(odd >= 0.03) & (odd < 0.06)] = -2.0  # clamps to 0: kept
        mask[(odd >= 0.06) & (odd < 0.09)] = 7.0   # clamps to 1: left out
    return u, v, mask


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


@pytest.mark.parametrize("w,h", [(2, 2), (2, 9), (9, 2), (5, 7), (65, 33)])
def test_unmasked_finite_flow_is_numpy_gradient(w, h):
    u, v = random_flow(np.random.default_rng(w * 100 + h), w, h)
    ref = deformation_reference(u, v)
    a, b, c, d = ref["gradient"]
    uy, ux = np.gradient(u, edge_order=1)
    vy, vx = np.gradient(v, edge_order=1)
    assert ux.dtype == F32
    for got, want, what in ((a, ux, "u_x"), (b, uy, "u_y"), (c, vx, "v_x"), (d, vy, "v_y")):
        assert np.array_equal(bits(got), bits(want)), what
    assert ref["valid"].all() and ref["stats"]["valid"][0] == w * h and ref["stats"]["invalid"][0] == 0
    assert np.array_equal(bits(ref["divergence"]), bits(ux + vy))


@pytest.mark.parametrize("w,h", [(2, 2), (7, 3), (64, 64), (33, 64)])
def test_exact_linear_fields(w, h):
    """u = 0.25 x - 0.5 y, v = 0.125 x + 0.375 y: every flow value and every difference is exact in fp32, so every plane is
    constant, borders included, and equal to the value worked out by hand."""
    y, x = np.mgrid[0:h, 0:w].astype(F32)
    u, v = F32(0.25) * x - F32(0.5) * y, F32(0.125) * x + F32(0.375) * y
    a, b, c, d = 0.25, -0.5, 0.125, 0.375
    first = {"divergence": 0.625, "vorticity": 0.625, "dilatation": 0.625 + (0.09375 + 0.0625)}
    strain = {SMALL: (0.25, 0.375, -0.1875),
              GREEN: (0.25 + 0.5 * (0.0625 + 0.015625), 0.375 + 0.5 * (0.25 + 0.140625), 0.5 * (-0.375 + (-0.125 + 0.046875)))}
    assert strain[GREEN] == (0.2890625, 0.5703125, -0.2265625)
    for measure in (SMALL, GREEN):
        ref = deformation_reference(u, v, None, measure)
        exx, eyy, exy = (F32(t) for t in strain[measure])
        mean, half = HALF * (exx + eyy), HALF * (exx - eyy)
        shear = np.sqrt(F32(half * half + exy * exy))
        want = dict(first, exx=exx, eyy=eyy, exy=exy, e1=F32(mean + shear), e2=F32(mean - shear), max_shear=shear)
        for name in PLANES:
            assert (bits(ref[name]) == F32(want[name]).view(U32)).all(), (measure, name)
        s = ref["stats"][0]
        assert s["valid"] == w * h and s["divergence"]["min"] == s["divergence"]["max"] == F32(0.625)
        assert s["divergence"]["sum"] == 0.625 * w * h and s["divergence"]["sum_sq"] == 0.390625 * w * h
    assert (a, b, c, d) == tuple(float(t[0, 0]) for t in ref["gradient"])


def test_rotation_has_no_green_lagrange_strain():
    """The 3-4-5 rotation about the origin, cos = 0.6 and sin = 0.8: x' = 0.6 x - 0.8 y, y' = 0.8 x + 0.6 y, so u = -0.4 x - 0.8 y
    and v = 0.8 x - 0.4 y, with cos^2 + sin^2 = 1 exactly in rationals.  0.4 and 0.8 are not fp32 numbers, so on the unit pixel
    grid the flow cannot be exact beyond the origin's row and column: it is formed in double and rounded once, an error of at
    most ulp/2 = 2^-24 |flow| per value (delta below).  A difference of two such values is then off by at most 2 delta (the
    subtraction and the halving of values this close are exact or add one rounding of a number below 1: 2^-24), so every entry
    of the gradient is within g = 2 delta + 2^-24 of (-0.4, -0.8, 0.8, -0.4).  E is exactly 0 at the true gradient; its partial
    derivatives there are at most 1 + |a| + |b| + |c| + |d| < 4 in sum for each entry, the second-order term is below g, and the
    six to eight fp32 operations of an entry, all on magnitudes below 1, add at most 8 * 2^-24:  bound = 4 g + g + 8 * 2^-24.
    The small strain of a rotation is not zero: exx = cos - 1 = -0.4, to within g everywhere, and bit for bit at the origin,
    where the forward difference is fl(-0.4) - 0."""
    n = 16
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    u, v = (-0.4 * x - 0.8 * y).astype(F32), (0.8 * x - 0.4 * y).astype(F32)
    unit = 2.0 ** -24
    delta = unit * float(max(np.abs(u).max(), np.abs(v).max()))
    g = 2 * delta + unit
    bound = 5 * g + 8 * unit
    assert bound < 2e-5
    green = deformation_reference(u, v, None, GREEN)
    for name in ("exx", "eyy", "exy", "e1", "e2", "max_shear"):
        assert np.abs(green[name]).max() <= (bound if name in ("exx", "eyy", "exy") else 2 * bound + 2 * unit), name
    small = deformation_reference(u, v, None, SMALL)
    assert np.abs(small["exx"].astype(np.float64) + 0.4).max() <= g
    assert small["exx"][0, 0] == F32(-0.4) and small["eyy"][0, 0] == F32(-0.4)
    assert np.abs(small["vorticity"].astype(np.float64) - 1.6).max() <= 2 * g + unit  # 2 sin


def neighbour_patterns(ok, axis):
    """Which of (both, low only, high only, neither) occur along `axis` among the pixels that are ok themselves."""
    okp = np.pad(ok, 1, constant_values=False)
    core = (slice(1, -1), slice(1, -1))
    lo = np.roll(okp, 1, axis)[core]
    hi = np.roll(okp, -1, axis)[core]
    return {(bool(l), bool(r)) for l, r in zip(lo[ok], hi[ok])}


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("measure", [SMALL, GREEN])
def test_masked_vectors_reach_no_output(soft, measure):
    w, h = 37, 29
    u, v, mask = masked_case(w, h, soft=soft)
    ok = vectors_ok(u, v, mask)
    every = {(True, True), (True, False), (False, True), (False, False)}
    assert neighbour_patterns(ok, 1) == every and neighbour_patterns(ok, 0) == every, "a bad fixture: not every neighbour pattern"
    assert not np.isfinite(u).all() and not np.isfinite(v).all()
    ref = deformation_reference(u, v, mask, measure)
    assert 0 < ref["stats"]["valid"][0] < w * h
    masked = ~(vectors_ok(np.zeros_like(u), np.zeros_like(v), mask))
    assert masked.sum() > 100
    rng = np.random.default_rng(5)
    for fill in (np.nan, np.inf, 1e30, None):
        u2, v2 = u.copy(), v.copy()
        u2[masked] = fill if fill is not None else rng.standard_normal(int(masked.sum())).astype(F32) * 100
        v2[masked] = fill if fill is not None else rng.standard_normal(int(masked.sum())).astype(F32) * 100
        other = deformation_reference(u2, v2, mask, measure)
        for name in PLANES:
            assert np.array_equal(bits(other[name]), bits(ref[name])), (name, fill)
        assert other["stats"].tobytes() == ref["stats"].tobytes()
    # an invalid pixel holds the one NaN, a valid one a finite value
    for name in PLANES:
        assert (bits(ref[name])[~ref["valid"]] == 0x7FC00000).all() and np.isfinite(ref[name][ref["valid"]]).all()


def test_empty_and_single_sets():
    u, v = random_flow(np.random.default_rng(1), 6, 5)
    ref = deformation_reference(u, v, np.ones_like(u))
    s = ref["stats"][0]
    assert s["valid"] == 0 and s["invalid"] == 30 and s["e1"]["min"] == 0 and s["e1"]["max"] == 0 and s["e1"]["sum"] == 0
    lone = np.ones_like(u)
    lone[2, 3] = 0
    assert deformation_reference(u, v, lone)["stats"]["valid"][0] == 0  # a lone vector has no derivative


# ---- the entry's host side ------------------------------------------------------------------------------------------------------
def test_workspace_bytes_and_refusals_without_a_device(flow2d):
    lib = flow2d.hip_lib()
    assert hasattr(lib, "flow2d_deformation_2d") and hasattr(lib, "flow2d_deformation_workspace_bytes")
    ws_bytes = lib.flow2d_deformation_workspace_bytes
    ws_bytes.restype = ctypes.c_size_t
    ws_bytes.argtypes = [ctypes.c_size_t] * 3
    assert ws_bytes(0, 5, 1) == ws_bytes(5, 0, 1) == ws_bytes(5, 5, 0) == 0
    one = ws_bytes(1, 1, 1)
    assert one > 0 and one % 16 == 0
    # one slab per workgroup of 64 columns x 16 rows and instance
    assert ws_bytes(64, 16, 1) == one and ws_bytes(65, 16, 1) == 2 * one and ws_bytes(64, 17, 1) == 2 * one
    assert ws_bytes(4096, 4096, 3) == 64 * 256 * 3 * one and ws_bytes(300, 37, 2) == 5 * 3 * 2 * one
    assert C_sizeof_stats(flow2d) == 256

    fake = ctypes.create_string_buffer(4096)
    ctx = ctypes.addressof(fake)
    # (the argument types are the package's own, set when the library is loaded: flow2d.DeformationPlanes is the host struct)
    w, h, pitch = 100, 40, 512
    span = pitch * h
    base = 1 << 20
    at = lambda k: base + k * (span + 4096)  # noqa: E731  (addresses only: nothing is dereferenced before the device is entered)
    need = ws_bytes(w, h, 1)
    d = dict(ctx=ctx, u=at(0), v=at(1), mask=at(2), w=w, h=h, pitch=pitch, measure=SMALL, stats=at(12), ws=at(13), ws_bytes=need,
             planes={name: at(3 + k) for k, name in enumerate(PLANES)}, out=True)

    def call(**kw):
        a = dict(d, **kw)
        out = flow2d.DeformationPlanes(**a["planes"])
        return lib.flow2d_deformation_2d(a["ctx"], a["u"], a["v"], a["mask"], a["w"], a["h"], a["pitch"], a["measure"],
                                         ctypes.byref(out) if a["out"] else None, a["stats"], a["ws"], a["ws_bytes"])

    bad = [dict(ctx=None), dict(u=None), dict(v=None), dict(out=False, stats=None), dict(planes={}, stats=None), dict(w=1), dict(h=1),
           dict(w=0), dict(pitch=pitch + 8), dict(pitch=396), dict(pitch=16), dict(measure=2), dict(measure=-1), dict(u=at(0) + 4),
           dict(mask=at(2) + 8), dict(planes={"e1": at(3) + 4}), dict(stats=at(12) + 4), dict(ws=at(13) + 8), dict(ws=None),
           dict(ws_bytes=need - 1), dict(ws_bytes=0),
           # aliasing: an output on an input, two outputs equal or overlapping, the record or the workspace on a plane, the record
           # inside the workspace
           dict(planes={"divergence": at(0)}), dict(planes={"max_shear": at(1) + pitch}), dict(planes={"exx": at(2)}),
           dict(planes={"exx": at(5), "exy": at(5)}), dict(planes={"e1": at(6), "e2": at(6) + span - pitch}), dict(stats=at(0) + 64),
           dict(stats=at(4)), dict(ws=at(1)), dict(ws=at(7) + 32), dict(stats=at(13) + 16), dict(stats=at(13) + need - 8)]
    for kw in bad:
        assert call(**kw) == 1, kw
    # (only refusals here: an accepted call would go on to launch on these made-up addresses where there is a device; the
    # accepted forms are the business of tests/test_gpu_deformation.py)


def C_sizeof_stats(flow2d):
    return ctypes.sizeof(flow2d.DeformationStats)


def test_python_record_matches_the_restatement_layout(flow2d):
    rec = flow2d.DeformationStats()
    rec.valid, rec.invalid = 5, 7
    rec.e2.sum_sq, rec.max_shear.max = 2.5, 3.5
    a = np.frombuffer(bytes(rec), STATS_DTYPE)[0]
    assert a["valid"] == 5 and a["invalid"] == 7 and a["e2"]["sum_sq"] == 2.5 and a["max_shear"]["max"] == 3.5
    assert flow2d.DEFORMATION_PLANES == PLANES and flow2d.DEFORMATION_STATS == STAT_NAMES
    assert (flow2d.STRAIN_SMALL, flow2d.STRAIN_GREEN_LAGRANGE) == (SMALL, GREEN)
    H = flow2d.host_lib()
    assert H.flow2d_host_deformation_args_ok(SMALL, 0.0) == 1 and H.flow2d_host_deformation_args_ok(GREEN, 8.5) == 1
    for measure, sigma in ((2, 0.0), (-1, 1.0), (SMALL, -0.5), (SMALL, float("nan")), (GREEN, 9.0), (GREEN, float("inf"))):
        assert H.flow2d_host_deformation_args_ok(measure, sigma) == 0, (measure, sigma)
