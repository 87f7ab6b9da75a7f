"""flow2d_bspline_prefilter_2d and the sampling step of flow2d_subset_refine_spline_2d / flow2d_subset_refine2_spline_2d restated in
numpy from the text of include/flow2d_c_abi.h.  The node loops are the existing restatements' (tests/test_subset_cpu.py,
test_subset_sequence_cpu.py, test_subset_masked_cpu.py, test_subset2_cpu.py): spline_sampler() puts bspline_sample in the place
of their module-level cubic_sample for the length of a with-block and puts it back, and the frame-1 argument is then the
coefficient plane.  The three summation orders stay available (all_orders_spline, all_orders2_spline).
What can be checked without a device: the prefilter against a brute-force evaluation of the definition and against the
interpolation condition, the accuracy on the six scenes and the bending scenes against the Catmull-Rom restatement on the same
starts -- the tables of profiles/subset_spline/table_numpy.md, which tools/subset_spline_table.py prints from the rows below --,
and the entries' host-side refusals."""
import contextlib
import ctypes
import functools
import json

import numpy as np
import pytest

import test_subset2_cpu
import test_subset_cpu
import test_subset_masked_cpu
import test_subset_sequence_cpu
from test_correlate_cpu import F32, bits
from test_subset_cpu import F64, ORDERS, SCENE_CASES, small_case

HORIZON = 16
ROOT3 = np.sqrt(F64(3.0))
Z = ROOT3 - 2.0
ZJ = [F64(1.0)]
for _ in range(HORIZON):
    ZJ.append(ZJ[-1] * Z)
G = ROOT3 / 6.0
RESTATEMENTS = (test_subset_cpu, test_subset_sequence_cpu, test_subset_masked_cpu, test_subset2_cpu)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def reflect(i, n):
    """reflect(i, n) of the header, for integer arrays."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)  # (numpy's mod of a positive p is non-negative)
    return np.where(m <= n - 1, m, p - m)


def prefilter_lines(s):
    """d of the header for every line s[r, :] of a float64 array."""
    n = s.shape[1]
    k = np.arange(n)
    acc = np.zeros_like(s)
    for j in range(HORIZON, 0, -1):
        acc = acc + ZJ[j] * (s[:, reflect(k - j, n)] + s[:, reflect(k + j, n)])
    acc = acc + s
    return G * acc


def bspline_prefilter_reference(plane):
    """flow2d_bspline_prefilter_2d: rows on the floats converted to double, columns on the rows' doubles, cast to float."""
    with np.errstate(all="ignore"):
        rows = prefilter_lines(np.asarray(plane, F32).astype(F64))
        return prefilter_lines(rows.T).T.astype(F32)


def bspline_weights(t):
    u = 1.0 - t
    return ((u * u) * u, ((3.0 * t - 6.0) * t) * t + 4.0, ((3.0 * u - 6.0) * u) * u + 4.0, (t * t) * t)


def bspline_sample(coeff, x, y):
    """g of flow2d_subset_refine_spline_2d at positions inside the frame (float64 arrays); coeff: the coefficient plane as float64."""
    h, w = coeff.shape
    fx, fy = np.floor(x), np.floor(y)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    wx, wy = bspline_weights(x - fx), bspline_weights(y - fy)
    cols = [reflect(ix - 1 + i, w) for i in range(4)]
    rows = []
    for j in range(4):
        row = reflect(iy - 1 + j, h)
        a = [coeff[row, c] for c in cols]
        rows.append(((wx[0] * a[0] + wx[1] * a[1]) + wx[2] * a[2]) + wx[3] * a[3])
    return ((wy[0] * rows[0] + wy[1] * rows[1]) + wy[2] * rows[2]) + wy[3] * rows[3]


@contextlib.contextmanager
def spline_sampler():
    """The existing restatements sample with bspline_sample inside the block; their own cubic_sample is put back on the way out."""
    kept = [m.cubic_sample for m in RESTATEMENTS]
    try:
        for m in RESTATEMENTS:
            m.cubic_sample = bspline_sample
        yield
    finally:
        for m, f in zip(RESTATEMENTS, kept):
            m.cubic_sample = f


def subset_refine_spline_reference(frame_0, coeff_1, node_u0, node_v0, start_gradients, mask, min_pixels, r, s, R, **kw):
    """flow2d_subset_refine_spline_2d as a Refined.  mask None: the bytes of a mask that excludes nothing, which are those of the
    unmasked node loop (tests/test_subset_masked_cpu.py asserts that equivalence of the two loops)."""
    with spline_sampler():
        return test_subset_masked_cpu.subset_refine_masked_reference(frame_0, coeff_1, node_u0, node_v0, start_gradients, mask, min_pixels, r, s,
                                                                     R, **kw)


def subset_refine2_spline_reference(frame_0, coeff_1, node_u0, node_v0, r, s, R, **kw):
    with spline_sampler():
        return test_subset2_cpu.subset_refine2_reference(frame_0, coeff_1, node_u0, node_v0, r, s, R, **kw)


def all_orders_spline(frame_0, coeff_1, node_u0, node_v0, r, s, R, **kw):
    with spline_sampler():
        return test_subset_cpu.all_orders(frame_0, coeff_1, node_u0, node_v0, r, s, R, **kw)


def all_orders2_spline(frame_0, coeff_1, node_u0, node_v0, r, s, R, **kw):
    with spline_sampler():
        return test_subset2_cpu.all_orders2(frame_0, coeff_1, node_u0, node_v0, r, s, R, **kw)


def test_the_sampler_is_put_back():
    before = [m.cubic_sample for m in RESTATEMENTS]
    with pytest.raises(RuntimeError):
        with spline_sampler():
            assert all(m.cubic_sample is bspline_sample for m in RESTATEMENTS)
            raise RuntimeError("leaves through the finally")
    assert [m.cubic_sample for m in RESTATEMENTS] == before and before[0] is test_subset_cpu.cubic_sample


# ---- the prefilter ------------------------------------------------------------------------------------------------------------------
def reflect_scalar(i, n):
    if n == 1:
        return 0
    p = 2 * (n - 1)
    m = i % p  # (Python's % of a positive p is non-negative)
    return m if m <= n - 1 else p - m


def line_brute(s):
    out = []
    for k in range(len(s)):
        acc = F64(0.0)
        for j in range(HORIZON, 0, -1):
            acc = acc + ZJ[j] * (s[reflect_scalar(k - j, len(s))] + s[reflect_scalar(k + j, len(s))])
        acc = acc + s[k]
        out.append(G * acc)
    return out


def prefilter_brute(plane):
    """The definition, one scalar operation at a time."""
    a = np.asarray(plane, F32).astype(F64)
    rows = np.array([line_brute(list(line)) for line in a], F64)
    return np.array([line_brute(list(column)) for column in rows.T], F64).T.astype(F32)


def test_reflect():
    assert reflect(np.arange(-7, 9), 1).tolist() == [0] * 16
    assert reflect(np.arange(-6, 9), 4).tolist() == [0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]
    assert reflect(np.arange(-3, 6), 2).tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert all(int(reflect(i, n)) == reflect_scalar(i, n) for n in (1, 2, 3, 5, 19) for i in range(-40, 60))


def test_constants():
    assert float(G) == 0.28867513459481287 and abs(float(ZJ[16])) < 7.1e-10 and abs(float(ZJ[16])) > 6.9e-10 and len(ZJ) == 17


def test_a_constant_plane_gives_a_thirty_sixth():
    for c in (1.0, 255.0, -3.5):
        for shape in ((23, 19), (3, 5), (1, 7)):
            got = bspline_prefilter_reference(np.full(shape, c, F32)).astype(F64)
            assert np.abs(got / (c / 36.0) - 1.0).max() <= 1e-6, (c, shape)


def test_prefilter_then_sampling_at_the_pixels_gives_the_plane_back():
    """Random 19 x 23 in 0 .. 255: within 4e-5 (an fp32 ulp of a coefficient of that size is 4.8e-7, and thirty-six go into a sample)."""
    plane = np.random.default_rng(7).uniform(0, 255, (23, 19)).astype(F32)
    coeff = bspline_prefilter_reference(plane).astype(F64)
    ys, xs = np.mgrid[0:23, 0:19].astype(F64)
    error = np.abs(bspline_sample(coeff, xs, ys) - plane.astype(F64)).max()
    print("largest error at the pixels %.3e" % error)
    assert error <= 4e-5


@pytest.mark.parametrize("w,h", [(5, 3), (1, 7), (7, 1)])
def test_small_planes_reflect_more_than_once(w, h):
    plane = np.random.default_rng(w * 10 + h).uniform(-100, 100, (h, w)).astype(F32)
    got = bspline_prefilter_reference(plane)
    assert np.isfinite(got).all() and np.array_equal(bits(got), bits(prefilter_brute(plane)))


def test_a_nan_reaches_its_footprint_only():
    plane = np.random.default_rng(3).uniform(0, 255, (40, 45)).astype(F32)
    plane[20, 22] = np.nan
    got = bspline_prefilter_reference(plane)
    bad = ~np.isfinite(got)
    want = np.zeros_like(bad)
    want[20 - 16:20 + 17, 22 - 16:22 + 17] = True
    assert np.array_equal(bad, want)


# ---- accuracy -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def spline_scene_rows(name, d):
    """One row of the first table: test_subset_cpu.scene_figures with the spline refinement in all three orders."""
    kept = {}

    def refine(f0, f1, u0, v0, r, s, R):
        got, kept["spread"] = all_orders_spline(f0, bspline_prefilter_reference(f1), u0, v0, r, s, R)
        return got

    row = test_subset_cpu.scene_figures(name, d, refine)
    row["spread"] = kept["spread"]
    return row


@functools.lru_cache(maxsize=None)
def spline_scene_rows2(name, R):
    """One row of the second table: test_subset2_cpu.scene_figures with the order-2 spline refinement in all three orders."""
    kept = {}

    def refine2(f0, f1, u0, v0, r, s, R):
        got, kept["spread"] = all_orders2_spline(f0, bspline_prefilter_reference(f1), u0, v0, r, s, R)
        return got

    row = test_subset2_cpu.scene_figures(name, R, refine2)
    row["spread"] = kept["spread"]
    return row


@pytest.mark.parametrize("name,d", SCENE_CASES)
def test_accuracy_on_the_six_scenes(name, d):
    """96 x 80, r = R = 7, s = 8, started from flow2d_correlate_2d's vectors, coefficients stored as fp32: every interior node
    converges, the mean interior endpoint error is at most a quarter of the Catmull-Rom restatement's on the same starts
    (measured: 0.07 to 0.10 of it), the mean gradient error at most 0.001 (measured: 0.0002), and the three summation orders agree
    on every state with a spread below 1e-9."""
    row, catmull = spline_scene_rows(name, d), test_subset_cpu.scene_rows(name, d)
    print(json.dumps(row), "Catmull-Rom mean EPE %.4f" % catmull["subset_mean_epe"])
    assert row["interior"] >= 12 and row["interior_converged"] == row["interior"]
    assert row["subset_mean_epe"] <= catmull["subset_mean_epe"] / 4.0
    assert row["gradient_mean_error"] <= 0.001
    assert row["spread"] < 1e-9


SPLINE_BENDING_CASES = [("bend", 7), ("bulge", 7), ("bend", 11)]


@pytest.mark.parametrize("name,R", SPLINE_BENDING_CASES)
def test_accuracy_on_the_bending_scenes_at_order_2(name, R):
    """Every scored node converges and the mean endpoint error is at most a third of order 2 with the Catmull-Rom sample
    (measured: 0.10 to 0.15 of it); the three summation orders agree on every state, spread below 1e-9."""
    row, catmull = spline_scene_rows2(name, R), test_subset2_cpu.scene_rows(name, R)
    print(json.dumps(row), "Catmull-Rom order-2 mean EPE %.4f" % catmull["order2_mean_epe"])
    assert row["order2_converged"] == row["nodes"]
    assert row["order2_mean_epe"] <= catmull["order2_mean_epe"] / 3.0
    assert row["spread"] < 1e-9


@functools.lru_cache(maxsize=None)
def spline_specimen_rows(name, refine=None):
    """The specimen's rows of the table (reported, not asserted): edge and interior nodes' mean endpoint error, Catmull-Rom and
    spline, both under the mask.  refine(scene, mask, u0, v0, spline) stands in for the restatement (the device rows)."""
    c = test_subset_masked_cpu.SPECIMEN
    scene, mask, u0, v0 = test_subset_masked_cpu.specimen_case(name)
    rows = {}
    for label in ("catmull_rom", "bspline"):
        if refine is not None:
            got = refine(scene, mask, u0, v0, label == "bspline")
        elif label == "bspline":
            got = subset_refine_spline_reference(scene.frame_0, bspline_prefilter_reference(scene.frame_1), u0, v0, None, mask, c["min_pixels"],
                                                 c["r"], c["s"], c["R"], max_shift=c["max_shift"])
        else:
            got = test_subset_masked_cpu.subset_refine_masked_reference(scene.frame_0, scene.frame_1, u0, v0, None, mask, c["min_pixels"], c["r"],
                                                                        c["s"], c["R"], max_shift=c["max_shift"])
        fig, on, edge = test_subset_masked_cpu.edge_figures(scene, mask, got)
        nh, nw = got.state.shape
        cy, cx = c["r"] + np.arange(nh) * c["s"], c["r"] + np.arange(nw) * c["s"]
        error = np.hypot(got.u.astype(F64) - scene.gt_u[np.ix_(cy, cx)], got.v.astype(F64) - scene.gt_v[np.ix_(cy, cx)])
        interior = on & ~edge & np.isfinite(error)
        rows[label] = dict(edge=fig["edge"], edge_mean_error=fig["mean_error"], edge_converged=fig["converged"], interior=int(interior.sum()),
                           interior_mean_error=float(error[interior].mean()) if interior.any() else None)
    return rows


# ---- the node loops under the substitution ------------------------------------------------------------------------------------------
def test_no_mask_and_a_zero_mask_give_the_same_bytes():
    f0, f1, u0, v0, r, s = small_case()
    coeff = bspline_prefilter_reference(f1)
    none = subset_refine_spline_reference(f0, coeff, u0, v0, None, None, -1, r, s, 3)
    zero = subset_refine_spline_reference(f0, coeff, u0, v0, None, np.zeros(f0.shape, F32), 49, r, s, 3)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(none.planes(), zero.planes())) and none.record.tobytes() == zero.record.tobytes()
    assert (none.state >= 1).sum() >= 20
    catmull = test_subset_masked_cpu.subset_refine_masked_reference(f0, f1, u0, v0, None, None, -1, r, s, 3)
    assert not np.array_equal(bits(none.u), bits(catmull.u))


def test_a_subset_at_the_frames_edge_reads_reflected_taps():
    """A start that puts subset pixels at X = 0 and X = width - 1: the taps -1 and width are read, mirrored and not clamped."""
    coeff = np.arange(12, dtype=F64).reshape(2, 6) ** 2
    x = np.array([0.0, 5.0, 0.25]), np.array([0.0, 1.0, 0.5])
    got = bspline_sample(coeff, *x)
    # at (0, 0): columns (1, 0, 1), rows (1, 0, 1) with the weights (1, 4, 1)
    assert got[0] == (1 * (coeff[1, 1] + 4 * coeff[1, 0] + coeff[1, 1]) + 4 * (coeff[0, 1] + 4 * coeff[0, 0] + coeff[0, 1])) + 1 * (coeff[1, 1] + 4 * coeff[1, 0] + coeff[1, 1])
    assert got[1] == (1 * (2 * coeff[0, 4] + 4 * coeff[0, 5]) + 4 * (2 * coeff[1, 4] + 4 * coeff[1, 5])) + 1 * (2 * coeff[0, 4] + 4 * coeff[0, 5])
    clamped = test_subset_cpu.cubic_sample(coeff, *x)
    assert np.isfinite(clamped).all()


# ---- the entries' host side ---------------------------------------------------------------------------------------------------------
def test_prefilter_refusals_without_a_device(flow2d):
    lib = flow2d.hip_lib()
    fake = ctypes.create_string_buffer(4096)
    w, h, pitch = 100, 40, 512
    span = pitch * h
    src, dst = 1 << 20, (1 << 20) + span + 4096
    d = dict(ctx=ctypes.addressof(fake), src=src, dst=dst, w=w, h=h, pitch=pitch)

    def call(**kw):
        a = dict(d, **kw)
        return lib.flow2d_bspline_prefilter_2d(a["ctx"], a["src"], a["dst"], a["w"], a["h"], a["pitch"])

    bad = [dict(ctx=None), dict(src=None), dict(dst=None), dict(w=0), dict(h=0), dict(pitch=pitch + 8), dict(pitch=256), dict(src=src + 4),
           dict(dst=dst + 8), dict(dst=src), dict(dst=src + span - pitch), dict(dst=src - span + 16), dict(src=dst + pitch)]
    for kw in bad:
        assert call(**kw) == 1, kw
    assert flow2d.BSPLINE_HORIZON == HORIZON


def test_spline_refusals_without_a_device(flow2d):
    """flow2d_subset_refine_spline_2d: what flow2d_subset_refine_masked_2d refuses, with and without a mask, and a coeff_1 that meets
    a written range."""
    lib = flow2d.hip_lib()
    fake = ctypes.create_string_buffer(4096)
    w, h, pitch, npitch = 100, 40, 512, 64
    span = pitch * h
    at = lambda k: (1 << 20) + k * (span + 4096)  # noqa: E731  (addresses only: nothing is dereferenced before the device is entered)
    d = dict(ctx=ctypes.addressof(fake), f0=at(0), c1=at(1), w=w, h=h, pitch=pitch, u0=at(2), v0=at(3), ux0=at(13), uy0=at(14), vx0=at(15),
             vy0=at(16), nw=11, nh=4, npitch=npitch, r=7, s=8, R=7, K=20, eps=1e-3, shift=4.0, grad=0.5, mask=at(17), min_pixels=57, u=at(4),
             v=at(5), ux=at(6), uy=at(7), vx=at(8), vy=at(9), score=at(10), state=at(11), record=at(12))

    def call(**kw):
        a = dict(d, **kw)
        return lib.flow2d_subset_refine_spline_2d(a["ctx"], a["f0"], a["c1"], a["w"], a["h"], a["pitch"], a["u0"], a["v0"], a["ux0"], a["uy0"],
                                                  a["vx0"], a["vy0"], a["nw"], a["nh"], a["npitch"], a["r"], a["s"], a["R"], a["K"], a["eps"],
                                                  a["shift"], a["grad"], a["mask"], a["min_pixels"], a["u"], a["v"], a["ux"], a["uy"], a["vx"],
                                                  a["vy"], a["score"], a["state"], a["record"])

    nan, inf = float("nan"), float("inf")
    bad = [dict(ctx=None), dict(f0=None), dict(c1=None), dict(u0=None), dict(v=None), dict(w=0), dict(nh=0), dict(pitch=pitch + 8),
           dict(npitch=32), dict(r=0), dict(s=65), dict(R=0), dict(R=16), dict(K=65), dict(eps=nan), dict(shift=0.0), dict(shift=inf),
           dict(grad=nan), dict(nw=12), dict(ux=None), dict(record=at(12) + 4), dict(u=at(0)), dict(uy=at(6)), dict(ux0=None),
           dict(uy0=None, vx0=None, vy0=None), dict(vx0=at(15) + 4), dict(u=at(13)), dict(record=at(15) + 64),
           dict(min_pixels=5), dict(min_pixels=226), dict(mask=at(17) + 4), dict(u=at(17)), dict(record=at(17) + 64),
           # coeff_1: a plane like the frames, met by no written range
           dict(c1=at(1) + 4), dict(u=at(1)), dict(vy=at(1) + span - pitch), dict(score=at(1) + pitch), dict(state=at(1)), dict(record=at(1) + 64)]
    # ... and without a mask the same, min_pixels not looked at
    bad += [dict(mask=None, min_pixels=0, **kw) for kw in (dict(c1=None), dict(ux0=None), dict(h=14), dict(vy=None), dict(u=at(1)), dict(R=16),
                                                           dict(state=at(1) + pitch), dict(c1=at(1) + 8))]
    for kw in bad:
        assert call(**kw) == 1, kw


def test_spline2_refusals_without_a_device(flow2d):
    lib = flow2d.hip_lib()
    fake = ctypes.create_string_buffer(4096)
    w, h, pitch, npitch = 100, 40, 512, 64
    span = pitch * h
    at = lambda k: (1 << 20) + k * (span + 4096)  # noqa: E731
    nan = float("nan")
    d = dict(ctx=ctypes.addressof(fake), f0=at(0), c1=at(1), w=w, h=h, pitch=pitch, u0=at(2), v0=at(3), sg=None, sc=None, nw=11, nh=4,
             npitch=npitch, r=7, s=8, R=7, K=20, eps=1e-3, shift=2.0, grad=0.5, curv=0.05, u=at(4), v=at(5),
             g=[at(6), at(7), at(8), at(9)], c=[at(10), at(11), at(12), at(13), at(14), at(15)], score=at(16), state=at(17), record=at(18))
    sg, sc = [at(20 + k) for k in range(4)], [at(24 + k) for k in range(6)]

    def group(planes):
        return None if planes is None else (ctypes.c_void_p * len(planes))(*planes)

    def call(**kw):
        a = dict(d, **kw)
        return lib.flow2d_subset_refine2_spline_2d(a["ctx"], a["f0"], a["c1"], a["w"], a["h"], a["pitch"], a["u0"], a["v0"], group(a["sg"]),
                                                   group(a["sc"]), a["nw"], a["nh"], a["npitch"], a["r"], a["s"], a["R"], a["K"], a["eps"],
                                                   a["shift"], a["grad"], a["curv"], a["u"], a["v"], group(a["g"]), group(a["c"]), a["score"],
                                                   a["state"], a["record"])

    bad = [dict(ctx=None), dict(f0=None), dict(c1=None), dict(u0=None), dict(v=None), dict(w=0), dict(pitch=pitch + 8), dict(R=1), dict(R=16),
           dict(K=0), dict(eps=nan), dict(curv=0.0), dict(nw=12), dict(record=at(18) + 4), dict(g=[None] + d["g"][1:]), dict(sc=sc),
           dict(sg=sg[:1] + [None] + sg[2:]), dict(c1=at(1) + 4), dict(u=at(1)), dict(c=d["c"][:3] + [at(1) + span - pitch] + d["c"][4:]),
           dict(state=at(1) + pitch), dict(record=at(1)), dict(sg=sg, u=sg[0])]
    for kw in bad:
        assert call(**kw) == 1, kw


def test_the_interpolation_travels_beside_the_options_record(flow2d):
    """flow2d_host_subset_options stays 40 bytes with its nine fields; the interpolation is the object's, set by
    flow2d_host_set_subset_interpolation, which refuses an unknown kind and a null object."""
    assert ctypes.sizeof(flow2d.SubsetOptions) == 40 and len(flow2d.SubsetOptions._fields_) == 9
    host = flow2d.host_lib()
    assert [host.flow2d_host_set_subset_interpolation(None, kind) for kind in (0, 1, 2)] == [1, 1, 1]  # (no object)
    # the setter's own test of the kind, which needs no object: 0 and 1 are the two samplers, 2 is refused
    assert [host.flow2d_host_subset_interpolation_ok(kind) for kind in (-1, 0, 1, 2, 3)] == [0, 1, 1, 0, 0]
    assert (flow2d.SUBSET_CATMULL_ROM, flow2d.SUBSET_BSPLINE) == (0, 1)
    assert flow2d.SUBSET_INTERPOLATIONS == {"catmull-rom": 0, "bspline": 1}
    flow = flow2d.OpticalFlow.__new__(flow2d.OpticalFlow)  # (no object of the host layer: the call does not get as far as one)
    with pytest.raises(ValueError):
        flow.refine_nodes_device(None, None, None, None, 7, 8, 7, interpolation="quintic")
    # (the setter on a real object, kind 2 included, is in tests/test_gpu_subset_spline_host.py)
