"""The pyramid started from a prior flow, as far as it can be checked without a device: the start-level rule against a table written
out here, the refusals of flow2d_prior_registration_2d, and a restatement of OpticalFlow2D::ComputeFlowFromPrior from the oracle's
stages (tests/test_gpu_prior.py holds the GPU to its bytes) with the accuracy it reaches on the speckle scenes when the prior is
the window correlation's node field."""
import ctypes
import importlib

import numpy as np
import pytest

from test_correlate_cpu import correlate_reference, expand_reference, frame_range, scenes_module

F32 = np.float32
U32 = np.uint32
GREY, GRADIENT, GRADIENT_UNTILED = 0, 1, 2
CLI_DEFAULTS = (50, 0.9, 40, 5, 35.0, 0.001, 0.001, 5, 1.5)  # levels, scale, outer, inner, alpha, e_smooth, e_data, median, sigma


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def sanitise(prior_u, prior_v):
    """The prior as flow2d_prior_registration_2d takes it: (0, 0) where either component is not finite; and the count of those."""
    pu, pv = np.ascontiguousarray(prior_u, F32), np.ascontiguousarray(prior_v, F32)
    bad = ~(np.isfinite(pu) & np.isfinite(pv))
    return np.where(bad, F32(0), pu), np.where(bad, F32(0), pv), int(bad.sum())


def start_level(width, height, levels, scale, reach, level=None):
    """OpticalFlow2D::PriorStartLevel in numpy float32 (np.power on float32 is the level geometry's pow)."""
    from oracle import np_restatement as NP
    top = min(levels, NP.max_warp_level(width, height, scale)) - 1
    if level is None:
        level = 0
        while level < top and not F32(reach) * F32(np.power(F32(scale), F32(level))) <= F32(1):
            level += 1
    return min(level, top)


def compute_flow_from_prior(O, frame_0, frame_1, prior_u, prior_v, levels, scale, outer, inner, alpha, e_smooth, e_data, median_radius,
                            sigma, constancy, start):
    """OpticalFlow2D::ComputeFlowFromPrior from the oracle's stages: the level loop of oracle.compute_flow from level `start` down,
    its first level's base flow the sanitised prior resampled from full resolution (no magnitude scaling).  Every plane keeps the
    container's size and the stages get the level's w, h.  Returns (u, v, count of non-finite prior pixels)."""
    f0, f1 = np.ascontiguousarray(frame_0, F32), np.ascontiguousarray(frame_1, F32)
    H, W = f0.shape
    pu, pv, count = sanitise(prior_u, prior_v)
    if sigma > 0:
        f0, f1 = O.convolution(f0, W, H, sigma), O.convolution(f1, W, H, sigma)
    u, v, pw, ph = pu, pv, W, H
    for level in range(start, -1, -1):
        cw, ch, hx, hy = O.level_geometry(W, H, scale, level)
        g0, g1 = (f0, f1) if level == 0 else (O.resample(f0, W, H, cw, ch), O.resample(f1, W, H, cw, ch))
        u, v = O.resample(u, pw, ph, cw, ch), O.resample(v, pw, ph, cw, ch)
        warped = O.registration(g0, g1, u, v, cw, ch, hx, hy)
        du, dv, _, _ = O.solve_level(g0, warped, u, v, cw, ch, hx, hy, alpha, e_smooth, e_data, outer, inner, constancy)
        u, v = O.add(u, du, cw, ch), O.add(v, dv, cw, ch)
        if median_radius != 1:
            window = median_radius - 1 if median_radius % 2 == 0 else median_radius
            u, v = O.median(u, cw, ch, window), O.median(v, cw, ch, window)
        pw, ph = cw, ch
    return u, v, count


def correlation_prior(frame_0, frame_1, r, d, s):
    """The prior of OpticalFlow2D::ComputeFlowCorrelationSeeded: the node field on the frame's grid, NaN where no node is valid."""
    lo, scale = frame_range(frame_0, frame_1)
    nu, nv, score, record, _ = correlate_reference(frame_0, frame_1, lo, scale, r, d, s)
    h, w = frame_0.shape
    return expand_reference(nu, nv, r, s, w, h) + ((nu, nv, score, record, (lo, scale)),)


def interior_epe(u, v, scene, margin):
    err = np.hypot(u - scene.gt_u, v - scene.gt_v)[margin:scene.gt_u.shape[0] - margin, margin:scene.gt_u.shape[1] - margin]
    return float(err.mean())


# ---- the start level -----------------------------------------------------------------------------------------------------------------
def test_start_level_table(flow2d):
    """reach * scale^l <= 1 for the first time: 0.9^6 = 0.531 and 0.9^7 = 0.478, 0.9^13 = 0.254 and 0.9^14 = 0.229; 0.5^l exact."""
    table = {(0.9, 1.0): 0, (0.9, 2.0): 7, (0.9, 4.0): 14, (0.5, 2.0): 1, (0.5, 4.0): 2, (0.5, 5.0): 3}
    for (scale, reach), want in table.items():
        assert flow2d.prior_start_level(4096, 4096, 50, scale, reach) == want, (scale, reach)
        assert start_level(4096, 4096, 50, scale, reach) == want, (scale, reach)
    assert flow2d.prior_start_level(4096, 4096, 50, 0.9) == 7  # the default reach is 2
    assert flow2d.prior_start_level(4096, 4096, 50, 0.9, 0.25) == 0  # a prior trusted to a quarter pixel enters at full resolution


def test_start_level_is_clamped_to_the_unseeded_top_level(flow2d):
    # few levels asked for
    assert flow2d.prior_start_level(4096, 4096, 5, 0.9, 4.0) == 4
    assert flow2d.prior_start_level(4096, 4096, 1, 0.5, 4.0) == 0
    # the frame allows fewer: 20 x 16 at 0.5 has levels 20 x 16, 10 x 8, 5 x 4
    top = flow2d.max_warp_level(20, 16, 0.5) - 1
    assert top == 2
    assert flow2d.prior_start_level(20, 16, 50, 0.5, 64.0) == top
    assert flow2d.prior_start_level(20, 16, 50, 0.5, 2.0) == 1
    for w, h, levels, scale, reach in ((96, 80, 50, 0.9, 2.0), (96, 80, 50, 0.9, 1000.0), (97, 61, 6, 0.7, 3.0), (33, 21, 50, 0.5, 4.0)):
        assert flow2d.prior_start_level(w, h, levels, scale, reach) == start_level(w, h, levels, scale, reach)


def test_prior_level_overrides_the_rule(flow2d):
    assert flow2d.prior_start_level(4096, 4096, 50, 0.9, 2.0, level=3) == 3
    assert flow2d.prior_start_level(4096, 4096, 50, 0.9, 2.0, level=0) == 0
    assert flow2d.prior_start_level(4096, 4096, 50, 0.9, 1000.0, level=11) == 11  # (the reach is not consulted)
    assert flow2d.prior_start_level(20, 16, 50, 0.5, 2.0, level=9) == 2  # clamped like the rule
    assert flow2d.prior_start_level(4096, 4096, 4, 0.5, 2.0, level=9) == 3


def test_start_level_refusals(flow2d):
    nan, inf = float("nan"), float("inf")
    for reach in (0.0, -1.0, nan, inf, -inf):
        with pytest.raises(ValueError):
            flow2d.prior_start_level(96, 80, 50, 0.9, reach)
    with pytest.raises(ValueError):
        flow2d.prior_start_level(96, 80, 50, 0.9, 2.0, level=-1)
    with pytest.raises(ValueError):
        flow2d.prior_start_level(96, 80, 0, 0.9, 2.0)  # no level to run
    with pytest.raises(ValueError):
        flow2d.prior_start_level(96, 80, 50, 1.0, 2.0)  # not a pyramid
    raw = flow2d.host_lib().flow2d_host_prior_start_level
    out = ctypes.c_size_t(77)
    assert raw(96, 80, 50, 0.9, 2.0, -2, ctypes.byref(out)) == 1 and out.value == 77  # below "not given": refused, nothing written
    assert raw(96, 80, 50, 0.9, 2.0, -1, None) == 1


# ---- the entry's refusals ----------------------------------------------------------------------------------------------------------
def test_entry_refusals_without_a_device(flow2d):
    """One case at least per refusal of flow2d_prior_registration_2d, each before any launch: the addresses are made up and nothing
    is dereferenced before the device is entered (only refusals here: an accepted call would launch on them)."""
    lib = flow2d.hip_lib()
    fake = ctypes.create_string_buffer(4096)
    in_w, in_h, w, h, pitch = 96, 80, 48, 40, 512
    span = pitch * in_h
    at = lambda k: (1 << 20) + k * (span + 4096)  # noqa: E731
    nan, inf = float("nan"), float("inf")
    d = dict(ctx=ctypes.addressof(fake), pu=at(0), pv=at(1), in_w=in_w, in_h=in_h, ou=at(2), ov=at(3), f0=at(4), f1=at(5), w=w, h=h,
             pitch=pitch, hx=2.0, hy=2.0, out=at(6), record=at(7))

    def call(**kw):
        a = dict(d, **kw)
        return lib.flow2d_prior_registration_2d(a["ctx"], a["pu"], a["pv"], a["in_w"], a["in_h"], a["ou"], a["ov"], a["f0"], a["f1"],
                                                a["w"], a["h"], a["pitch"], a["hx"], a["hy"], a["out"], a["record"])

    level_span = pitch * h
    refusals = {
        "a null plane or record": [dict(ctx=None), dict(pu=None), dict(pv=None), dict(ou=None), dict(ov=None), dict(f0=None),
                                   dict(f1=None), dict(out=None), dict(record=None), dict(record=at(7) + 4)],
        "a zero size": [dict(w=0), dict(h=0), dict(in_w=0), dict(in_h=0)],
        "a level larger than the prior": [dict(w=in_w + 1), dict(h=in_h + 1), dict(w=100, in_w=96), dict(in_h=39)],
        "a bad pitch": [dict(pitch=pitch + 8), dict(pitch=4 * in_w - 16), dict(pitch=100), dict(pu=at(0) + 4), dict(out=at(6) + 8)],
        "hx / hy": [dict(hx=0.0), dict(hx=-1.0), dict(hx=nan), dict(hx=inf), dict(hy=0.0), dict(hy=-2.0), dict(hy=nan), dict(hy=inf)],
        "overlapping ranges": [dict(ou=at(0)), dict(ov=at(1) + span - pitch), dict(out=at(4)), dict(out=at(5) + level_span - 16),
                               dict(ou=at(3)), dict(ov=at(6) + pitch), dict(out=at(2) + level_span - pitch), dict(record=at(0) + 64),
                               dict(record=at(5) + 8), dict(record=at(2) + 16), dict(record=at(6) + level_span - 8)],
    }
    for why, cases in refusals.items():
        for kw in cases:
            assert call(**kw) == 1, (why, kw)
    assert lib.flow2d_abi_version() == 1  # the entry was added under the same version


# ---- the restatement's accuracy ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def speckle():
    """scene, expanded node field and margin per motion: computed once."""
    cache = {}

    def get(motion):
        if motion not in cache:
            r, s, d = 7, 8, (12 if motion == "large_translation" else 6)
            scene = scenes_module().make_speckle_scene(motion, 96, 80, seed=0)
            pu, pv, _ = correlation_prior(scene.frame_0, scene.frame_1, r, d, s)
            cache[motion] = (scene, pu, pv, r + d)
        return cache[motion]
    return get


@pytest.mark.parametrize("constancy", [GREY, GRADIENT], ids=["grey", "gradient"])
@pytest.mark.parametrize("motion", ["translation", "affine", "large_translation"])
def test_seeded_flow_beats_both_methods_on_speckle(oracle, speckle, motion, constancy):
    """96 x 80, seed 0, radius 7, spacing 8, range 6 (12 for the large translation), the CLI's defaults, reach 2: the mean endpoint
    error over the pixels at least r + d from the border is at most the expanded node field's and at most the unseeded flow's; for
    the large translation at most 0.5 px while the unseeded flow is above 10 px."""
    scene, pu, pv, margin = speckle(motion)
    levels, scale = CLI_DEFAULTS[:2]
    start = start_level(96, 80, levels, scale, 2.0)
    assert start == 7
    u, v, count = compute_flow_from_prior(oracle, scene.frame_0, scene.frame_1, pu, pv, *CLI_DEFAULTS, constancy, start)
    plain_u, plain_v, _ = oracle.compute_flow(scene.frame_0, scene.frame_1, *CLI_DEFAULTS, constancy)
    su, sv, counted = sanitise(pu, pv)
    seeded, nodes, unseeded = interior_epe(u, v, scene, margin), interior_epe(su, sv, scene, margin), interior_epe(plain_u, plain_v, scene, margin)
    print("%s constancy %d: unseeded %.3f  expanded nodes %.3f  from prior %.3f  (%d prior pixels not finite)" %
          (motion, constancy, unseeded, nodes, seeded, count))
    assert count == counted
    assert seeded <= nodes
    assert seeded <= unseeded
    if motion == "large_translation":
        assert seeded <= 0.5 and unseeded > 10.0


def test_zero_prior_at_the_top_level_is_the_unseeded_flow(oracle):
    """The restatement itself: from an all-zero prior at the unseeded top level it is oracle.compute_flow, bit for bit (the zero
    prior resamples to the zeros the unseeded pyramid starts from)."""
    f0, f1 = oracle.synthetic_pair(96, 80, 1.5, -0.75, seed=2, noise=True)
    zero = np.zeros_like(f0)
    for scale, constancy in ((0.9, GREY), (0.5, GRADIENT)):
        top = min(50, oracle.max_warp_level(96, 80, scale)) - 1
        assert start_level(96, 80, 50, scale, 2.0, level=top) == top
        u, v, count = compute_flow_from_prior(oracle, f0, f1, zero, zero, 50, scale, 3, 5, 35.0, 0.001, 0.001, 5, 1.5, constancy, top)
        ou, ov, _ = oracle.compute_flow(f0, f1, 50, scale, 3, 5, 35.0, 0.001, 0.001, 5, 1.5, constancy)
        assert count == 0
        assert np.array_equal(bits(u), bits(ou)) and np.array_equal(bits(v), bits(ov)), (scale, constancy)
