"""flow2d_subset_refine_masked_2d restated in numpy from the text of include/flow2d_c_abi.h: the node of
tests/test_subset_sequence_cpu.py's refinement with the header's list of usable pixels in place of the subset, the four state
tests in the header's order, and the three summation orders of tests/test_subset_cpu.py applied to the compacted list (the
device's is "butterfly": lane l adds elements l, l + 64, ... of the list).  What can be checked without a device: that no mask and
a mask that excludes nothing give the bytes of flow2d_subset_refine_from_2d's restatement, the mask's values and the stencil
rule, the state rules around min_pixels, the accuracy on the specimen scenes -- the table of profiles/subset_mask/README.md,
which tools/subset_mask_table.py prints from specimen_rows() below --, and the entry's host-side refusals."""
import ctypes
import functools
import json

import numpy as np
import pytest

from test_correlate_cpu import F32, U32, NAN_BITS, bits, frame_range, scenes_module
from test_multipass_cpu import multipass_reference
from test_subset_cpu import (F64, FLAT, NO_INPUT, ORDERS, STRAYED, SUBSET_DTYPE, SUMS, Refined, cholesky, cubic_sample, small_case, solve,
                             subset_refine_reference)
from test_subset_sequence_cpu import PLANES, predict_passes, same_planes, subset_refine_from_reference

MASKED = -4
MIN_PIXELS = 6
# the scene the restatement is scored on, looked up here: where the scene does not exist nothing of this file loads
make_speckle_specimen = scenes_module().make_speckle_specimen


def default_min_pixels(R):
    """OpticalFlow2D::SubsetOptions::min_pixels = 0: a quarter of the subset, rounded up, six at least."""
    return max(MIN_PIXELS, ((2 * R + 1) ** 2 + 3) // 4)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def excluded_plane(mask):
    """*Excluded* of the header: !(m < 0.5) on the float, so a NaN is excluded."""
    with np.errstate(invalid="ignore"):
        return ~(np.asarray(mask, F32) < F32(0.5))


def usable_plane(mask, stencil=True):
    """*Usable* of the header: the pixel and the four its fx and fy read, each clamped to the frame, are not excluded.
    stencil=False: the pixel alone (not the header's rule; the table's third row)."""
    ex = excluded_plane(mask)
    if not stencil:
        return ~ex
    h, w = ex.shape
    ys, xs = np.mgrid[0:h, 0:w]
    return ~(ex | ex[ys, np.minimum(xs + 1, w - 1)] | ex[ys, np.maximum(xs - 1, 0)] | ex[np.minimum(ys + 1, h - 1), xs] |
             ex[np.maximum(ys - 1, 0), xs])


def refine_node_masked(f0, f1, usable, cx, cy, start, R, K, epsilon, max_shift, max_gradient, min_pixels, total):
    """(state, p, c, iterations begun) of one node whose centre is not excluded and whose start is finite: the text from "Frame-0
    window" on, every sum over the list of usable pixels."""
    h, w = f0.shape
    side = 2 * R + 1
    p = np.array(start, F64)
    u0, v0 = p[0], p[3]
    if not (cx - R >= 0 and cy - R >= 0 and cx + R <= w - 1 and cy + R <= h - 1):
        return STRAYED, p, F64(0), 0
    k = np.arange(side * side)
    k = k[usable[cy + k // side - R, cx + k % side - R]]  # the list, in ascending k
    if not k.size >= min_pixels:
        return MASKED, p, F64(0), 0
    n = F64(k.size)
    kx, ky = k % side - R, k // side - R
    xi, eta = kx.astype(F64), ky.astype(F64)
    xs, ys = cx + kx, cy + ky
    f = f0[ys, xs]
    fx = (f0[ys, np.minimum(xs + 1, w - 1)] - f0[ys, np.maximum(xs - 1, 0)]) * 0.5
    fy = (f0[np.minimum(ys + 1, h - 1), xs] - f0[np.maximum(ys - 1, 0), xs]) * 0.5
    fd = f - total(f) / n
    df2 = total(fd * fd)
    if not df2 > 0:
        return FLAT, p, F64(0), 0
    df = np.sqrt(df2)
    J = np.stack([fx, fx * xi, fx * eta, fy, fy * xi, fy * eta], axis=1)
    L = cholesky(total(J[:, :, None] * J[:, None, :]))
    if L is None:
        return FLAT, p, F64(0), 0
    c = F64(0)
    radius = F64(R)
    for it in range(1, K + 1):
        u, ux, uy, v, vx, vy = p
        X = xs.astype(F64) + ((u + ux * xi) + uy * eta)
        Y = ys.astype(F64) + ((v + vx * xi) + vy * eta)
        if not ((X >= 0) & (X <= w - 1) & (Y >= 0) & (Y <= h - 1)).all():
            return STRAYED, p, c, it
        g = cubic_sample(f1, X, Y)
        gd = g - total(g) / n
        dg2 = total(gd * gd)
        if not dg2 > 0:
            return FLAT, p, c, it
        dg = np.sqrt(dg2)
        c = total(fd * gd) / (df * dg)
        res = fd - (df / dg) * gd
        x = solve(L, total(J * res[:, None]))
        du, dux, duy, dv, dvx, dvy = -x
        ma, mb, mc, md = 1.0 + dux, duy, dvx, 1.0 + dvy
        det = ma * md - mb * mc
        if not abs(det) > 1e-12:
            return STRAYED, p, c, it
        ia, ib, ic, id_ = md / det, (-mb) / det, (-mc) / det, ma / det
        tx, ty = -(ia * du + ib * dv), -(ic * du + id_ * dv)
        p11, p12, p21, p22 = 1.0 + ux, uy, vx, 1.0 + vy
        p = np.array([(p11 * tx + p12 * ty) + u, (p11 * ia + p12 * ic) - 1.0, p11 * ib + p12 * id_,
                      (p21 * tx + p22 * ty) + v, p21 * ia + p22 * ic, (p21 * ib + p22 * id_) - 1.0], F64)
        if not (abs(p[0] - u0) <= max_shift and abs(p[3] - v0) <= max_shift and abs(p[1]) <= max_gradient and
                abs(p[2]) <= max_gradient and abs(p[4]) <= max_gradient and abs(p[5]) <= max_gradient):
            return STRAYED, p, c, it
        step = np.sqrt(((((du * du + (radius * dux) * (radius * dux)) + (radius * duy) * (radius * duy)) + dv * dv) +
                        (radius * dvx) * (radius * dvx)) + (radius * dvy) * (radius * dvy))
        if step < epsilon:
            return it, p, c, it
    return 0, p, c, K


def subset_refine_masked_reference(frame_0, frame_1, node_u0, node_v0, start_gradients, mask, min_pixels, r, s, R, K=20, epsilon=1e-3,
                                   max_shift=4.0, max_gradient=0.5, order="butterfly", stencil=True):
    """flow2d_subset_refine_masked_2d as a Refined whose record's eighth word holds the masked nodes; start_gradients = (ux0, uy0,
    vx0, vy0) or None; mask None: flow2d_subset_refine_from_2d (min_pixels is not looked at)."""
    if mask is None:
        return subset_refine_from_reference(frame_0, frame_1, node_u0, node_v0, start_gradients, r, s, R, K, epsilon, max_shift, max_gradient,
                                            order)
    assert MIN_PIXELS <= min_pixels <= (2 * R + 1) ** 2
    f0, f1 = np.asarray(frame_0, F32).astype(F64), np.asarray(frame_1, F32).astype(F64)
    excluded, usable = excluded_plane(mask), usable_plane(mask, stencil)
    assert excluded.shape == f0.shape
    if start_gradients is None:
        start_gradients = [np.zeros(np.shape(node_u0), F32)] * 4
    start = np.stack([np.asarray(q, F32) for q in (node_u0, start_gradients[0], start_gradients[1], node_v0, start_gradients[2],
                                                  start_gradients[3])], axis=-1)
    nh, nw = start.shape[:2]
    epsilon, max_shift, max_gradient = (F64(F32(x)) for x in (epsilon, max_shift, max_gradient))
    out = Refined()
    planes = np.zeros((8, nh, nw), F32)
    words = np.zeros((6, nh, nw), U32)
    out.p64 = np.full((nh, nw, 6), np.nan)
    record = np.zeros(1, SUBSET_DTYPE)
    record["nodes"] = nh * nw
    to_planes = [0, 3, 1, 2, 4, 5]
    with np.errstate(all="ignore"):
        for j in range(nh):
            for i in range(nw):
                cx, cy = r + i * s, r + j * s
                p0 = start[j, i]
                if excluded[cy, cx]:  # 1: before *no input*
                    state = MASKED
                elif not np.isfinite(p0).all():
                    words[:, j, i] = NAN_BITS
                    planes[7, j, i] = NO_INPUT
                    record["no_input"] += 1
                    continue
                else:
                    state, p, c, begun = refine_node_masked(f0, f1, usable, cx, cy, p0.astype(F64), R, K, epsilon, max_shift, max_gradient,
                                                            min_pixels, SUMS[order])
                planes[7, j, i] = state
                if state == MASKED:
                    words[:, j, i] = NAN_BITS
                    record["reserved"] += 1
                    continue
                record["iterations"] += begun
                if state >= 0:
                    words[:, j, i] = bits(p[to_planes].astype(F32))
                    planes[6, j, i] = F32(c)
                    out.p64[j, i] = p
                    record["converged" if state >= 1 else "unconverged"] += 1
                else:  # flat, strayed: the whole start, bit for bit
                    words[:, j, i] = bits(p0[to_planes])
                    record["flat" if state == FLAT else "strayed"] += 1
    nan = np.isnan(words.view(F32))
    words[nan] = NAN_BITS
    planes[:6] = words.view(F32)
    for name, plane in zip(Refined.NAMES, planes):
        setattr(out, name, plane)
    out.record = record
    return out


def all_orders_masked(*args, **kw):
    """(the butterfly order's result, the largest spread of p between the three orders); the orders must agree on every state."""
    runs = [subset_refine_masked_reference(*args, order=o, **kw) for o in ORDERS]
    for other in runs[:2]:
        assert np.array_equal(other.state, runs[2].state) and other.record.tobytes() == runs[2].record.tobytes()
    stack = np.stack([q.p64 for q in runs])
    live = np.isfinite(stack[2])
    spread = float((stack.max(0) - stack.min(0))[live].max()) if live.any() else 0.0
    return runs[2], spread


def usable_counts(mask, nw, nh, r, s, R):
    """Nv of every node of the grid whose subset lies inside the frame (else -1)."""
    usable = usable_plane(mask)
    h, w = usable.shape
    out = np.full((nh, nw), -1)
    for j in range(nh):
        for i in range(nw):
            cx, cy = r + i * s, r + j * s
            if cx - R >= 0 and cy - R >= 0 and cx + R <= w - 1 and cy + R <= h - 1:
                out[j, i] = usable[cy - R:cy + R + 1, cx - R:cx + R + 1].sum()
    return out


def random_mask(shape, fraction=0.3, seed=5):
    return (np.random.default_rng(seed).random(shape) < fraction).astype(F32)


# ---- equivalences -------------------------------------------------------------------------------------------------------------------
def started_case():
    """tests/test_subset_cpu.py's small case with a start from a previous step and nodes of every state."""
    f0, f1, u0, v0, r, s = small_case()
    first = subset_refine_reference(f0, f1, u0, v0, r, s, 3)
    start = [q.copy() for q in predict_passes([getattr(first, n) for n in PLANES], first.state, s)[0]]
    start[0][2, 2], start[4][3, 3], start[0][4, 4], start[2][1, 1] = np.nan, np.inf, 1e30, 2.0
    f0 = f0.copy()
    f0[8, 38] = np.nan  # flat nodes
    return f0, f1, start, r, s


@pytest.mark.parametrize("order", ORDERS)
def test_no_mask_and_a_mask_that_excludes_nothing_are_the_plain_refinement(order):
    f0, f1, start, r, s = started_case()
    for R in (3, 6):  # R = 6: the border nodes' subsets leave frame 0
        for grads in (start[2:], None):
            want = subset_refine_from_reference(f0, f1, start[0], start[1], grads, r, s, R, order=order)
            assert {NO_INPUT, FLAT, STRAYED} <= set(np.unique(want.state)) and (want.state >= 1).any()
            none = subset_refine_masked_reference(f0, f1, start[0], start[1], grads, None, -5, r, s, R, order=order)
            zero = subset_refine_masked_reference(f0, f1, start[0], start[1], grads, np.zeros(f0.shape, F32), (2 * R + 1) ** 2, r, s, R, order=order)
            for got in (none, zero):
                assert same_planes(got, want) and got.record.tobytes() == want.record.tobytes()
                assert np.array_equal(got.p64[got.state >= 0], want.p64[want.state >= 0])


# ---- the mask's values, the stencil rule ------------------------------------------------------------------------------------------
def test_mask_values():
    m = np.zeros((5, 6), F32)
    m[0, 0], m[0, 1] = 0.49999997, -0.0           # included
    m[2, 2], m[4, 5], m[0, 4] = 0.5, np.nan, np.inf  # excluded
    ex = excluded_plane(m)
    assert ex.sum() == 3 and ex[2, 2] and ex[4, 5] and ex[0, 4] and not ex[0, 0] and not ex[0, 1]
    assert excluded_plane(np.full((1, 1), -np.inf, F32)).sum() == 0 and excluded_plane(np.full((1, 1), 1.0, F32)).all()
    us = usable_plane(m)
    want = np.ones((5, 6), bool)
    for y, x in ((2, 2), (1, 2), (3, 2), (2, 1), (2, 3), (4, 5), (3, 5), (4, 4), (0, 4), (1, 4), (0, 3), (0, 5)):
        want[y, x] = False
    assert np.array_equal(us, want)
    # at a frame border the clamped neighbour is the pixel itself: a corner pixel with clean neighbours inside the frame is usable
    assert us[0, 0] and us[4, 0] and us[0, 1]
    assert np.array_equal(usable_plane(m, stencil=False), ~ex)


def test_a_masked_pixel_changes_only_the_nodes_whose_subset_holds_its_stencil():
    f0, f1, u0, v0, r, s = small_case()
    base = subset_refine_from_reference(f0, f1, u0, v0, None, r, s, 3)
    mask = np.zeros(f0.shape, F32)
    mask[16, 21] = np.nan  # in the subsets of four nodes, the centre of none
    got, spread = all_orders_masked(f0, f1, u0, v0, None, mask, 10, r, s, 3)
    nv = usable_counts(mask, u0.shape[1], u0.shape[0], r, s, 3)
    hit = nv < 49
    assert 1 <= hit.sum() <= 4 and set(nv[hit]) <= {44, 45, 46, 47, 48} and spread < 1e-9
    assert all(np.array_equal(bits(a)[~hit], bits(b)[~hit]) for a, b in zip(got.planes(), base.planes()))
    assert (got.state[hit] >= 1).all() and not np.array_equal(bits(got.u)[hit], bits(base.u)[hit])
    # a NaN of frame 0 under an excluded pixel no longer makes the node flat
    g0 = f0.copy()
    g0[16, 21] = np.nan
    assert (subset_refine_from_reference(g0, f1, u0, v0, None, r, s, 3).state[hit] == FLAT).all()
    assert (subset_refine_masked_reference(g0, f1, u0, v0, None, mask, 10, r, s, 3).state[hit] >= 1).all()


# ---- the state rules ----------------------------------------------------------------------------------------------------------------
def block_mask(shape, cx, cy, rows, cols):
    """Everything excluded but a rows x cols block around (cx, cy): its usable pixels are the (rows - 2) x (cols - 2) inside it."""
    mask = np.ones(shape, F32)
    mask[cy - rows // 2:cy - rows // 2 + rows, cx - cols // 2:cx - cols // 2 + cols] = 0
    return mask


def test_nv_at_min_pixels_runs_and_one_below_is_masked():
    f0, f1, u0, v0, r, s = small_case()
    cx, cy = r + 4 * s, r + 3 * s  # node (3, 4)
    mask = block_mask(f0.shape, cx, cy, 5, 7)  # inside the 7 x 7 subset: 3 x 5 usable pixels
    nv = usable_counts(mask, u0.shape[1], u0.shape[0], r, s, 3)
    assert nv[3, 4] == 15
    at = subset_refine_masked_reference(f0, f1, u0, v0, None, mask, 15, r, s, 3)
    below = subset_refine_masked_reference(f0, f1, u0, v0, None, mask, 16, r, s, 3)
    assert at.state[3, 4] != MASKED and at.record["iterations"][0] >= 1 and below.state[3, 4] == MASKED
    assert (at.state == MASKED).sum() == u0.size - 1 and (below.state == MASKED).all()
    assert below.record.tolist() == [(u0.size, 0, 0, 0, 0, 0, 0, u0.size)]  # the eighth word; a masked node adds no iterations
    assert at.record["reserved"][0] == u0.size - 1
    assert (bits(below.u) == NAN_BITS).all() and (bits(below.vy) == NAN_BITS).all() and (below.score == 0).all()


def test_the_order_of_the_state_tests():
    f0, f1, u0, v0, r, s = small_case()
    u0, v0 = u0.copy(), v0.copy()
    mask = np.zeros(f0.shape, F32)
    mask[r + 2 * s, r + 2 * s] = 1  # the centre of node (2, 2)
    u0[2, 2] = np.nan                # ... whose start is not finite: masked, not *no input*
    u0[2, 4] = np.nan                # a clean centre: no input
    got = subset_refine_masked_reference(f0, f1, u0, v0, None, mask, 10, r, s, 6)
    assert got.state[2, 2] == MASKED and got.state[2, 4] == NO_INPUT and bits(got.u)[2, 2] == NAN_BITS
    # R = 6 > r: the border nodes stray by the frame-0 window test before their pixels are counted, whatever the mask
    assert got.state[0, 0] == STRAYED and got.record["strayed"][0] >= 15
    mask[:] = 1
    mask[r, r] = 0  # the corner node's centre alone: the window test comes before Nv
    got = subset_refine_masked_reference(f0, f1, u0, v0, None, mask, 10, r, s, 6)
    assert got.state[0, 0] == STRAYED and (got.state == MASKED).sum() == u0.size - 1
    assert int(got.record["reserved"][0]) == u0.size - 1 and int(got.record["strayed"][0]) == 1 and int(got.record["no_input"][0]) == 0


def test_the_three_orders_agree_under_a_random_mask():
    f0, f1, start, r, s = started_case()
    got, spread = all_orders_masked(f0, f1, start[0], start[1], start[2:], random_mask(f0.shape, 0.1), 6, r, s, 3)
    print("spread %.3e" % spread, got.record)
    assert spread < 1e-9 and (got.state == MASKED).sum() >= 5 and (got.state >= 1).sum() >= 5


# ---- the accuracy on the specimen scenes --------------------------------------------------------------------------------------------
SPECIMEN = dict(width=96, height=80, r=7, s=8, R=7, d=6, min_pixels=57, max_shift=2.0)


@functools.lru_cache(maxsize=None)
def specimen_case(name):
    """The scene, its mask and the chain's start: search (d = 6) and validation with replacement, restated."""
    c = SPECIMEN
    scene, mask = make_speckle_specimen(name, c["width"], c["height"], seed=0)
    lo, scale = frame_range(scene.frame_0, scene.frame_1)
    u0, v0, _, _, _ = multipass_reference(scene.frame_0, scene.frame_1, lo, scale, [(c["r"], c["d"], c["s"])], replace=True, validate_last=True)
    return scene, mask, u0, v0


def edge_figures(scene, mask, got, truth_start=None):
    """The table's figures of one refinement over the edge nodes: on the specimen, with a subset that is not all usable."""
    c = SPECIMEN
    nh, nw = got.state.shape
    cy, cx = c["r"] + np.arange(nh) * c["s"], c["r"] + np.arange(nw) * c["s"]
    on = mask[np.ix_(cy, cx)] < 0.5
    nv = usable_counts(mask, nw, nh, c["r"], c["s"], c["R"])
    edge = on & (nv < (2 * c["R"] + 1) ** 2)
    tu, tv = scene.gt_u[np.ix_(cy, cx)].astype(F64), scene.gt_v[np.ix_(cy, cx)].astype(F64)
    with np.errstate(invalid="ignore"):
        error = np.hypot(got.u.astype(F64) - tu, got.v.astype(F64) - tv)
        converged = got.state >= 1
    # (the mean and the worst are over every edge node that has a vector: an unconverged node delivers its p, a strayed one its start)
    has = edge & np.isfinite(error)
    fig = dict(on_specimen=int(on.sum()), edge=int(edge.sum()), converged=int((converged & edge).sum()),
               on_specimen_converged=int((converged & on).sum()), with_vector=int(has.sum()),
               mean_error=float(error[has].mean()) if has.any() else None, worst_error=float(error[has].max()) if has.any() else None)
    return fig, on, edge


@functools.lru_cache(maxsize=None)
def specimen_rows(name, refine=None):
    """The three rows of the table for one deformation: the refinement as it is, masked by the header's rule, masked with the
    pixel's own value only.  refine(scene, mask_or_None, u0, v0) stands in for the restatement (the device rows of
    tools/subset_mask_table.py).  The interior nodes -- on the specimen, every pixel usable -- must be the same bytes in all three."""
    c = SPECIMEN
    scene, mask, u0, v0 = specimen_case(name)
    kw = dict(max_shift=c["max_shift"])
    if refine is None:
        plain = subset_refine_from_reference(scene.frame_0, scene.frame_1, u0, v0, None, c["r"], c["s"], c["R"], **kw)
        masked, spread = all_orders_masked(scene.frame_0, scene.frame_1, u0, v0, None, mask, c["min_pixels"], c["r"], c["s"], c["R"], **kw)
        own = subset_refine_masked_reference(scene.frame_0, scene.frame_1, u0, v0, None, mask, c["min_pixels"], c["r"], c["s"], c["R"],
                                             stencil=False, **kw)
    else:
        plain, masked, own, spread = refine(scene, None, u0, v0), refine(scene, mask, u0, v0), None, None
    rows = {}
    for label, got in (("plain", plain), ("masked", masked), ("own_pixel_only", own)):
        if got is not None:
            rows[label], on, edge = edge_figures(scene, mask, got)
            interior = on & ~edge
            assert all(np.array_equal(bits(a)[interior], bits(b)[interior]) for a, b in zip(got.planes(), plain.planes())), label
    rows["masked"]["masked_nodes"] = int(masked.record["reserved"][0])
    rows["masked"]["spread"] = spread
    return rows, masked


def test_accuracy_on_the_stretched_specimen():
    """make_speckle_specimen("stretch"), seed 0, 96 x 80, grid r = 7, s = 8; search (d = 6), validation with replacement,
    refinement (R = 7, K = 20, epsilon 1e-3, max_shift 2, max_gradient 0.5), min_pixels 57.  Every node whose centre lies on
    the specimen converges under the mask, none left out (the restatement: 44 of 44, 40 of them edge nodes); the masked edge
    nodes' mean endpoint error is at most 0.03 px (0.0153), the unmasked ones' at least 0.15 px (0.242)."""
    rows, masked = specimen_rows("stretch")
    print(json.dumps(rows))
    m, p = rows["masked"], rows["plain"]
    assert m["on_specimen"] == 44 and m["edge"] == 40
    assert m["on_specimen_converged"] == m["on_specimen"] and m["converged"] == m["edge"]
    assert m["mean_error"] <= 0.03
    assert p["mean_error"] >= 0.15
    assert m["masked_nodes"] == 99 - 44 and m["spread"] < 1e-9
    assert (masked.state[np.isnan(masked.u)] == MASKED).all()


# what the restatement gives on the other two deformations (profiles/subset_mask/README.md): the edge nodes' mean error under the mask
# and without it; the bounds are the measured figures with a margin of a half -- times 1.5 above, times 0.5 below
OTHER_SPECIMENS = {"rotation": (0.0217, 0.247), "shear": (0.0275, 0.228)}


@pytest.mark.parametrize("name", sorted(OTHER_SPECIMENS))
def test_accuracy_on_the_rotated_and_the_sheared_specimen(name):
    """The same chain on the other two deformations: under the mask every on-specimen node converges (44 of 44, measured) and
    the edge nodes' mean error is at most 1.5 times the measured figure; without the mask it is at least half the measured one."""
    rows, _ = specimen_rows(name)
    print(json.dumps(rows))
    m, p = rows["masked"], rows["plain"]
    masked_mean, plain_mean = OTHER_SPECIMENS[name]
    assert m["on_specimen"] == 44 and m["edge"] == 40 and m["on_specimen_converged"] == 44
    assert m["mean_error"] <= 1.5 * masked_mean and p["mean_error"] >= 0.5 * plain_mean and m["spread"] < 1e-9


def test_the_specimen_scene():
    sc = scenes_module()
    scene, mask = sc.make_speckle_specimen("stretch", 96, 80, seed=0)
    plain = sc.make_speckle_deformation("stretch", 96, 80, seed=0)
    assert scene.frame_0.dtype == scene.frame_1.dtype == mask.dtype == np.float32 and mask.shape == (80, 96)
    assert set(np.unique(mask)) == {0.0, 1.0}
    inside = mask == 0
    # the plate |x - 47.5| <= 30.5, |y - 39.5| <= 24.5 without the hole of radius 9.5
    assert inside[15:65, 17:79].sum() == inside.sum() and not inside[39:41, 47:49].any() and inside[15, 17] and inside[64, 78]
    assert not inside[39, 39:57].any() and inside[39, 38] and inside[39, 57]
    assert np.array_equal(scene.frame_0[inside], plain.frame_0[inside]) and not np.array_equal(scene.frame_0[~inside], plain.frame_0[~inside])
    assert np.array_equal(scene.gt_u, plain.gt_u)
    # the background is static and dark; the specimen's texture moves with W
    far = np.s_[0:8, 0:10]
    assert np.array_equal(scene.frame_0[far], scene.frame_1[far]) and scene.frame_0[~inside].max() < 0.3 * 240 + 5
    ys, xs = np.mgrid[30:50, 62:72].astype(F64)
    there = scene.frame_1_at(xs + scene.gt_u[30:50, 62:72].astype(F64), ys + scene.gt_v[30:50, 62:72].astype(F64))
    assert np.abs(there - scene.frame_0[30:50, 62:72]).max() < 1e-3
    small, small_mask = sc.make_speckle_specimen("rotation", 48, 40, seed=2)
    assert small_mask.shape == (40, 48) and (small_mask == 0).sum() > 400 and small_mask[20, 24] == 1
    with pytest.raises(ValueError):
        sc.make_speckle_specimen("translation")


# ---- the entry's host side ------------------------------------------------------------------------------------------------------------
def test_masked_refusals_without_a_device(flow2d):
    lib = flow2d.hip_lib()
    fake = ctypes.create_string_buffer(4096)
    w, h, pitch, npitch = 100, 40, 512, 64
    span = pitch * h
    at = lambda k: (1 << 20) + k * (span + 4096)  # noqa: E731  (addresses only: nothing is dereferenced before the device is entered)
    d = dict(ctx=ctypes.addressof(fake), f0=at(0), f1=at(1), w=w, h=h, pitch=pitch, u0=at(2), v0=at(3), ux0=at(13), uy0=at(14), vx0=at(15),
             vy0=at(16), nw=11, nh=4, npitch=npitch, r=7, s=8, R=7, K=20, eps=1e-3, shift=4.0, grad=0.5, mask=at(17), min_pixels=57, u=at(4),
             v=at(5), ux=at(6), uy=at(7), vx=at(8), vy=at(9), score=at(10), state=at(11), record=at(12))

    def call(**kw):
        a = dict(d, **kw)
        return lib.flow2d_subset_refine_masked_2d(a["ctx"], a["f0"], a["f1"], a["w"], a["h"], a["pitch"], a["u0"], a["v0"], a["ux0"], a["uy0"],
                                                  a["vx0"], a["vy0"], a["nw"], a["nh"], a["npitch"], a["r"], a["s"], a["R"], a["K"], a["eps"],
                                                  a["shift"], a["grad"], a["mask"], a["min_pixels"], a["u"], a["v"], a["ux"], a["uy"], a["vx"],
                                                  a["vy"], a["score"], a["state"], a["record"])

    nan, inf = float("nan"), float("inf")
    bad = [dict(ctx=None), dict(f0=None), dict(f1=None), dict(u0=None), dict(v=None), dict(w=0), dict(nh=0), dict(pitch=pitch + 8),
           dict(npitch=32), dict(r=0), dict(s=65), dict(R=0), dict(R=16), dict(K=65), dict(eps=nan), dict(shift=0.0), dict(shift=inf),
           dict(grad=nan), dict(nw=12), dict(ux=None), dict(record=at(12) + 4), dict(u=at(0)), dict(uy=at(6)), dict(ux0=None),
           dict(uy0=None, vx0=None, vy0=None), dict(vx0=at(15) + 4), dict(u=at(13)), dict(record=at(15) + 64),
           # min_pixels outside 6 .. (2R + 1)^2
           dict(min_pixels=5), dict(min_pixels=0), dict(min_pixels=-1), dict(min_pixels=226), dict(R=1, min_pixels=10), dict(R=3, min_pixels=50),
           # the mask: a plane like the frames, met by no written range
           dict(mask=at(17) + 4), dict(u=at(17)), dict(vy=at(17) + span - pitch), dict(score=at(17) + pitch), dict(state=at(17)),
           dict(record=at(17) + 64)]
    # ... and without a mask whatever flow2d_subset_refine_from_2d refuses, min_pixels not looked at
    bad += [dict(mask=None, min_pixels=0, **kw) for kw in (dict(f1=None), dict(ux0=None), dict(h=14), dict(vy=None), dict(u=at(1)), dict(R=16))]
    for kw in bad:
        assert call(**kw) == 1, kw
    # (only refusals here: an accepted call would go on to launch on these made-up addresses where there is a device)


def test_python_record_alias_and_constants(flow2d):
    rec = flow2d.SubsetRecord()
    rec.nodes, rec.reserved = 9, 4
    assert rec.masked == 4 and np.frombuffer(bytes(rec), SUBSET_DTYPE)["reserved"][0] == 4
    with pytest.raises(AttributeError):
        rec.masked = 1
    assert list(rec.summary()) == list(SUBSET_DTYPE.names[:7])  # (what the other entries' callers print stays as it is)
    assert flow2d.SUBSET_MASKED == MASKED and flow2d.SUBSET_MIN_PIXELS == MIN_PIXELS
    assert [flow2d.subset_min_pixels(R) for R in (1, 2, 7, 15)] == [default_min_pixels(R) for R in (1, 2, 7, 15)] == [6, 7, 57, 241]


def test_subset_options_with_a_mask(flow2d):
    """OpticalFlow2D::SubsetOptionsOk: a mask goes with order 1 only, min_pixels is 0 (the default) or 6 .. (2R + 1)^2."""
    ok = flow2d.OpticalFlow.subset_options_ok
    assert ok(7, mask=True) and ok(7, mask=True, min_pixels=57) and ok(7, mask=True, min_pixels=6) and ok(7, mask=True, min_pixels=225)
    assert not ok(7, mask=True, order=2) and ok(7, order=2) and not ok(7, mask=True, order=2, min_pixels=57)
    assert not ok(7, mask=True, min_pixels=5) and not ok(7, mask=True, min_pixels=226) and not ok(7, mask=True, min_pixels=-1)
    assert ok(1, mask=True) and ok(1, mask=True, min_pixels=9) and not ok(1, mask=True, min_pixels=10) and not ok(16, mask=True)
    host = flow2d.host_lib()
    assert [host.flow2d_host_subset_min_pixels(R) for R in (1, 2, 7, 15)] == [default_min_pixels(R) for R in (1, 2, 7, 15)]
    # the one host entry refuses a call without its options; min_pixels goes with a mask, and a mask with order 1 (both before any call)
    assert host.flow2d_host_refine_nodes_device(None, None, None, None, None, 7, 8, None, None, None) == 1
    flow = flow2d.OpticalFlow.__new__(flow2d.OpticalFlow)  # (no object of the host layer: neither call gets as far as one)
    with pytest.raises(ValueError):
        flow.refine_nodes_device(None, None, None, None, 7, 8, 7, min_pixels=57)
    with pytest.raises(flow2d.Flow2DError) as refused:
        flow.refine_nodes_device(None, None, None, None, 7, 8, 7, mask=1 << 20, order=2)
    assert refused.value.status == 1


def test_the_options_record_has_the_host_layers_fields(flow2d):
    """flow2d_host_subset_options as ctypes lays it out against the C++ struct: one field made invalid at a time (the values are
    those OpticalFlow2D::SubsetOptionsOk refuses) is refused, and a refusal that follows each field alone shows that the offsets
    agree."""
    assert ctypes.sizeof(flow2d.SubsetOptions) == 40
    ok = flow2d.host_lib().flow2d_host_subset_options_ok
    assert ok(None) == 0
    R = 7
    default = dict(radius=R, iterations=20, epsilon=1e-3, max_shift=2.0, max_gradient=0.5, order=1, max_curvature=0.05, min_pixels=0, mask=None)
    assert [name for name, _ in flow2d.SubsetOptions._fields_] == list(default)

    def accepted(**fields):
        return ok(ctypes.byref(flow2d.SubsetOptions(**dict(default, **fields))))

    assert accepted() == 1 and accepted(mask=1) == 1
    nan = float("nan")
    bad = [dict(radius=0), dict(radius=16), dict(iterations=0), dict(epsilon=nan), dict(max_shift=0.0), dict(max_gradient=-1.0), dict(order=3),
           dict(max_curvature=nan), dict(min_pixels=5), dict(min_pixels=(2 * R + 1) ** 2 + 1), dict(mask=1, order=2)]
    for fields in bad:
        assert accepted(**fields) == 0, fields
    # ... and the same fields at the other end of what is accepted, with and without the mask's mark
    good = [dict(radius=1), dict(radius=15), dict(iterations=1), dict(iterations=64), dict(epsilon=0.0), dict(max_shift=1e-3),
            dict(max_gradient=1e-3), dict(order=2), dict(radius=2, order=2), dict(max_curvature=1e-3), dict(min_pixels=6),
            dict(min_pixels=(2 * R + 1) ** 2)]
    for fields in good:
        assert accepted(**fields) == 1, fields
        if fields.get("order") != 2:
            assert accepted(mask=1, **fields) == 1, fields
