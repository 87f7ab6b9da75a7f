"""flow2d_compose_nodes_2d restated in numpy from the text of include/flow2d_c_abi.h -- compose_reference, which the gpu tests and
tools/subset_reference_table.py import -- and the chain a sequence with a moving reference frame builds from it and from the
restatements of tests/test_subset_sequence_cpu.py: chained_with_reference.  What can be checked without a device: the properties
of the composition on hand-made fields, the table of the rotation to 60 degrees as a test, the entry's refusals, and the Python
constants and record."""
import ctypes
import functools
import json
import types

import numpy as np
import pytest

from test_correlate_cpu import F32, U32, NAN_BITS, bits, scenes_module
from test_subset_cpu import F64, Refined
from test_subset_sequence_cpu import PLANES, chained, judge, pair_chain, predict_passes, subset_refine_from_reference

COMPOSE_DTYPE = np.dtype([("nodes", "<u8"), ("composed", "<u8"), ("no_base", "<u8"), ("outside", "<u8"), ("no_increment", "<u8"),
                          ("reserved", "<u8", (3,))])
assert COMPOSE_DTYPE.itemsize == 64
COMPOSED = 66
CORNERS = ((0, 0), (1, 0), (0, 1), (1, 1))  # (di, dj), the header's order


# ---- flow2d_compose_nodes_2d ----------------------------------------------------------------------------------------------------------
def usable_nodes(nodes, state, min_state):
    with np.errstate(invalid="ignore"):
        ok = state >= F32(min_state)
    for q in nodes:
        ok = ok & np.isfinite(q)
    return ok


def cell_of(a, n):
    """i0 = floor(a) clamped to [0, n - 2] and t = a - i0 clamped to [0, 1]."""
    i0 = min(max(np.floor(a), F64(0)), F64(n - 2))
    t = min(max(a - i0, F64(0)), F64(1))
    return int(i0), t


def compose_reference(base, increment, r, s, min_state=1, score=None):
    """(the six planes u, v, ux, uy, vx, vy, the state plane, the score plane or None, the record) of flow2d_compose_nodes_2d;
    base and increment are the seven planes u, v, ux, uy, vx, vy, state each."""
    A = [np.ascontiguousarray(q, F32) for q in base]
    B = [np.ascontiguousarray(q, F32) for q in increment]
    nh, nw = A[6].shape
    assert nw >= 2 and nh >= 2
    usable_a, usable_b = usable_nodes(A[:6], A[6], min_state), usable_nodes(B[:6], B[6], min_state)
    a64, b64 = [q.astype(F64) for q in A[:6]], [q.astype(F64) for q in B[:6]]
    sc64 = None if score is None else np.ascontiguousarray(score, F32).astype(F64)
    out = [np.full((nh, nw), NAN_BITS, U32) for _ in range(6)]
    out_state = np.full((nh, nw), -1, F32)
    out_score = None if score is None else np.full((nh, nw), NAN_BITS, U32)
    record = np.zeros(1, COMPOSE_DTYPE)
    record["nodes"] = nh * nw
    rr, ss, one = F64(r), F64(s), F64(1)
    with np.errstate(all="ignore"):
        for j in range(nh):
            for i in range(nw):
                if not usable_a[j, i]:
                    record["no_base"] += 1
                    continue
                uA, vA, uxA, uyA, vxA, vyA = [q[j, i] for q in a64]
                X, Y = F64(r + i * s) + uA, F64(r + j * s) + vA
                a, b = (X - rr) / ss, (Y - rr) / ss
                if not (a >= -0.5 and a <= F64(nw) - 0.5 and b >= -0.5 and b <= F64(nh) - 0.5):
                    record["outside"] += 1
                    continue
                i0, tx = cell_of(a, nw)
                j0, ty = cell_of(b, nh)
                W, sums, sum_score = F64(0), [F64(0)] * 6, F64(0)
                for di, dj in CORNERS:
                    at = (j0 + dj, i0 + di)
                    if not usable_b[at]:
                        continue
                    w = (tx if di else one - tx) * (ty if dj else one - ty)
                    dx, dy = X - F64(r + (i0 + di) * s), Y - F64(r + (j0 + dj) * s)
                    u, v, ux, uy, vx, vy = [q[at] for q in b64]
                    W = W + w
                    for k, c in enumerate(((u + ux * dx) + uy * dy, (v + vx * dx) + vy * dy, ux, uy, vx, vy)):
                        sums[k] = sums[k] + w * c
                    if sc64 is not None:
                        sum_score = sum_score + w * sc64[at]
                if not W > 0:
                    record["no_increment"] += 1
                    continue
                record["composed"] += 1
                uB, vB, uxB, uyB, vxB, vyB = [q / W for q in sums]
                got = (uA + uB, vA + vB,
                       (((one + uxB) * (one + uxA)) + uyB * vxA) - one, (one + uxB) * uyA + uyB * (one + vyA),
                       vxB * (one + uxA) + (one + vyB) * vxA, ((vxB * uyA) + (one + vyB) * (one + vyA)) - one)
                for k in range(6):
                    out[k][j, i] = F32(got[k]).view(U32)
                out_state[j, i] = COMPOSED
                if out_score is not None:
                    out_score[j, i] = F32(sum_score / W).view(U32)
    for q in out + ([] if out_score is None else [out_score]):
        q[np.isnan(q.view(F32))] = NAN_BITS
    return [q.view(F32) for q in out], out_state, (None if out_score is None else out_score.view(F32)), record


def first5(record):
    """nodes, composed, no_base, outside, no_increment of a composition record."""
    return [int(record[n][0]) for n in COMPOSE_DTYPE.names[:5]]


# ---- the chain with a moving reference ------------------------------------------------------------------------------------------------
def seven(field):
    return [getattr(field, n) for n in PLANES] + [field.state]


def composed_field(planes, state, score, record):
    out = Refined()
    for name, plane in zip(PLANES, planes):
        setattr(out, name, plane)
    out.state, out.score, out.record = state, score, record
    return out


def chained_with_reference(scenes, r, s, R, reference_every=0, d=6, fill=2, min_state=1, max_shift=4.0, order="sequential",
                           refine_from=None, first=None, compose=None, **kw):
    """OpticalFlow2D::CorrelateSubsetSequence with SequenceOptions::reference_every = N: (the delivered field per step, the
    composition record per step or None where nothing was composed, the increments per step).  Step k is measured against frame
    ref(k) = N * floor((k - 1) / N); the steps with ref = 0 are `chained`'s; the first step after a change is the pair chain of
    search range d on (frame ref, frame k), the later ones the prediction passes and the refinement from the previous increment;
    the base of a reference ref > 0 is `fill` prediction passes over the delivered field of step ref.  refine_from(pair, nodes),
    first(pair) and compose(base, increment, score) stand in for the restatements (the device rows of the table tool)."""
    N = int(reference_every)
    steps = len(scenes)
    if N <= 0:
        got, _ = chained(scenes, r, s, R, fill=fill, max_shift=max_shift, order=order, refine_from=refine_from, first=first, **kw)
        return got, [None] * steps, got
    lead = min(N, steps)
    got, _ = chained(scenes[:lead], r, s, R, fill=fill, max_shift=max_shift, order=order, refine_from=refine_from, first=first, **kw)
    delivered, records, increments = list(got), [None] * lead, list(got)
    base = None
    for k in range(lead + 1, steps + 1):
        ref = N * ((k - 1) // N)
        pair = types.SimpleNamespace(frame_0=scenes[ref - 1].frame_1, frame_1=scenes[k - 1].frame_1)
        if ref == k - 1:
            nodes, state, _ = predict_passes(seven(delivered[ref - 1])[:6], delivered[ref - 1].state, s, fill, min_state)
            base = list(nodes) + [state]
            inc = first(pair) if first else pair_chain(pair, r, s, R, d, order=order, **kw)
        else:
            last = increments[-1]
            nodes, _, _ = predict_passes(seven(last)[:6], last.state, s, fill, min_state)
            if refine_from:
                inc = refine_from(pair, nodes)
            else:
                inc = subset_refine_from_reference(pair.frame_0, pair.frame_1, nodes[0], nodes[1], nodes[2:], r, s, R, max_shift=max_shift,
                                                   order=order, **kw)
        increments.append(inc)
        planes, state, score, record = (compose or compose_reference)(base, seven(inc), r, s, min_state, inc.score)
        delivered.append(composed_field(planes, state, score, record))
        records.append(record)
    return delivered, records, increments


ROTATION = dict(width=96, height=80, r=7, s=8, R=7, steps=15, step_size=4.0, d=6)
POLICIES = (0, 3, 5)


@functools.lru_cache(maxsize=None)
def rotation_scenes():
    c = ROTATION
    return scenes_module().make_speckle_deformation_sequence("rotation", c["steps"], c["step_size"], c["width"], c["height"], seed=0)


def step_rows(scenes, delivered, records, r, s, R, step_size):
    rows = []
    for k, (scene, step, record) in enumerate(zip(scenes, delivered, records)):
        row = dict(step=k + 1, amount=step_size * (k + 1), **judge(scene, step, r, s, R))
        row["compose"] = None if record is None else first5(record)
        rows.append(row)
    return rows


def sequence_rows(scenes, c, reference_every, **stand_ins):
    """(rows, delivered fields) of a sequence under one reference policy; every pair chain -- step 1's and the one after every
    reference change -- searches the range c["d"], as the host call does with its one schedule of passes."""
    first = stand_ins.pop("first", None) or (lambda pair: pair_chain(pair, c["r"], c["s"], c["R"], c["d"]))
    delivered, records, _ = chained_with_reference(scenes, c["r"], c["s"], c["R"], reference_every, c["d"], first=first, **stand_ins)
    return step_rows(scenes, delivered, records, c["r"], c["s"], c["R"], c["step_size"]), delivered


@functools.lru_cache(maxsize=None)
def rotation_rows(reference_every):
    """The table of the rotation to 60 degrees for one reference policy, restated (sequential order): (rows, delivered fields)."""
    return sequence_rows(rotation_scenes(), ROTATION, reference_every)


# The stretch sequence of the table: (1 + 0.04 k) x (1 - 0.02 k), fifteen steps at 96 x 80, to ux = 0.6.  The fixed reference loses
# its nodes from step 13 on, where the first-order warp's ux = 0.52 passes max_gradient = 0.5.
STRETCH = dict(ROTATION, step_size=0.04)


@functools.lru_cache(maxsize=None)
def stretch_scenes():
    c = STRETCH
    return scenes_module().make_speckle_deformation_sequence("stretch", c["steps"], c["step_size"], c["width"], c["height"], seed=0)


@functools.lru_cache(maxsize=None)
def stretch_rows(reference_every):
    return sequence_rows(stretch_scenes(), STRETCH, reference_every)


# ---- the composition on hand-made fields ----------------------------------------------------------------------------------------------
def affine_field(nh, nw, r, s, M, t, state=1.0):
    """The seven planes of the map x -> M x + t about the origin of the frame, on the grid (r, s): u = (M - I) x + t."""
    cy, cx = np.meshgrid(F64(r) + np.arange(nh) * F64(s), F64(r) + np.arange(nw) * F64(s), indexing="ij")
    G = np.asarray(M, F64) - np.eye(2)
    u, v = G[0, 0] * cx + G[0, 1] * cy + t[0], G[1, 0] * cx + G[1, 1] * cy + t[1]
    planes = [u, v] + [np.full((nh, nw), g) for g in (G[0, 0], G[0, 1], G[1, 0], G[1, 1])]
    return [q.astype(F32) for q in planes] + [np.full((nh, nw), state, F32)]


def rotation_about(deg, cx, cy):
    a = np.radians(deg)
    M = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return M, np.array([cx, cy]) - M @ np.array([cx, cy])


def test_two_affine_fields_compose_to_the_product_map():
    """A: a rotation of 10 degrees about the grid's centre plus a translation.  B: a stretch and shear.  An affine field's
    first-order extrapolation is exact, so B sampled anywhere is B there, and the result is the field of M_B M_A, t_B + M_B t_A:
    u and v within 1e-5 px (a float ulp at these displacements is 1e-6), the gradients within 1e-6 (they are below 1, ulp 6e-8)."""
    nh, nw, r, s = 9, 11, 7, 8
    MA, tA = rotation_about(10.0, 47.0, 39.0)
    tA = tA + np.array([1.25, -0.75])
    MB, tB = np.array([[1.04, 0.03], [-0.02, 0.97]]), np.array([-0.5, 0.25])
    A, B = affine_field(nh, nw, r, s, MA, tA), affine_field(nh, nw, r, s, MB, tB)
    planes, state, score, record = compose_reference(A, B, r, s)
    want = affine_field(nh, nw, r, s, MB @ MA, tB + MB @ tA)
    done = state == COMPOSED
    # (the rotation carries the nodes far from its centre more than half a cell off the grid: those are outside)
    assert first5(record) == [nh * nw, int(done.sum()), 0, nh * nw - int(done.sum()), 0] and done.sum() >= nh * nw // 2 and score is None
    for k in range(6):
        err = np.abs(planes[k].astype(F64) - want[k].astype(F64))[done].max()
        print(PLANES[k], err)
        assert err <= (1e-5 if k < 2 else 1e-6), PLANES[k]


def test_a_zero_base_returns_the_increment_bit_for_bit():
    nh, nw, r, s = 5, 6, 3, 4
    rng = np.random.default_rng(3)
    B = [(rng.standard_normal((nh, nw)) * a).astype(F32) for a in (2.0, 2.0, 0.1, 0.1, 0.1, 0.1)] + [np.full((nh, nw), 4, F32)]
    assert all((q != 0).all() for q in B[:2])
    A = [np.zeros((nh, nw), F32) for _ in range(6)] + [np.ones((nh, nw), F32)]
    sc = rng.random((nh, nw)).astype(F32)
    planes, state, score, record = compose_reference(A, B, r, s, score=sc)
    assert first5(record) == [nh * nw, nh * nw, 0, 0, 0] and (state == COMPOSED).all() and not record["reserved"].any()
    assert np.array_equal(bits(planes[0]), bits(B[0])) and np.array_equal(bits(planes[1]), bits(B[1]))
    assert np.array_equal(bits(score), bits(sc))
    for k in range(2, 6):  # (1 + g) - 1 rounds: the gradients come back to a double ulp of 1, not bit for bit
        assert np.abs(planes[k].astype(F64) - B[k].astype(F64)).max() <= 2.0 ** -24


def holes_case():
    """A 6 x 5 grid (r = 3, s = 4) with every kind of node: (base, increment, score, what each node must be)."""
    nh, nw, r, s = 5, 6, 3, 4
    rng = np.random.default_rng(11)
    A = [(rng.standard_normal((nh, nw)) * a).astype(F32) for a in (0.8, 0.8, 0.05, 0.05, 0.05, 0.05)] + [np.full((nh, nw), 3, F32)]
    B = [(rng.standard_normal((nh, nw)) * a).astype(F32) for a in (0.8, 0.8, 0.05, 0.05, 0.05, 0.05)] + [np.full((nh, nw), 2, F32)]
    sc = rng.random((nh, nw)).astype(F32)
    kind = np.full((nh, nw), "composed", object)
    A[6][0, 0] = -3                      # a lost base node
    kind[0, 0] = "no_base"
    A[3][0, 1] = np.nan                  # a NaN in a converged base node
    kind[0, 1] = "no_base"
    A[0][2, 0], A[1][2, 0] = -2.5, 0.0   # carried 0.625 of a cell beyond the left edge
    kind[2, 0] = "outside"
    A[0][4, 5], A[1][4, 5] = 0.0, 2.5    # ... beyond the bottom edge
    kind[4, 5] = "outside"
    A[0][0, 5], A[1][0, 5] = 1.5, -1.5   # 0.375 of a cell beyond the corner: inside, clamped, extrapolated
    # a cell whose four corners are lost: the base node (3, 3) lands inside cell (3 .. 4, 3 .. 4)
    A[0][3, 3], A[1][3, 3] = 1.0, 1.0
    for at in ((3, 3), (3, 4), (4, 3), (4, 4)):
        B[6][at] = -3
    B[2][4, 4] = np.nan
    kind[3, 3] = "no_increment"
    # the nodes (3, 4), (4, 3), (4, 4) of the base lie near lost corners as well: send them where the cell is whole or partly lost
    A[0][3, 4], A[1][3, 4] = 1.0, -3.0   # into cell (4 .. 5, 2 .. 3): corners (2,4) (2,5) usable, (3,4) lost, (3,5) usable
    A[0][4, 3], A[1][4, 3] = -3.0, -1.0  # into cell (2 .. 3, 3 .. 4): (3,2) usable, (3,3) lost, (4,2) usable, (4,3) lost
    A[0][4, 4], A[1][4, 4] = 2.0, -6.0   # into cell (4 .. 5, 2 .. 3) again
    # a NaN in a converged node of the increment counts as lost: node (1, 1) sits exactly on it (weight 1 on a lost corner)
    A[0][1, 1] = A[1][1, 1] = 0.0
    B[5][1, 1] = np.inf
    kind[1, 1] = "no_increment"
    # a state-0 node of the increment, exactly under base node (1, 3): lost at min_state 1, usable at 0
    A[0][1, 3] = A[1][1, 3] = 0.0
    B[6][1, 3] = 0
    return A, B, sc, kind, r, s


def test_lost_outside_and_uncovered_nodes_get_nan_and_their_own_count():
    A, B, sc, kind, r, s = holes_case()
    kind = kind.copy()
    kind[1, 3] = "no_increment"  # min_state 1
    planes, state, score, record = compose_reference(A, B, r, s, 1, sc)
    names = ["composed", "no_base", "outside", "no_increment"]
    assert first5(record) == [kind.size] + [int((kind == n).sum()) for n in names], (first5(record), state)
    assert min(first5(record)[1:]) >= 2
    lost = kind != "composed"
    assert np.array_equal(state == -1, lost) and (state[~lost] == COMPOSED).all()
    for q in planes + [score]:
        assert (bits(q)[lost] == NAN_BITS).all() and np.isfinite(q[~lost]).all()


def test_a_cell_with_lost_corners_uses_the_rest():
    """Base node (3, 4) lands at a = 4.25, b = 2.25 in cell (4 .. 5, 2 .. 3) whose corner (3, 4) is lost: the result is the other
    three corners' extrapolations, weighted and divided by their weights' sum."""
    A, B, sc, kind, r, s = holes_case()
    planes, state, score, record = compose_reference(A, B, r, s, 1, sc)
    assert state[3, 4] == COMPOSED
    X, Y = F64(r + 4 * s) + F64(A[0][3, 4]), F64(r + 3 * s) + F64(A[1][3, 4])
    tx, ty = (X - r) / s - 4, (Y - r) / s - 2
    assert (tx, ty) == (0.25, 0.25)
    W = uB = sB = F64(0)
    for (di, dj) in ((0, 0), (1, 0), (1, 1)):
        at = (2 + dj, 4 + di)
        w = (tx if di else 1 - tx) * (ty if dj else 1 - ty)
        W += w
        uB += w * ((F64(B[0][at]) + F64(B[2][at]) * (X - (r + (4 + di) * s))) + F64(B[3][at]) * (Y - (r + (2 + dj) * s)))
        sB += w * F64(sc[at])
    assert planes[0][3, 4] == F32(F64(A[0][3, 4]) + uB / W) and score[3, 4] == F32(sB / W)
    # with the corner usable again the value changes: it was really left out
    B[6][3, 4] = 2
    again, _, _, _ = compose_reference(A, B, r, s, 1, sc)
    assert again[0][3, 4] != planes[0][3, 4]


def test_half_a_cell_beyond_the_hull_is_extrapolated_not_refused():
    A, B, sc, kind, r, s = holes_case()
    planes, state, _, _ = compose_reference(A, B, r, s, 1, sc)
    # node (0, 5): a = 5.375, b = -0.375: cell (4 .. 5, 0 .. 1), tx = 1, ty = 0: corner (0, 5) alone, extrapolated
    X, Y = F64(r + 5 * s) + 1.5, F64(r) - 1.5
    at = (0, 5)
    uB = (F64(B[0][at]) + F64(B[2][at]) * (X - (r + 5 * s))) + F64(B[3][at]) * (Y - r)
    assert state[at] == COMPOSED and planes[0][at] == F32(1.5 + uB / 1.0)


def test_min_state_decides_on_a_state_0_node():
    A, B, sc, kind, r, s = holes_case()
    strict, state1, _, record1 = compose_reference(A, B, r, s, 1, sc)
    loose, state0, _, record0 = compose_reference(A, B, r, s, 0, sc)
    assert state1[1, 3] == -1 and state0[1, 3] == COMPOSED and bits(strict[0])[1, 3] == NAN_BITS
    assert loose[0][1, 3] == F32(F64(A[0][1, 3]) + F64(B[0][1, 3]))
    assert first5(record0)[1] > first5(record1)[1] and first5(record0)[4] < first5(record1)[4]
    # ... and a state-0 node of the base
    A[6][2, 2] = 0
    assert compose_reference(A, B, r, s, 1, sc)[1][2, 2] == -1 and compose_reference(A, B, r, s, 0, sc)[1][2, 2] == COMPOSED


def test_the_minimum_grid_clamps_every_cell():
    """2 x 2: one cell; every node's i0 = j0 = 0 and tx, ty in [0, 1] however far (up to half a cell) it is carried."""
    r, s = 2, 3
    A = [np.array(q, F32) for q in ([[-1.4, 1.4], [0.5, -0.5]], [[-1.4, -1.4], [1.4, 0.25]], [[0.01, 0], [0, 0]], [[0, 0.02], [0, 0]],
                                    [[0, 0], [0.03, 0]], [[0, 0], [0, -0.01]], [[1, 1], [1, 1]])]
    B = affine_field(2, 2, r, s, np.array([[1.02, 0.01], [0.0, 0.99]]), np.array([0.3, -0.2]))
    planes, state, _, record = compose_reference(A, B, r, s)
    assert first5(record) == [4, 4, 0, 0, 0]
    for (j, i) in ((0, 0), (0, 1), (1, 0), (1, 1)):
        X, Y = r + i * s + F64(A[0][j, i]), r + j * s + F64(A[1][j, i])
        want = F64(A[0][j, i]) + (0.02 * X + 0.01 * Y + 0.3)
        assert abs(F64(planes[0][j, i]) - want) < 1e-6


# ---- the table's condition ------------------------------------------------------------------------------------------------------------
def test_reference_every_0_is_the_chain_as_it_was():
    c = ROTATION
    scenes = rotation_scenes()[:3]
    want, _ = chained(scenes, c["r"], c["s"], c["R"])
    got, records, increments = chained_with_reference(scenes, c["r"], c["s"], c["R"], 0, c["d"])
    assert records == [None] * 3 and len(got) == 3
    for a, b in zip(got, want):
        assert all(np.array_equal(bits(getattr(a, n)), bits(getattr(b, n))) for n in Refined.NAMES) and a.record.tobytes() == b.record.tobytes()


@pytest.mark.parametrize("reference_every", [3, 5])
def test_a_moving_reference_follows_the_rotation_to_60_degrees(reference_every):
    """Speckle(0) at 96 x 80, grid r = 7, s = 8, R = 7, the defaults elsewhere, a rotation of 4 degrees per step to 60 degrees; the
    first step after a reference change is a pair chain of search range 6.  At every step found >= judged - 2 and wrong = 0."""
    rows, _ = rotation_rows(reference_every)
    for row in rows:
        print(json.dumps(row))
    for row in rows:
        assert row["judged"] >= 50 and row["good"] >= row["judged"] - 2 and row["wrong"] == 0, row
        assert (row["compose"] is None) == (row["step"] <= reference_every), row


def test_the_fixed_reference_finds_nothing_from_32_degrees_on():
    rows, _ = rotation_rows(0)
    for row in rows:
        print(json.dumps(row))
    assert [row["amount"] for row in rows[7:]] == [32.0 + 4 * k for k in range(8)]
    for row in rows[7:]:
        assert row["judged"] >= 50 and row["good"] == 0, row


# ---- the entry's host side ------------------------------------------------------------------------------------------------------------
def test_compose_refusals_without_a_device(flow2d):
    lib = flow2d.hip_lib()
    fake = ctypes.create_string_buffer(4096)
    npitch, nh = 64, 4
    span = npitch * nh
    at = lambda k: (1 << 20) + k * 4096  # noqa: E731  (addresses only: nothing is dereferenced before the device is entered)
    names = ("u", "v", "ux", "uy", "vx", "vy", "state")
    d = dict(ctx=ctypes.addressof(fake), nw=11, nh=nh, npitch=npitch, r=7, s=8, min_state=1, score=at(14), out_score=at(23), record=at(24))
    d.update({"a_" + n: at(i) for i, n in enumerate(names)})
    d.update({"b_" + n: at(7 + i) for i, n in enumerate(names)})
    d.update({"out_" + n: at(16 + i) for i, n in enumerate(names)})

    def call(base=True, increment=True, out=True, **kw):
        a = dict(d, **kw)
        arrays = [(ctypes.c_void_p * 7)(*[a[p + n] for n in names]) for p in ("a_", "b_")] + [(ctypes.c_void_p * 6)(*[a["out_" + n] for n in names[:6]])]
        return lib.flow2d_compose_nodes_2d(a["ctx"], arrays[0] if base else None, arrays[1] if increment else None, a["score"], a["nw"],
                                           a["nh"], a["npitch"], a["r"], a["s"], a["min_state"], arrays[2] if out else None, a["out_state"],
                                           a["out_score"], a["record"])

    assert call(base=False) == 1 and call(increment=False) == 1 and call(out=False) == 1
    bad = [dict(ctx=None)] + [{"a_" + n: None} for n in names] + [{"b_" + n: None} for n in names] + [{"out_" + n: None} for n in names[:6]]
    bad += [dict(nw=0), dict(nh=0), dict(nw=1), dict(nh=1), dict(npitch=32), dict(npitch=npitch + 4), dict(a_u=at(0) + 4), dict(b_vy=at(12) + 8),
            dict(out_state=at(22) + 8), dict(score=at(14) + 4), dict(r=0), dict(r=16), dict(s=0), dict(s=65), dict(min_state=-1), dict(min_state=2),
            dict(record=at(24) + 4), dict(score=None), dict(out_score=None),
            dict(out_u=at(0)), dict(out_vy=at(6) + span - npitch), dict(out_state=at(10)), dict(out_v=at(16)), dict(out_state=at(21) + npitch),
            dict(out_score=at(14)), dict(out_score=at(22)), dict(record=at(9)), dict(record=at(17) + 64), dict(out_ux=at(13))]
    for kw in bad:
        assert call(**kw) == 1, kw
    # 2^31 nodes: FLOW2D_ERR_UNSUPPORTED, behind every other check
    assert call(nw=1 << 16, nh=1 << 15, npitch=4 << 16) == 5
    assert call(nw=1 << 16, nh=1 << 15, npitch=4 << 16, min_state=2) == 1


def test_host_entries_refuse_without_an_object(flow2d):
    """The host facade's new entries with no object: each refuses (1), the records' count is 0; nothing needs a device."""
    host = flow2d.host_lib()
    assert [host.flow2d_host_set_reference_every(None, n) for n in (-1, 0, 3)] == [1, 1, 1]
    assert host.flow2d_host_compose_records(None, None, 4) == 0
    seven, eight = (ctypes.c_void_p * 7)(*[4096] * 7), (ctypes.c_void_p * 8)(*[4096] * 8)
    assert host.flow2d_host_compose_nodes_device(None, seven, eight, 7, 8, 1, eight, None) == 1
    fp = ctypes.POINTER(ctypes.c_float)
    assert host.flow2d_host_compose_nodes(None, (fp * 7)(), (fp * 8)(), 7, 8, 1, (fp * 8)(), None) == 1
    # the Python wrappers check their own arguments before any call
    flow = flow2d.OpticalFlow.__new__(flow2d.OpticalFlow)
    flow.width, flow.height = 96, 80
    with pytest.raises(ValueError):
        flow.compose_nodes({"u": 0}, {"u": 0}, 7, 8)
    field = {n: np.zeros((9, 11), F32) for n in flow2d.OpticalFlow.COMPOSE_BASE}
    with pytest.raises(ValueError):
        flow.compose_nodes(field, {n: np.zeros((9, 10), F32) for n in field}, 7, 8)


def test_python_record_and_constants(flow2d):
    rec = flow2d.ComposeRecord()
    rec.nodes, rec.composed, rec.no_base, rec.outside, rec.no_increment = 9, 1, 2, 3, 4
    a = np.frombuffer(bytes(rec), COMPOSE_DTYPE)[0]
    assert list(a.tolist()[:5]) == [9, 1, 2, 3, 4] and not a["reserved"].any()
    assert ctypes.sizeof(flow2d.ComposeRecord) == flow2d.COMPOSE_RECORD_BYTES == COMPOSE_DTYPE.itemsize
    assert flow2d.SUBSET_STATE_COMPOSED == COMPOSED == flow2d.SUBSET_STATE_PREDICTED + 1
    assert list(rec.summary()) == list(COMPOSE_DTYPE.names[:5])
