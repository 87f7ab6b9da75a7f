"""Motion segmentation, the parts that need no device: the new entries are exported, flow2d_segment_motion_workspace_bytes is host
logic, the entry refuses bad arguments before it touches the device, and segment_motion_reference -- the numpy restatement of
the definition in include/flow2d_c_abi.h and the checker of tests/test_gpu_segmentation.py -- finds two_layer's square, keeps a
ramp in one piece, separates two motions at a finite `join` and drops what is below `min_area`.

The restatement: foreground and edges in fp32, one operation at a time as the header writes them; components by union-find with
the smallest index as the representative -- vectorised: every edge hooks the larger of its two roots under the smaller
(np.minimum.at), then pointer jumping, until nothing changes --; numbering by smallest linear index; records and summary as
exact integer sums.  A plain-Python union-find over the edges (components_by_loop) checks it at the small shapes, and
scipy.ndimage.label where scipy imports.  Everything is an integer: there is no tolerance anywhere.

The case builders (PATTERNS, pattern_case, truncation and shape lists) are exported to the GPU file."""
import ctypes
import os

import numpy as np
import pytest

from test_denoise_cpu import scenes_module

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
TILE_W, TILE_H = 64, 16  # the kernels' tile: the shapes below straddle it in each direction
SMALL_SHAPES = [(1, 1), (2, 1), (1, 9), (5, 3), (64, 64), (65, 65), (67, 33), (257, 33), (300, 70), (640, 480),
                (63, 15), (64, 16), (65, 17)]
REGION_DTYPE = np.dtype([("area", "<u8"), ("sum_x", "<u8"), ("sum_y", "<u8"), ("sum_u_q16", "<i8"), ("sum_v_q16", "<i8"),
                         ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("first", "<u8")])
SUMMARY_DTYPE = np.dtype([("region_count", "<u8"), ("foreground", "<u8"), ("dropped", "<u8"), ("recorded", "<u4"),
                          ("reserved", "<u4")])
assert REGION_DTYPE.itemsize == 64 and SUMMARY_DTYPE.itemsize == 32


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def foreground_and_edges(ru, rv, mask, threshold, join):
    """(fg [h, w], right [h, w - 1], down [h - 1, w]): fg of the definition, and whether a pixel is joined to its right / lower
    neighbour.  fp32, each operation rounded on its own."""
    ru, rv = np.ascontiguousarray(ru, F32), np.ascontiguousarray(rv, F32)
    t, j = F32(threshold), F32(join)
    with np.errstate(invalid="ignore", over="ignore"):
        if mask is None:
            m = np.zeros_like(ru)
        else:
            m = np.array(mask, F32)
            m[~(m <= F32(1))] = F32(1)  # NaN: left out
            m[~(m >= F32(0))] = F32(0)
        fg = ((ru * ru + rv * rv) > t * t) & (m < F32(0.5))

        def joined(a, b):
            du, dv = ru[a] - ru[b], rv[a] - rv[b]
            return (du * du + dv * dv) <= j * j

        h, w = ru.shape
        left, right_ = (slice(None), slice(0, w - 1)), (slice(None), slice(1, w))
        up, down_ = (slice(0, h - 1), slice(None)), (slice(1, h), slice(None))
        right = fg[left] & fg[right_] & joined(left, right_)
        down = fg[up] & fg[down_] & joined(up, down_)
    return fg, right, down


def edge_lists(right, down, w):
    h = right.shape[0]
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    a = np.concatenate([idx[:, :-1][right], idx[:-1, :][down]])
    b = np.concatenate([idx[:, 1:][right], idx[1:, :][down]])
    return a, b


def components(fg, right, down):
    """root [h*w]: the smallest linear index of every pixel's component (-1 for background)."""
    h, w = fg.shape
    n = h * w
    parent = np.arange(n, dtype=np.int64)
    a, b = edge_lists(right, down, w)
    while a.size:
        ra, rb = parent[a], parent[b]
        low = np.minimum(ra, rb)
        np.minimum.at(parent, ra, low)
        np.minimum.at(parent, rb, low)
        while True:  # pointer jumping
            jumped = parent[parent]
            if np.array_equal(jumped, parent):
                break
            parent = jumped
        keep = parent[a] != parent[b]
        a, b = a[keep], b[keep]
    parent[~fg.ravel()] = -1
    return parent


def components_by_loop(fg, right, down):
    """The same by a plain union-find over the edges, one at a time."""
    h, w = fg.shape
    parent = list(range(h * w))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    a, b = edge_lists(right, down, w)
    for p, q in zip(a.tolist(), b.tolist()):
        p, q = find(p), find(q)
        if p != q:
            parent[max(p, q)] = min(p, q)
    root = np.array([find(i) for i in range(h * w)], np.int64)
    root[~fg.ravel()] = -1
    return root


def q16(r):
    """llrint((double)clamp(r, -32768.f, 32768.f) * 65536.0), round to nearest even."""
    return np.rint(np.clip(np.asarray(r, F32), F32(-32768), F32(32768)).astype(F64) * 65536.0).astype(np.int64)


def segment_motion_reference(ru, rv, threshold, join=INF, min_area=1, mask=None, max_regions=4096, root_of=components):
    """The definition of flow2d_segment_motion_2d: {"labels": int32 [h, w], "regions": REGION_DTYPE [max_regions],
    "summary": SUMMARY_DTYPE [1], "all_regions": REGION_DTYPE [region_count]}."""
    ru, rv = np.ascontiguousarray(ru, F32), np.ascontiguousarray(rv, F32)
    h, w = ru.shape
    fg, right, down = foreground_and_edges(ru, rv, mask, threshold, join)
    root = root_of(fg, right, down)
    on = root >= 0
    area = np.bincount(root[on], minlength=h * w)
    kept_roots = np.flatnonzero(area >= min_area)       # ascending: the order of the smallest linear index
    number = np.zeros(h * w + 1, np.int64)              # (index -1: background)
    number[kept_roots] = np.arange(1, kept_roots.size + 1)
    labels = number[root]
    k = labels[labels > 0] - 1
    ys, xs = np.divmod(np.arange(h * w, dtype=np.int64), w)
    sel = labels > 0
    count = kept_roots.size
    regions = np.zeros(count, REGION_DTYPE)
    regions["area"] = area[kept_roots]
    regions["first"] = kept_roots
    for name, values in (("sum_x", xs[sel]), ("sum_y", ys[sel]), ("sum_u_q16", q16(ru.ravel()[sel])),
                         ("sum_v_q16", q16(rv.ravel()[sel]))):
        total = np.zeros(count, np.int64)
        np.add.at(total, k, values)
        regions[name] = total
    for name, values, op, start in (("x0", xs[sel], np.minimum, w), ("y0", ys[sel], np.minimum, h), ("x1", xs[sel], np.maximum, -1),
                                    ("y1", ys[sel], np.maximum, -1)):
        bound = np.full(count, start, np.int64)
        op.at(bound, k, values)
        regions[name] = bound
    table = np.zeros(max_regions, REGION_DTYPE)
    recorded = min(count, max_regions)
    table[:recorded] = regions[:recorded]
    summary = np.zeros(1, SUMMARY_DTYPE)
    summary["region_count"], summary["foreground"] = count, int(fg.sum())
    summary["dropped"], summary["recorded"] = int(area[(area > 0) & (area < min_area)].sum()), recorded
    return {"labels": labels.reshape(h, w).astype(np.int32), "regions": table, "summary": summary, "all_regions": regions}


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------------------------
def spiral(w, h):
    """One long winding region: every other ring of the frame, each cut below its top-left corner and bridged to the next."""
    ys, xs = np.mgrid[0:h, 0:w]
    ring = np.minimum(np.minimum(xs, ys), np.minimum(w - 1 - xs, h - 1 - ys))
    on = ring % 2 == 0
    for k in range(0, (min(w, h) + 1) // 2, 2):
        if k + 2 < h - k and k + 2 < w - k - 2:
            on[k + 1, k] = False
            on[k + 2, k + 1] = True
    return on


def pattern_case(name, w, h):
    """One case: dict(ru, rv, mask, threshold, join, min_area).  The residuals are chosen so that the definition bites."""
    ys, xs = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(1000 * w + h)
    ru, rv = np.zeros((h, w), F32), np.zeros((h, w), F32)
    case = dict(mask=None, threshold=0.5, join=INF, min_area=1)

    def paint(on, u=2.0, v=-1.0):
        ru[on], rv[on] = u, v

    if name == "empty":
        ru[:], rv[:] = 0.25, -0.25   # below the threshold everywhere
    elif name == "full":
        paint(np.ones((h, w), bool))
    elif name in ("checkerboard", "checkerboard_dropped"):
        paint((xs + ys) % 2 == 0, 0.0, 1.5)
        case["min_area"] = 2 if name == "checkerboard_dropped" else 1
    elif name == "h_stripes":
        paint(ys % 2 == 0)
    elif name == "v_stripes":
        paint(xs % 2 == 0)
    elif name == "serpentine":
        paint((ys % 2 == 0) | ((ys % 4 == 1) & (xs == w - 1)) | ((ys % 4 == 3) & (xs == 0)))
    elif name == "spiral":
        paint(spiral(w, h))
    elif name == "comb":
        paint((xs % 2 == 0) | (ys == h - 1))
    elif name == "noise":
        on = rng.random((h, w)) < 0.59
        ru[on] = (1.0 + rng.random((h, w)))[on]
        rv[:] = rng.normal(0, 0.2, (h, w))
        case["min_area"] = 3
    elif name in ("rectangles", "rectangles_join"):
        paint((xs < w // 2) & (ys < max(h - 1, 1)), 2.0, 0.0)
        paint((xs >= w // 2) & (ys >= min(1, h - 1)), 5.0, 0.0)
        case["join"] = 1.0 if name == "rectangles_join" else INF
    elif name == "ramp":
        ru[:] = (1.0 + 0.4 * xs).astype(F32)
        ru[ys % 5 == 4] = 0.0
        case["join"] = 0.5
    elif name == "bar":
        paint(np.ones((h, w), bool))
        if w >= 5:
            ru[:, w // 3] = np.nan
            case["mask"] = np.zeros((h, w), F32)
            case["mask"][:, 2 * w // 3] = 1.0
            case["mask"][0, 0] = 0.25        # soft, still foreground
            case["mask"][h - 1, w - 1] = np.nan  # NaN = 1: left out
    elif name == "extremes":
        paint(np.ones((h, w), bool), 1.0, 1.0)
        wild = np.array([1e6, -1e6, np.inf, -np.inf, 32768.0, -32768.5, 3e38, 1.00001], F32)
        pick = rng.random((h, w)) < 0.3
        ru[pick] = rng.choice(wild, int(pick.sum()))
        pick = rng.random((h, w)) < 0.3
        rv[pick] = rng.choice(wild, int(pick.sum()))
    else:
        raise ValueError(name)
    case["ru"], case["rv"] = ru, rv
    return case


PATTERNS = ("empty", "full", "checkerboard", "checkerboard_dropped", "h_stripes", "v_stripes", "serpentine", "spiral", "comb",
            "noise", "rectangles", "rectangles_join", "ramp", "bar", "extremes")


def reference_of(case, max_regions=4096, **kw):
    return segment_motion_reference(case["ru"], case["rv"], case["threshold"], case["join"], case["min_area"], case["mask"],
                                    max_regions, **kw)


def two_layer_case(w, h):
    sc = scenes_module().make_scene("two_layer", w, h, seed=0)
    return sc, dict(ru=sc.gt_u, rv=sc.gt_v, mask=None, threshold=0.5, join=INF, min_area=1)


# ---- properties of the restatement ------------------------------------------------------------------------------------------------
def test_two_layer_is_one_square():
    sc, case = two_layer_case(64, 64)
    ref = reference_of(case)
    assert ref["summary"]["region_count"][0] == 1 and ref["summary"]["recorded"][0] == 1 and ref["summary"]["dropped"][0] == 0
    r = ref["regions"][0]
    assert r["area"] == 256 and (r["x0"], r["y0"], r["x1"], r["y1"]) == (20, 24, 35, 39)
    assert (r["sum_u_q16"] / 65536.0 / r["area"], r["sum_v_q16"] / 65536.0 / r["area"]) == (4.5, -2.25)
    assert (r["sum_x"] / r["area"], r["sum_y"] / r["area"]) == (27.5, 31.5) and r["first"] == 24 * 64 + 20
    assert np.array_equal(ref["labels"] == 1, sc.gt_u != 0) and ref["labels"].max() == 1
    assert not ref["regions"][1:].view(np.uint8).any()
    for (w, h), area in (((67, 33), 64), ((300, 70), 289)):
        ref = reference_of(two_layer_case(w, h)[1])
        assert ref["summary"]["region_count"][0] == 1 and ref["regions"][0]["area"] == area, (w, h)


def test_ramp_join_and_min_area():
    w, h = 40, 4
    ys, xs = np.mgrid[0:h, 0:w]
    ramp = dict(ru=(1.0 + 0.4 * xs).astype(F32), rv=np.zeros((h, w), F32), mask=None, threshold=0.5, join=0.5, min_area=1)
    ref = reference_of(ramp)
    assert ref["summary"]["region_count"][0] == 1 and ref["regions"][0]["area"] == w * h       # ends 15.6 px apart, one region
    assert reference_of(dict(ramp, join=0.39))["summary"]["region_count"][0] == w              # columns only
    rect = pattern_case("rectangles", 40, 9)
    one, two = reference_of(rect), reference_of(dict(rect, join=1.0))
    assert one["summary"]["region_count"][0] == 1 and two["summary"]["region_count"][0] == 2
    assert two["regions"]["area"][:2].sum() == one["regions"]["area"][0]
    assert two["regions"][0]["sum_u_q16"] == 2 * 65536 * two["regions"][0]["area"]
    assert two["regions"][1]["sum_u_q16"] == 5 * 65536 * two["regions"][1]["area"]
    # min_area: the regions below it become background, the others keep their order
    board = pattern_case("checkerboard", 8, 6)
    assert reference_of(board)["summary"]["region_count"][0] == 24
    dropped = reference_of(dict(board, min_area=2))
    assert dropped["summary"]["region_count"][0] == 0 and dropped["summary"]["dropped"][0] == dropped["summary"]["foreground"][0] == 24
    assert not dropped["labels"].any()
    mixed = dict(ru=np.array([[1, 0, 1, 1, 0, 1, 1, 1]], F32), rv=np.zeros((1, 8), F32), mask=None, threshold=0.5, join=INF, min_area=2)
    ref = reference_of(mixed)
    assert ref["labels"].tolist() == [[0, 0, 1, 1, 0, 2, 2, 2]] and ref["summary"]["dropped"][0] == 1
    assert ref["regions"]["first"][:2].tolist() == [2, 5]
    # a NaN residual and a mask of 1 cut a bar into three; a soft mask does not
    bar = reference_of(pattern_case("bar", 30, 5))
    assert bar["summary"]["region_count"][0] == 3 and bar["summary"]["foreground"][0] == 28 * 5 - 1
    # the clamp: +-1e6, +-inf and 3e38 count as +-32768
    wild = dict(ru=np.array([[1e6, -np.inf, 3e38, 1.5]], F32), rv=np.array([[-1e6, 0.0, 0.0, 2 ** -17]], F32), mask=None,
                threshold=0.5, join=INF, min_area=1)
    ref = reference_of(wild)
    assert ref["all_regions"]["sum_u_q16"].sum() == (32768 - 32768 + 32768) * 65536 + 98304
    assert ref["all_regions"]["sum_v_q16"].sum() == -32768 * 65536 + 0   # 2^-17 * 65536 = 0.5 rounds to even
    trunc = reference_of(pattern_case("checkerboard", 64, 64), max_regions=100)
    assert trunc["summary"]["region_count"][0] == 2048 and trunc["summary"]["recorded"][0] == 100 and trunc["labels"].max() == 2048
    assert len(trunc["regions"]) == 100 and trunc["regions"][99]["area"] == 1


@pytest.mark.parametrize("w,h", [s for s in SMALL_SHAPES if s[0] * s[1] <= 300 * 70])
def test_vectorised_components_equal_the_loop(w, h):
    for name in PATTERNS:
        case = pattern_case(name, w, h)
        fast, slow = reference_of(case), reference_of(case, root_of=components_by_loop)
        for key in ("labels", "regions", "summary"):
            assert fast[key].tobytes() == slow[key].tobytes(), (name, key)
        if name in ("serpentine", "spiral", "comb", "full") and w * h > 1:
            assert fast["summary"]["region_count"][0] == 1, name
        if name == "checkerboard":
            assert fast["summary"]["region_count"][0] == (w * h + 1) // 2


def test_plain_labelling_equals_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    for name in ("noise", "spiral", "comb", "checkerboard", "bar"):
        case = dict(pattern_case(name, 257, 33), min_area=1)
        ref = reference_of(case, max_regions=0)
        fg = foreground_and_edges(case["ru"], case["rv"], case["mask"], case["threshold"], case["join"])[0]
        labels, count = ndimage.label(fg)   # 4-connectivity, numbered in raster order of the first pixel
        assert count == ref["summary"]["region_count"][0] and np.array_equal(labels, ref["labels"]), name


# ---- the library without a device ---------------------------------------------------------------------------------------------------
def test_new_entries_are_exported(flow2d):
    lib, host = flow2d.hip_lib(), flow2d.host_lib()
    for name in ("flow2d_segment_motion_2d", "flow2d_segment_motion_workspace_bytes"):
        assert hasattr(lib, name), name
    for name in ("flow2d_host_segment_motion", "flow2d_host_segment_motion_device", "flow2d_host_segment_motion_args_ok"):
        assert hasattr(host, name), name
    for name in ("segment_motion", "read_regions", "read_segment_summary"):
        assert hasattr(flow2d.Context, name), name
    assert hasattr(flow2d.OpticalFlow, "segment_motion")
    assert lib.flow2d_abi_version() == 1  # additions: the version stays
    assert ctypes.sizeof(flow2d.MotionRegion) == flow2d.MOTION_REGION_BYTES == REGION_DTYPE.itemsize
    assert ctypes.sizeof(flow2d.SegmentSummary) == flow2d.SEGMENT_SUMMARY_BYTES == SUMMARY_DTYPE.itemsize
    for (name, kind), field in zip(flow2d.MotionRegion._fields_, REGION_DTYPE.names):
        assert name == field and getattr(flow2d.MotionRegion, name).offset == REGION_DTYPE.fields[field][1]
    header = open(os.path.join(ROOT, "include", "flow2d_c_abi.h")).read()
    assert "#define FLOW2D_MOTION_REGION_BYTES 64" in header and "#define FLOW2D_SEGMENT_SUMMARY_BYTES 32" in header


def test_workspace_bytes(flow2d):
    size = flow2d.hip_lib().flow2d_segment_motion_workspace_bytes
    assert size(0, 5, 1) == size(5, 0, 1) == size(5, 5, 0) == 0
    shapes = [(1, 1), (2, 1), (5, 3), (64, 16), (65, 17), (300, 70), (1920, 1080), (4096, 4096)]
    for w, h in shapes:
        one = size(w, h, 1)
        assert one >= 8 * w * h and one % 16 == 0, (w, h)
        assert size(w + 1, h, 1) >= one and size(w, h + 1, 1) >= one and size(8 * w, h, 1) > one and size(w, 8 * h, 1) > one
        for instances in (2, 3, 7):
            assert size(w, h, instances) == instances * one
    assert size(4096, 4096, 1) <= 8.25 * 4096 * 4096


BASE = 0x1000000


def test_entry_rejects_bad_arguments_without_a_device(flow2d):
    """Every refusal below happens before the context is touched: the context is a zeroed stand-in and the planes are 16-byte
    aligned addresses nothing reads."""
    lib = flow2d.hip_lib()
    fake_ctx = ctypes.create_string_buffer(4096)
    w, h, pitch = 64, 8, 256
    need = lib.flow2d_segment_motion_workspace_bytes(w, h, 1)
    d = dict(ctx=ctypes.addressof(fake_ctx), ru=BASE, rv=2 * BASE, mask=3 * BASE, w=w, h=h, pitch=pitch, threshold=0.5, join=INF,
             min_area=1, labels=4 * BASE, regions=5 * BASE, max_regions=16, summary=6 * BASE, ws=7 * BASE, ws_bytes=need)

    def call(**kw):
        a = dict(d, **kw)
        return lib.flow2d_segment_motion_2d(a["ctx"], a["ru"], a["rv"], a["mask"], a["w"], a["h"], a["pitch"], a["threshold"],
                                            a["join"], a["min_area"], a["labels"], a["regions"], a["max_regions"], a["summary"],
                                            a["ws"], a["ws_bytes"])

    assert call(ctx=None) == 1
    for name in ("ru", "rv", "labels", "regions", "summary", "ws"):
        assert call(**{name: None}) == 1, name
    assert call(mask=3 * BASE + 4) == 1
    assert call(w=0) == 1 and call(h=0) == 1
    assert call(w=1 << 16, h=1 << 15, pitch=4 << 16, ws_bytes=1 << 40) == 1   # width * height = 2^31
    assert call(pitch=8) == 1 and call(pitch=264) == 1 and call(pitch=128) == 1
    for bad in (-1.0, -1e-30, float("nan"), -INF):
        assert call(threshold=bad) == 1 and call(join=bad) == 1, bad
    assert call(min_area=0) == 1
    assert call(regions=5 * BASE + 4) == 1 and call(summary=6 * BASE + 4) == 1 and call(ws=7 * BASE + 8) == 1
    assert call(ws_bytes=need - 1) == 1
    for name in ("labels", "regions", "summary", "ws"):
        assert call(**{name: BASE}) == 1 and call(**{name: 2 * BASE + pitch}) == 1 and call(**{name: 3 * BASE}) == 1, name
    assert call(regions=4 * BASE) == 1 and call(summary=4 * BASE + 16) == 1 and call(ws=4 * BASE) == 1
    assert call(summary=5 * BASE + 64) == 1 and call(ws=5 * BASE + 15 * 64) == 1 and call(ws=6 * BASE + 16) == 1
    assert call(regions=7 * BASE + need - 64) == 1
