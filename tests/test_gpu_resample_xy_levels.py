"""flow2d_resample_xy_levels: the x and the y passes of all levels of a halving pyramid in one launch.

The contract is bit identity with flow2d_resample_x_levels followed by flow2d_resample_y_levels (compared on the uint32 view, so
NaN payloads, signed zeros and denormals count), refusal of every other geometry before anything is launched, an alias check by
byte ranges, and whole pipelines that still equal the CPU oracle in every pixel whichever path the geometry selects.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32, F32 = np.uint32, np.float32
POISON = 0x7F7F7F7F
INVALID_ARGUMENT, UNSUPPORTED = 1, 5


def random_plane(w, h, seed):
    return np.random.default_rng(seed).uniform(-4.0, 4.0, (h, w)).astype(F32)


def special_plane(w, h, seed):
    """Random values seeded with what ordinary arithmetic treats specially.  Rows 0-3: blocks of -0 (a chain that starts from +0
    gives +0, one that starts from its first cell gives -0); denormals that only survive without flushing; neighbours near FLT_MAX
    so that an x chain overflows to +Inf; +Inf above -Inf in one column so that a y chain meets Inf - Inf; NaNs with payloads."""
    a = random_plane(w, h, seed)
    a[0:4, 0:48] = -0.0
    a[4:8, 0:64] = np.array([1e-40, -3e-41, 1.4e-45, -1e-39], F32).repeat(16)[None, :]
    a[8:10, 0:8] = np.finfo(F32).max * F32(0.75)
    a[10, 16] = -np.finfo(F32).max
    a[10, 17] = -np.finfo(F32).max
    a[12, 33] = np.inf
    a[13, 33] = -np.inf
    a[14, 5] = -np.inf
    a.view(U32)[16, 7] = 0x7FC12345
    a.view(U32)[17, 40] = 0xFFC00001
    a.view(U32)[h - 1, w - 1] = 0x7FC00055
    a[h // 2, w // 2] = np.inf
    return a


class Stack:
    """`count` instances of a cw x ch container, `stride_rows` rows apart, in one plane; what the batched launchers address."""

    def __init__(self, ctx, cw, ch, count, stride_rows):
        self.ch, self.count, self.stride_rows = ch, count, stride_rows
        self.plane = ctx.plane(cw, stride_rows * count)
        self.ptr, self.pitch = self.plane.ptr, self.plane.pitch

    def put(self, arrays):
        full = np.full((self.plane.height, self.plane.width), POISON, U32)
        for b in range(self.count):
            a = np.ascontiguousarray(arrays[b % len(arrays)], F32).view(U32)
            full[b * self.stride_rows:b * self.stride_rows + a.shape[0], :a.shape[1]] = a
        self.plane.upload(full.view(F32))
        return self

    def poison(self):
        return self.put([np.zeros((0, 0), F32)])

    def get(self):
        full = self.plane.download().view(U32)
        return [full[b * self.stride_rows:(b + 1) * self.stride_rows] for b in range(self.count)]


def geometry(w, h, ratios, offsets):
    widths, heights = [w // r for r in ratios], [h // r for r in ratios]
    xcolumns, rows, columns = [], [], []
    column, row = 0, 5 if offsets else 0
    for i, (lw, lh) in enumerate(zip(widths, heights)):
        xcolumns.append(column)
        column += (lw + 3) // 4 * 4
        rows.append(row)
        row += lh + (i % 3 if offsets else 0)
        columns.append(4 * (1 + i % 4) if offsets else 0)
    return widths, heights, xcolumns, rows, columns, row


def compare(ctx, w, h, ratios, planes, make, count=1, pad_rows=0, extra_width=0, offsets=False):
    """The fused launch against the two launchers composed, every instance and every plane, every word of the output planes."""
    widths, heights, xcolumns, rows, columns, used_rows = geometry(w, h, ratios, offsets)
    cw, ch = w + extra_width, max(h, used_rows)
    stride_rows = ch + pad_rows
    sources = [[make(w, h, 100 * p + b) for b in range(count)] for p in range(planes)]
    src = [Stack(ctx, cw, ch, count, stride_rows).put(sources[p]) for p in range(planes)]
    packed, ref, out = ([Stack(ctx, cw, ch, count, stride_rows).poison() for _ in range(planes)] for _ in range(3))
    b = lambda group: group[1] if planes == 2 else None
    with ctx.set_batch(count, stride_rows * src[0].pitch):
        ctx.resample_x_levels(src[0], packed[0], w, h, widths, xcolumns, b(src), b(packed))
        ctx.resample_y_levels(packed[0], ref[0], h, widths, heights, xcolumns, rows, b(packed), b(ref))
        ctx.resample_xy_levels(src[0], out[0], w, h, widths, heights, rows, columns if offsets else None, b(src), b(out))
    ctx.synchronize()
    for p in range(planes):
        for inst, (want, got) in enumerate(zip(ref[p].get(), out[p].get())):
            untouched = np.ones(got.shape, bool)
            for lw, lh, row, column, ratio in zip(widths, heights, rows, columns, ratios):
                a, g = want[row:row + lh, :lw], got[row:row + lh, column:column + lw]
                assert not (a == POISON).any(), "the two launches left words of the region unwritten"
                assert np.array_equal(a, g), "plane %d, instance %d, ratio %d: %d of %d words differ" % (p, inst, ratio, (a != g).sum(), a.size)
                untouched[row:row + lh, column:column + lw] = False
            assert (got[untouched] == POISON).all(), "plane %d, instance %d: words outside the level regions were written" % (p, inst)
        for inst, (a, g) in enumerate(zip(sources[p], src[p].get())):
            assert np.array_equal(a.view(U32), g[:h, :w]), "an input changed"


HALVING = (2, 4, 8, 16, 32, 64, 128)


@pytest.mark.parametrize("make", [random_plane, special_plane], ids=["random", "special"])
@pytest.mark.parametrize("planes", [1, 2], ids=["plane", "pair"])
@pytest.mark.parametrize("w,h,ratios", [
    (256, 128, HALVING),                 # the deepest level is 2 x 1: LDS chains and a y chain as long as the frame
    (512, 256, (2, 4)), (64, 64, (2, 4)),
    (8192, 128, HALVING),                # the widest eligible width: 256 x 32 cells, eight column ranges
    (512, 256, HALVING + (256,)),        # a 256-row band: the sixteen-wave instantiation
    (64, 40, (2, 4, 8)),                 # no deep level and a last band that ends below the frame
    (256, 128, (2, 8, 64)),              # absent ratios between present ones
])
def test_fused_equals_the_two_launches(ctx, w, h, ratios, planes, make):
    compare(ctx, w, h, ratios, planes, make)


@pytest.mark.parametrize("make", [random_plane, special_plane], ids=["random", "special"])
@pytest.mark.parametrize("planes", [1, 2], ids=["plane", "pair"])
def test_batch_of_three_padded_stride_wide_pitch_offset_regions(ctx, planes, make):
    """3 instances, a batch stride of three rows more than the container, a pitch wider than the frame, and level regions at
    non-zero column and row offsets."""
    compare(ctx, 256, 128, HALVING, planes, make, count=3, pad_rows=3, extra_width=72, offsets=True)
    compare(ctx, 1024 + 32, 64, (2, 4, 8, 16, 32), planes, make, count=3, pad_rows=3, extra_width=40, offsets=True)


@pytest.mark.parametrize("w,h,lw,lh,why", [
    (96, 96, 32, 32, "ratio 3"),
    (48, 32, 24, 16, "width 48: no whole number of 32-cell threads"),
    (8192 + 32, 32, 4096 + 16, 16, "a width above the limit"),
    (256, 128, 128, 32, "different ratios in the two directions"),
])
def test_ineligible_geometry_is_refused_untouched(ctx, flow2d, w, h, lw, lh, why):
    src = ctx.plane(w, h, random_plane(w, h, 1))
    out = ctx.plane(w, h).fill_bytes(0x7F)
    with pytest.raises(flow2d.Flow2DError) as e:
        ctx.resample_xy_levels(src, out, w, h, [lw], [lh], [0])
    assert e.value.status == UNSUPPORTED, why
    ctx.synchronize()
    assert (out.download().view(U32) == POISON).all(), why


def test_overlapping_ranges_with_different_base_pointers_are_refused(ctx, flow2d):
    w, h = 256, 128
    src_a, src_b = ctx.plane(w, 2 * h, random_plane(w, 2 * h, 2)), ctx.plane(w, h, random_plane(w, h, 3))
    out = ctx.plane(w, 2 * h).fill_bytes(0x7F)
    pitch = out.pitch
    args = (w, h, [w // 2, w // 4], [h // 2, h // 4], [0, h // 2])
    refused = [
        dict(src_a=src_a, out_a=out.ptr, src_b=src_b, out_b=out.ptr + 16),                  # the two outputs, 16 bytes apart
        dict(src_a=src_a, out_a=out.ptr, src_b=src_b, out_b=out.ptr + 8 * pitch),           # ... and eight rows apart
        dict(src_a=src_a.ptr, out_a=src_a.ptr + (h - 1) * pitch),                           # the output starts in the input's last row
        dict(src_a=src_a.ptr + 40 * pitch, out_a=src_a.ptr),                                # the input starts inside the output rows
    ]
    for case in refused:
        with pytest.raises(flow2d.Flow2DError) as e:
            ctx.resample_xy_levels(case["src_a"], case["out_a"], *args, None, case.get("src_b"), case.get("out_b"), pitch=pitch)
        assert e.value.status == INVALID_ARGUMENT, case
    with pytest.raises(flow2d.Flow2DError) as e:  # two level regions of one plane that meet
        ctx.resample_xy_levels(src_a, out, w, h, [w // 2, w // 4], [h // 2, h // 4], [0, h // 2 - 1])
    assert e.value.status == INVALID_ARGUMENT
    ctx.synchronize()
    assert (out.download().view(U32) == POISON).all()
    # the same planes without the overlap: accepted (the rows behind the output's last region belong to nobody)
    ctx.resample_xy_levels(src_a.ptr, src_a.ptr + h * pitch, *args, pitch=pitch)
    ctx.synchronize()


@pytest.mark.parametrize("w,h,levels,scale,constancy,path", [
    (256, 256, 5, 0.5, 1, "fused"),      # Gradient, ratios 2 ... 16
    (200, 136, 4, 0.8, 0, "fallback"),   # no power-of-two ratios: the per-level passes
])
def test_pipelines_equal_the_oracle(flow2d, oracle, ctx, w, h, levels, scale, constancy, path):
    """OpticalFlow2D on a geometry of either path, eager and replayed from a graph: the oracle's flow in every pixel, and the
    pyramid built by the path the geometry selects (the process-wide count of one-launch pyramids: it rises with every eager run or recorded
    graph on the fused path and never on the fallback)."""
    p = flow2d.OpticalFlow.params(levels, scale, 3, 5, 35.0, 0.001, 0.001, 5, 1.5)
    f0, f1 = oracle.synthetic_pair(w, h, 1.5, -0.75, seed=7, noise=True)
    ou, ov = oracle.compute_flow(f0, f1, levels, scale, 3, 5, 35.0, 0.001, 0.001, 5, 1.5, constancy)[:2]
    flow = flow2d.OpticalFlow(w, h, constancy, ctx=ctx)
    try:
        planes = [ctx.plane(w, h, f0), ctx.plane(w, h, f1), ctx.plane(w, h), ctx.plane(w, h)]
        for graph, rounds in ((False, 1), (True, 2)):
            flow.use_graph(graph)
            for rnd in range(rounds):
                planes[2].fill_bytes(0x55)
                planes[3].fill_bytes(0x55)
                before = flow2d.resample_xy_levels_launches()
                flow.compute_flow_device(*[q.ptr for q in planes], p)
                ctx.synchronize()
                launched = flow2d.resample_xy_levels_launches() - before
                if path == "fallback" or rnd > 0:  # (a replayed graph calls no launcher)
                    assert launched == 0, (path, graph, rnd, launched)
                else:
                    assert launched >= 1, (path, graph, rnd, launched)
                assert np.array_equal(planes[2].download(), ou) and np.array_equal(planes[3].download(), ov), (path, graph, rnd)
    finally:
        flow.close()


def test_lock_step_group_of_three_equals_the_oracle(flow2d, oracle):
    """A group of 3 pairs in tall containers (every launch, the fused pyramid launch too, acts on the three instances), eager and
    replayed: each pair equals the oracle's flow of that pair alone."""
    w, h, G, constancy = 256, 128, 3, 1
    p = (5, 0.5, 3, 5, 35.0, 0.001, 0.001, 5, 1.5)
    pairs = [oracle.synthetic_pair(w, h, 1.0 + 0.5 * k, -0.5 * k, seed=30 + k, noise=True) for k in range(G)]
    want = [oracle.compute_flow(f0, f1, *p, constancy)[:2] for f0, f1 in pairs]
    c = flow2d.Context(0)
    batch = flow2d.OpticalFlowBatch(w, h, constancy, lanes=1, group_size=G)
    try:
        planes = [c.plane(w, h * G, np.vstack([q[0] for q in pairs])), c.plane(w, h * G, np.vstack([q[1] for q in pairs])),
                  c.plane(w, h * G), c.plane(w, h * G)]
        params = batch.params(*p)
        for graph, rounds in ((False, 1), (True, 2)):
            batch.use_graph(graph)
            for rnd in range(rounds):
                planes[2].fill_bytes(0x7F)
                planes[3].fill_bytes(0x7F)
                c.synchronize()
                before = flow2d.resample_xy_levels_launches()
                batch.compute_flow_batch_device(*[[q.ptr] for q in planes], params)
                batch.synchronize()
                launched = flow2d.resample_xy_levels_launches() - before
                assert (launched >= 1) if rnd == 0 else (launched == 0), ("the group's pyramids take the one-launch path", graph, rnd, launched)
                u, v = planes[2].download(), planes[3].download()
                for k, (wu, wv) in enumerate(want):
                    assert np.array_equal(u[k * h:(k + 1) * h], wu) and np.array_equal(v[k * h:(k + 1) * h], wv), (graph, rnd, k)
    finally:
        batch.close()
        c.close()
