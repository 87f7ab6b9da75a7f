"""flow2d_propagate_flow_2d on the MI355X: bytes and record against the numpy restatement of tests/test_propagate_cpu.py, over the
shapes at which the kernels take another path (one pixel, exactly one workgroup, a partial block in x and in y, several blocks) and
the fields the definition speaks of; per instance of a lock-step batch with a padded stride; under graph replay."""
import ctypes

import numpy as np
import pytest

from test_propagate_cpu import F32, U32, RECORD_FIELDS, bits, propagate_reference

pytestmark = pytest.mark.gpu
POISON = U32(0x7F7F7F7F)
SHAPES = [(1, 1), (64, 4), (67, 9), (130, 37), (257, 5)]


# ---- the fields ------------------------------------------------------------------------------------------------------------------
def grid(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return xs.astype(F32), ys.astype(F32)


def constant(w, h, u, v):
    return np.full((h, w), u, F32), np.full((h, w), v, F32)


def expansion(w, h, factor):
    xs, ys = grid(w, h)
    return (F32(factor - 1) * (xs - F32((w - 1) / 2))).astype(F32), (F32(factor - 1) * (ys - F32((h - 1) / 2))).astype(F32)


def two_layers(w, h):
    """A block in the middle moves by (2.5, -1.25) over a ground at rest: the block's leading edge collides with the ground."""
    u, v = constant(w, h, 0.0, 0.0)
    u[h // 4:max(h // 4 + 1, 3 * h // 4), w // 4:max(w // 4 + 1, w // 2)] = 2.5
    v[h // 4:max(h // 4 + 1, 3 * h // 4), w // 4:max(w // 4 + 1, w // 2)] = -1.25
    return u, v


def frames(w, h, seed):
    rng = np.random.default_rng(seed)
    f0, f1 = rng.uniform(0, 255, (h, w)).astype(F32), rng.uniform(0, 255, (h, w)).astype(F32)
    f1[h // 2, w // 2] = np.nan      # a difference that is not finite: q = 255
    f0[0, w - 1] = np.inf
    return f0, f1


def ties(w, h):
    """Columns in pairs: u = +0.5 beside u = -0.5, both landing exactly half a pixel off, on the same target."""
    xs, _ = grid(w, h)
    return np.where(xs.astype(np.int64) % 2 == 0, F32(0.5), F32(-0.5)).astype(F32), np.zeros((h, w), F32)


def specials(w, h, seed):
    rng = np.random.default_rng(seed)
    u, v = rng.normal(0, 2, (h, w)).astype(F32), rng.normal(0, 2, (h, w)).astype(F32)
    values = (np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38)
    for k in range(min(w * h, 18)):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        (u if k % 2 else v)[y, x] = values[k % len(values)]
    mask = (rng.uniform(0, 1, (h, w)) < 0.1).astype(F32)
    mask[0, 0] = np.nan          # not == 0: unusable
    mask[h - 1, w - 1] = -0.0    # == 0: usable
    return u, v, mask


def borders(w, h):
    """The first column lands exactly on -0.5 (pixel 0), the last on width - 0.5 (outside); rows alike."""
    u, v = constant(w, h, 0.0, 0.0)
    u[:, 0], u[:, w - 1] = -0.5, 0.5
    v[0, :], v[h - 1, :] = -0.5, 0.5
    return u, v


def cases(w, h):
    """name -> keyword arguments of propagate_reference"""
    out = {}
    out["zero"] = dict(zip("uv", constant(w, h, 0.0, 0.0)), fill_passes=0)
    out["integer"] = dict(zip("uv", constant(w, h, 2.0, -1.0)), fill_passes=0)
    out["half_integer"] = dict(zip("uv", constant(w, h, 1.5, -0.5)), fill_passes=0)
    out["ties"] = dict(zip("uv", ties(w, h)), fill_passes=0)
    out["expansion_1.5"] = dict(zip("uv", expansion(w, h, 1.5)), fill_passes=0)
    out["expansion_2.5"] = dict(zip("uv", expansion(w, h, 2.5)), fill_passes=4)
    f0, f1 = frames(w, h, w + h)
    out["layers"] = dict(zip("uv", two_layers(w, h)), fill_passes=2)
    out["layers_frames"] = dict(zip("uv", two_layers(w, h)), frame_from=f0, frame_to=f1, photo_scale=0.5, fill_passes=2)
    out["layers_frames_scale_0"] = dict(zip("uv", two_layers(w, h)), frame_from=f0, frame_to=f1, photo_scale=0.0, fill_passes=2)
    su, sv, mask = specials(w, h, 3 * w + h)
    lu, lv = two_layers(w, h)
    out["layers_mask"] = dict(u=lu, v=lv, mask=mask, frame_from=f0, frame_to=f1, fill_passes=1)
    out["specials"] = dict(u=su, v=sv, mask=mask, fill_passes=0)
    out["specials_frames"] = dict(u=su, v=sv, frame_from=f0, frame_to=f1, photo_scale=3.0, fill_passes=3)
    out["borders"] = dict(zip("uv", borders(w, h)), fill_passes=0)
    out["step_-1"] = dict(u=su, v=sv, step=-1.0, fill_passes=1)
    out["step_2"] = dict(zip("uv", expansion(w, h, 1.5)), step=2.0, fill_passes=1)
    for n in (0, 1, 3, 64):
        eu, ev = expansion(w, h, 2.5)
        eu[h // 3:h // 3 + 7, w // 3:w // 3 + 9] = np.nan  # a hole that three passes do not close
        out["fill_%d" % n] = dict(u=eu, v=ev, fill_passes=n)
    return out


CASE_NAMES = sorted(cases(3, 3))


def run_on_device(ctx, kw, w, h, pad=(3, 2)):
    """The entry on planes in a poisoned container wider and taller than the field: (u bits, v bits, record), the container beyond
    the field checked for writes."""
    cw, ch = w + pad[0], h + pad[1]

    def plane(a):
        return ctx.plane(cw, ch).fill_bytes(0x7F).upload(np.ascontiguousarray(a, F32)) if a is not None else None

    pu, pv, mask, f0, f1 = (plane(kw.get(name)) for name in ("u", "v", "mask", "frame_from", "frame_to"))
    out = [ctx.plane(cw, ch).fill_bytes(0x7F) for _ in range(2)]
    _, _, rec = ctx.propagate_flow(pu, pv, w, h, mask=mask, frame_from=f0, frame_to=f1, step=kw.get("step", 1.0),
                                   photo_scale=kw.get("photo_scale", 1.0), fill_passes=kw["fill_passes"], out_u=out[0], out_v=out[1])
    got = [bits(q.download()) for q in out]
    for g in got:
        assert (g[h:] == POISON).all() and (g[:, w:] == POISON).all(), "written beyond the field"
    return got[0][:h, :w], got[1][:h, :w], rec


@pytest.mark.parametrize("name", CASE_NAMES)
def test_entry_equals_the_restatement(ctx, name):
    for w, h in SHAPES:
        kw = cases(w, h)[name]
        want_u, want_v, want_rec = propagate_reference(**kw)
        got_u, got_v, rec = run_on_device(ctx, kw, w, h)
        for got, want, plane in ((got_u, want_u, "u"), (got_v, want_v, "v")):
            same = got == bits(want)
            assert same.all(), "%s %dx%d: %s differs at %d places, first (y, x) = %s" % (name, w, h, plane, (~same).sum(), np.argwhere(~same)[0])
        assert {k: getattr(rec, k) for k in RECORD_FIELDS} == want_rec and rec.reserved == 0, (name, w, h)
        assert rec.pixels == w * h == rec.unusable + rec.left + rec.landed


def test_the_cases_reach_what_they_are_for():
    """The fields do what their names say at the shapes of the test (the restatement alone: no device)."""
    w, h = 130, 37
    c = cases(w, h)
    rec = {name: propagate_reference(**kw)[2] for name, kw in c.items()}
    assert rec["zero"]["holes"] == 0 and rec["zero"]["landed"] == w * h
    assert rec["ties"]["holes"] > 0 and rec["ties"]["left"] == 0
    assert rec["expansion_1.5"]["holes"] > 0 and rec["expansion_2.5"]["filled"] > 0
    assert rec["specials"]["unusable"] > 10 and rec["specials"]["left"] >= 2
    assert rec["borders"]["left"] == h + w - 1  # the last column and the last row leave, the first ones stay
    assert rec["fill_0"]["unfilled"] == rec["fill_0"]["holes"] > 0 and rec["fill_64"]["unfilled"] == 0
    assert rec["fill_1"]["unfilled"] > rec["fill_3"]["unfilled"] > 0
    u_plain = propagate_reference(**c["layers_frames_scale_0"])[0]
    u_frames = propagate_reference(**c["layers_frames"])[0]
    assert np.array_equal(bits(u_plain), bits(propagate_reference(**c["layers"])[0])) and not np.array_equal(bits(u_plain), bits(u_frames))


def test_zero_flow_gives_the_input_back(ctx):
    w, h = 67, 9
    u, v = constant(w, h, 0.0, 0.0)
    u[2, 3], v[4, 5] = -0.0, 0.25  # (the winner's vector bit for bit: -0 stays -0; a quarter pixel lands on its own pixel)
    got_u, got_v, rec = run_on_device(ctx, dict(u=u, v=v, fill_passes=0), w, h)
    assert np.array_equal(got_u, bits(u)) and np.array_equal(got_v, bits(v)) and rec.holes == 0 and rec.landed == w * h


# ---- the context -------------------------------------------------------------------------------------------------------------------
def test_batch_of_three_with_a_padded_stride(ctx):
    w, h, G, pad = 67, 9, 3, 5
    stride_rows = h + pad
    names = ("layers_mask", "specials_frames", "fill_3")
    fields = []
    for b, name in enumerate(names):  # every instance needs every plane: those a case lacks are neutral
        kw = dict(cases(w, h)[name])
        f0, f1 = frames(w, h, 90 + b)
        kw.setdefault("mask", np.zeros((h, w), F32))
        kw.setdefault("frame_from", f0)
        kw.setdefault("frame_to", f1)
        kw.update(fill_passes=3, photo_scale=1.5)
        fields.append(kw)
    lone = [run_on_device(ctx, kw, w, h, pad=(0, 0)) for kw in fields]
    assert len({(r.holes, r.unusable) for _, _, r in lone}) == G

    def stack(arrays):
        full = np.full((stride_rows * G, w), POISON, U32)
        for b, a in enumerate(arrays):
            full[b * stride_rows:b * stride_rows + h] = bits(a)
        return ctx.plane(w, stride_rows * G).upload(full.view(F32))

    d = {name: stack([kw[name] for kw in fields]) for name in ("u", "v", "mask", "frame_from", "frame_to")}
    out = [stack([]) for _ in range(2)]
    record = ctx.propagate_records(G).fill_bytes(0x7F)
    work = ctx.propagate_workspace(w, h, G).fill_bytes(0x7F)
    with ctx.set_batch(G, stride_rows * d["u"].pitch):
        ctx.propagate_flow(d["u"], d["v"], w, h, mask=d["mask"], frame_from=d["frame_from"], frame_to=d["frame_to"], photo_scale=1.5,
                           fill_passes=3, out_u=out[0], out_v=out[1], record=record, workspace=work, instances=G)
    ctx.synchronize()
    records = ctx.read_propagate_record(record, G)
    for b in range(G):
        assert bytes(records[b]) == bytes(lone[b][2]), b
    for k, q in enumerate(out):
        got = bits(q.download())
        outside = np.ones(got.shape, bool)
        for b in range(G):
            r = b * stride_rows
            assert np.array_equal(got[r:r + h], lone[b][k]), (k, b)
            outside[r:r + h] = False
        assert (got[outside] == POISON).all(), "words outside the instances' regions were written"


def test_two_replays_of_a_captured_launch(flow2d, ctx):
    w, h = 130, 37
    lib = flow2d.hip_lib()
    vp = ctypes.c_void_p
    lib.flow2d_capture_begin.argtypes = [vp]
    lib.flow2d_capture_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.flow2d_graph_launch.argtypes = [vp, vp]
    lib.flow2d_graph_destroy.argtypes = [vp, vp]
    kw = cases(w, h)["specials_frames"]
    want_u, want_v, want_rec = propagate_reference(**kw)
    planes = [ctx.plane(w, h, kw[name]) for name in ("u", "v", "frame_from", "frame_to")]
    out = [ctx.plane(w, h).fill_bytes(0x7F) for _ in range(2)]
    record = ctx.propagate_records().fill_bytes(0x7F)
    work = ctx.propagate_workspace(w, h).fill_bytes(0x7F)
    args = dict(frame_from=planes[2], frame_to=planes[3], photo_scale=kw["photo_scale"], fill_passes=kw["fill_passes"], out_u=out[0],
                out_v=out[1], record=record, workspace=work)
    assert lib.flow2d_capture_begin(ctx.handle) == 0
    try:
        ctx.propagate_flow(planes[0], planes[1], w, h, **args)
    finally:
        graph = vp()
        assert lib.flow2d_capture_end(ctx.handle, ctypes.byref(graph)) == 0
    try:
        ctx.synchronize()
        assert (bits(out[0].download()) == POISON).all()  # captured, not run
        for _ in range(2):
            for q in out:
                q.fill_bytes(0x3C)
            assert lib.flow2d_graph_launch(ctx.handle, graph) == 0
            ctx.synchronize()
            assert np.array_equal(bits(out[0].download()), bits(want_u)) and np.array_equal(bits(out[1].download()), bits(want_v))
            rec = ctx.read_propagate_record(record)[0]
            assert {k: getattr(rec, k) for k in RECORD_FIELDS} == want_rec  # zeroed and counted again: not doubled
    finally:
        lib.flow2d_graph_destroy(ctx.handle, graph)


def test_refusals_on_the_device(flow2d, ctx):
    """What the entry can only refuse with a context: ranges that overlap across the instances of a batch."""
    w, h = 64, 4
    u, v = constant(w, h, 1.0, 0.0)
    tall = [ctx.plane(w, 3 * h, np.vstack([a] * 3)) for a in (u, v)]
    out = [ctx.plane(w, 3 * h) for _ in range(2)]
    record, work = ctx.propagate_records(3), ctx.propagate_workspace(w, h, 3)
    with ctx.set_batch(3, h * tall[0].pitch):
        ctx.propagate_flow(tall[0], tall[1], w, h, out_u=out[0], out_v=out[1], record=record, workspace=work, instances=3)  # accepted
        ctx.synchronize()
        with pytest.raises(flow2d.Flow2DError):  # instance 1 of the output is instance 0 of ... itself: out_v inside out_u's span
            ctx.propagate_flow(tall[0], tall[1], w, h, out_u=out[0], out_v=_shifted(out[0], h), record=record, workspace=work, instances=3)
    with pytest.raises(ValueError):
        ctx.propagate_flow(tall[0], tall[1], w, h, out_u=out[0])


class _shifted:
    """A Plane's handle `rows` rows further down."""

    def __init__(self, plane, rows):
        self.ptr, self.pitch, self.width, self.height = plane.ptr + rows * plane.pitch, plane.pitch, plane.width, plane.height - rows
