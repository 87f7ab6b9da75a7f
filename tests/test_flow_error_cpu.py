"""Flow error against ground truth, the parts that need no device: the new entries are exported, flow2d_flow_error_2d refuses
bad arguments before it touches the device, the ctypes record matches the C header, Middlebury .flo files round-trip and bad
ones are refused, the numpy restatement of the metrics (include/flow2d_c_abi.h, flow2d_flow_error_2d) -- the checker of
tests/test_gpu_flow_error.py -- gives hand-computed answers, and every analytic scene satisfies its ground truth."""
import ctypes
import importlib
import os
import struct
import subprocess

import numpy as np
import pytest

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = (0.5, 1.0, 2.0, 3.0)


def flow_error_reference(u, v, gt_u, gt_v, occlusion=None):
    """flow2d_flow_error_2d restated: returns (record, epe, ae).  The EPE, the classes and the counts follow the definition
    operation for operation in fp32; the AE is the exact angle in float64 (the device's is within 1e-4 degrees of it); the
    sums are float64 sums of the float32 EPE (and of this float64 AE)."""
    u, v, gu, gv = (np.asarray(a, F32) for a in (u, v, gt_u, gt_v))
    with np.errstate(invalid="ignore", over="ignore"):
        valid = (np.abs(gu) <= F32(1e9)) & (np.abs(gv) <= F32(1e9))
        take = valid & np.isfinite(u) & np.isfinite(v)
        du, dv = u - gu, v - gv
        epe = np.sqrt(du * du + dv * dv)
        a = np.stack([u, v, np.ones_like(u)], -1).astype(np.float64)
        b = np.stack([gu, gv, np.ones_like(gu)], -1).astype(np.float64)
        ae = np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1)))
        gmag = np.sqrt(gu * gu + gv * gv)
        occluded = np.zeros(u.shape, bool) if occlusion is None else (np.asarray(occlusion, F32) != 0)
        rec = {"invalid_ground_truth": int((~valid).sum()), "nonfinite_estimate": int((valid & ~take).sum())}
        for name, sel in (("all", take), ("noc", take & ~occluded), ("occ", take & occluded)):
            e = epe[sel]
            rec[name] = {"count": int(sel.sum()), "above": [int((e > F32(t)).sum()) for t in THRESHOLDS],
                         "fl": int(((e > F32(3)) & (e > F32(0.05) * gmag[sel])).sum()),
                         "sum_epe": float(e.astype(np.float64).sum()),
                         "sum_epe_sq": float((e.astype(np.float64) ** 2).sum()),
                         "sum_ae": float(ae[sel].sum()), "max_epe": float(e.max()) if e.size else 0.0}
    nan = F32(np.nan)
    return rec, np.where(take, epe, nan).astype(F32), np.where(take, ae, np.nan)


def one(u, v, gu, gv, occ=None):
    arr = lambda x: np.array([x], F32).reshape(1, -1)  # noqa: E731
    return flow_error_reference(arr(u), arr(v), arr(gu), arr(gv), None if occ is None else arr(occ))


def test_new_entries_are_exported(flow2d):
    lib = flow2d.hip_lib()
    assert hasattr(lib, "flow2d_flow_error_2d") and hasattr(lib, "flow2d_flow_error_workspace_bytes")
    host = flow2d.host_lib()
    for name in ("flow2d_host_read_flo", "flow2d_host_write_flo", "flow2d_host_flow_error"):
        assert hasattr(host, name), name
    assert hasattr(flow2d.Context, "flow_error")
    for name in ("read_flo", "write_flo", "evaluate_flow", "flow_error_metrics"):
        assert callable(getattr(flow2d, name)), name
    assert lib.flow2d_abi_version() == 1  # an addition: the version stays


def test_record_layout_matches_the_header(flow2d, tmp_path):
    """sizeof and every field offset of flow2d_flow_error_stats as a C compiler lays it out, against the ctypes mirror."""
    src = tmp_path / "layout.c"
    fields = ["all.count", "all.above", "all.fl", "all.sum_epe", "all.sum_epe_sq", "all.sum_ae", "all.max_epe", "noc", "occ",
              "invalid_ground_truth", "nonfinite_estimate"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flow2d_c_abi.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(flow2d_flow_error_stats));\n' +
                   "".join('  printf("%%zu\\n", offsetof(flow2d_flow_error_stats, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = flow2d.FlowErrorStats
    want = [ctypes.sizeof(S)]
    for f in fields:
        parts = f.split(".")
        off = getattr(S, parts[0]).offset
        if len(parts) == 2:
            off += getattr(flow2d.FlowErrorClass, parts[1]).offset
        want.append(off)
    assert got == want
    assert got[0] == flow2d.FLOW_ERROR_STATS_BYTES == 256


def test_workspace_query(flow2d):
    q = flow2d.hip_lib().flow2d_flow_error_workspace_bytes
    assert q(0, 5, 1) == 0 and q(5, 0, 1) == 0 and q(5, 5, 0) == 0
    one_block = q(1, 1, 1)
    assert one_block > 0 and one_block % 16 == 0
    assert q(256, 32, 1) == one_block and q(257, 32, 1) == 2 * one_block and q(256, 33, 1) == 2 * one_block
    assert q(4096, 4096, 3) == 3 * q(4096, 4096, 1) == 3 * 16 * 128 * one_block


def test_flow_error_rejects_bad_arguments_without_a_device(flow2d):
    """Every refusal below happens before the context is touched: the context is a zeroed stand-in and the planes are
    16-byte aligned addresses nothing reads."""
    lib = flow2d.hip_lib()
    fake_ctx = ctypes.create_string_buffer(4096)
    ctx = ctypes.addressof(fake_ctx)
    w, h, pitch = 64, 8, 256
    u, v, gu, gv, occ, epe, ae = (0x1000000 * (k + 1) for k in range(7))
    stats, ws = 0x9000000, 0xA000000
    need = lib.flow2d_flow_error_workspace_bytes(w, h, 1)

    def call(ctx=ctx, u=u, v=v, gu=gu, gv=gv, occ=occ, w=w, h=h, pitch=pitch, epe=epe, ae=ae, stats=stats, ws=ws, ws_bytes=need):
        return lib.flow2d_flow_error_2d(ctx, u, v, gu, gv, occ, w, h, pitch, epe, ae, stats, ws, ws_bytes)

    assert call(ctx=None) == 1
    for plane in ("u", "v", "gu", "gv"):
        assert call(**{plane: None}) == 1, plane
        assert call(**{plane: locals()[plane] + 4}) == 1, plane  # misaligned
    assert call(occ=occ + 4) == 1 and call(epe=epe + 4) == 1 and call(ae=ae + 8) == 1
    assert call(w=0) == 1 and call(h=0) == 1
    assert call(pitch=8) == 1 and call(pitch=260) == 1  # narrower than a row; not a multiple of 16
    assert call(stats=None) == 1 and call(stats=stats + 4) == 1
    assert call(ws=None) == 1 and call(ws=ws + 8) == 1 and call(ws_bytes=need - 16) == 1
    # written ranges against read ones and each other: overlapping regions at different base pointers
    assert call(epe=u + pitch) == 1              # starts inside u
    assert call(ae=gv - pitch) == 1              # ends inside gt_v
    assert call(epe=occ + (h - 1) * pitch) == 1  # shares the occlusion plane's last row only
    assert call(ae=epe + pitch) == 1             # the two outputs overlap
    assert call(ae=epe) == 1
    assert call(epe=stats - pitch) == 1 and call(ae=ws - 16) == 1
    assert call(stats=u + 64) == 1 and call(ws=gu + 1024) == 1 and call(stats=ws + 16) == 1
    if flow2d.device_count() == 0:
        # arguments that pass every check reach the device guard: no device here, so a device error -- not a refusal
        assert call() == 3
        assert call(occ=None, epe=None, ae=None) == 3
        assert call(epe=u + h * pitch, ae=u - h * pitch) == 3


def flo_bytes(u, v):
    h, w = u.shape
    body = np.stack([u, v], -1).astype("<f4").tobytes()
    return struct.pack("<fii", 202021.25, w, h) + body


def test_flo_round_trip_is_bit_exact(flow2d, tmp_path):
    rng = np.random.default_rng(0)
    u = rng.normal(0, 30, (7, 13)).astype(F32)
    v = rng.normal(0, 30, (7, 13)).astype(F32)
    u[0, 0], v[1, 1], u[2, 2], v[3, 3] = np.nan, np.inf, 1e10, -0.0  # non-finite, unknown-flow and signed-zero values too
    p = tmp_path / "a.flo"
    flow2d.write_flo(str(p), u, v)
    assert p.read_bytes() == flo_bytes(u, v)  # magic, int32 width, int32 height, interleaved (u, v) row-major
    ru, rv = flow2d.read_flo(str(p))
    assert ru.tobytes() == u.tobytes() and rv.tobytes() == v.tobytes()
    # a file written by other tools: trailing bytes are ignored
    q = tmp_path / "b.flo"
    q.write_bytes(flo_bytes(v, u) + b"\0" * 7)
    ru, rv = flow2d.read_flo(str(q))
    assert ru.tobytes() == v.tobytes() and rv.tobytes() == u.tobytes()
    one_pixel = tmp_path / "c.flo"
    flow2d.write_flo(str(one_pixel), np.full((1, 1), 2.5, F32), np.full((1, 1), -1, F32))
    assert [a.tolist() for a in flow2d.read_flo(str(one_pixel))] == [[[2.5]], [[-1.0]]]


def test_flo_bad_files_are_refused(flow2d, tmp_path):
    u = np.arange(12, dtype=F32).reshape(3, 4)
    good = flo_bytes(u, -u)
    cases = {
        "truncated_body": good[:-1],
        "header_only": good[:12],
        "short_header": good[:10],
        "empty": b"",
        "bad_magic": struct.pack("<fii", 202021.0, 4, 3) + good[12:],
        "text_magic": b"PIEX" + good[4:],
        "zero_width": struct.pack("<fii", 202021.25, 0, 3),
        "zero_height": struct.pack("<fii", 202021.25, 4, 0) + good[12:],
        "negative": struct.pack("<fii", 202021.25, -4, 3) + good[12:],
        "absurd": struct.pack("<fii", 202021.25, 1 << 30, 1 << 30) + good[12:],
        "too_many_pixels": struct.pack("<fii", 202021.25, 1 << 20, 1 << 20) + good[12:],
    }
    for name, data in cases.items():
        p = tmp_path / (name + ".flo")
        p.write_bytes(data)
        with pytest.raises(ValueError):
            flow2d.read_flo(str(p))
    with pytest.raises(ValueError):
        flow2d.read_flo(str(tmp_path / "missing.flo"))
    with pytest.raises(OSError):
        flow2d.write_flo(str(tmp_path / "no_such_dir" / "x.flo"), u, u)


def test_reference_hand_computed_answers():
    rec, epe, ae = one(3, 4, 0, 0)  # a 3-4-5 error
    assert epe[0, 0] == 5 and rec["all"]["sum_epe"] == 5 and rec["all"]["sum_epe_sq"] == 25 and rec["all"]["max_epe"] == 5
    assert rec["all"]["above"] == [1, 1, 1, 1] and rec["all"]["fl"] == 1  # 5 > 3 and 5 > 0.05 * 0
    assert ae[0, 0] == pytest.approx(np.degrees(np.arccos(1 / np.sqrt(26))), abs=1e-12)
    rec, epe, ae = one(1, 0, 0, 1)  # (1, 0, 1) against (0, 1, 1): cos = 1 / 2
    assert ae[0, 0] == pytest.approx(60.0, abs=1e-12) and epe[0, 0] == F32(np.sqrt(F32(2)))
    assert rec["all"]["above"] == [1, 1, 0, 0]
    rec, epe, ae = one(2.5, -1, 2.5, -1)  # exact
    assert epe[0, 0] == 0 and ae[0, 0] == 0 and rec["all"]["above"] == [0, 0, 0, 0]
    # the thresholds are strict: an EPE of exactly 0.5, 1, 2 or 3 is not above it
    u = np.array([[0.5, 1, 2, 3, 3.0000002]], F32)
    rec, _, _ = flow_error_reference(u, 0 * u, 0 * u, 0 * u)
    assert rec["all"]["above"] == [4, 3, 2, 1] and rec["all"]["fl"] == 1
    # KITTI Fl: EPE 4 is above 3 px but not above 5 % of |gt| = 100; it is of |gt| = 50
    rec, _, _ = one(104, 0, 100, 0)
    assert rec["all"]["fl"] == 0 and rec["all"]["above"][3] == 1
    rec, _, _ = one(54, 0, 50, 0)
    assert rec["all"]["fl"] == 1
    # small angles keep their precision (the acos form would give 0 here)
    _, _, ae = one(1e-4, 0, 0, 0)
    assert ae[0, 0] == pytest.approx(np.degrees(np.arctan(float(F32(1e-4)))), rel=1e-12)


def test_reference_classifies_invalid_and_nonfinite_pixels():
    nan, inf = np.nan, np.inf
    gu = np.array([[1e9, F32(1e9) * F32(1.0000001), -1e9, nan, inf, 0, 0, 0, nan]], F32)
    gv = np.array([[0, 0, 0, 0, 0, -inf, 0, 0, 0]], F32)
    u = np.array([[0, 0, 0, 0, 0, 0, nan, inf, nan]], F32)
    v = np.zeros_like(u)
    rec, epe, ae = flow_error_reference(u, v, gu, gv)
    # valid: 1e9, -1e9 (|gt| <= 1e9) and the three zeros; invalid: the float above 1e9, NaN, inf, -inf (in v), NaN with a NaN estimate
    assert rec["invalid_ground_truth"] == 5
    assert rec["nonfinite_estimate"] == 2  # NaN and inf estimates at valid pixels
    assert rec["all"]["count"] == 2 and rec["all"]["sum_epe"] == 2e9
    assert np.isnan(epe).sum() == 7 and np.isnan(ae).sum() == 7
    assert epe[0, 0] == 1e9 and epe[0, 2] == 1e9


def test_reference_infinite_epe_propagates():
    """A finite estimate whose du * du overflows has an infinite EPE: counted, above every threshold, in every sum as inf."""
    u = np.array([[1e30, 1.0]], F32)
    rec, epe, _ = flow_error_reference(u, 0 * u, 0 * u, 0 * u)
    assert np.isinf(epe[0, 0]) and rec["all"]["count"] == 2 and rec["nonfinite_estimate"] == 0
    assert rec["all"]["above"] == [2, 1, 1, 1] and rec["all"]["fl"] == 1
    assert rec["all"]["sum_epe"] == np.inf and rec["all"]["sum_epe_sq"] == np.inf and rec["all"]["max_epe"] == np.inf


def test_reference_occlusion_classes():
    rng = np.random.default_rng(1)
    h, w = 6, 9
    u, v, gu, gv = (rng.normal(0, 2, (h, w)).astype(F32) for _ in range(4))
    occ = np.zeros((h, w), F32)
    occ[1, :4] = 1
    occ[2, 2] = np.nan  # what flow2d_consistency_2d never writes but a ground-truth map may hold: occluded
    occ[3, 3] = -0.0    # == 0: not occluded
    rec, _, _ = flow_error_reference(u, v, gu, gv, occ)
    assert rec["occ"]["count"] == 5 and rec["noc"]["count"] == h * w - 5 and rec["all"]["count"] == h * w
    for key in ("above", "fl"):
        assert np.array_equal(np.add(rec["noc"][key], rec["occ"][key]), rec["all"][key])
    assert rec["noc"]["sum_epe"] + rec["occ"]["sum_epe"] == pytest.approx(rec["all"]["sum_epe"], rel=1e-15)
    assert max(rec["noc"]["max_epe"], rec["occ"]["max_epe"]) == rec["all"]["max_epe"]
    no_mask, _, _ = flow_error_reference(u, v, gu, gv)
    assert no_mask["noc"] == no_mask["all"] and no_mask["occ"]["count"] == 0 and no_mask["occ"]["max_epe"] == 0


def test_metrics_of_a_record(flow2d):
    rec, _, _ = flow_error_reference(np.array([[3, 0, 1]], F32), np.array([[4, 0, 0]], F32), np.zeros((1, 3), F32),
                                     np.zeros((1, 3), F32), np.array([[0, 0, 1]], F32))
    m = flow2d.flow_error_metrics(rec)
    assert m["all"]["epe"] == 2.0 and m["all"]["rmse"] == np.sqrt(26 / 3) and m["all"]["r1"] == 1 / 3
    assert m["noc"]["epe"] == 2.5 and m["noc"]["r0.5"] == 0.5 and m["occ"]["count"] == 1 and m["occ"]["r1"] == 0.0
    empty = flow2d.flow_error_metrics(flow_error_reference(np.zeros((1, 1), F32), *(np.zeros((1, 1), F32),) * 3)[0])
    assert empty["occ"]["epe"] is None and empty["occ"]["fl"] is None and empty["occ"]["max_epe"] == 0


@pytest.mark.parametrize("name", ["translation", "rotation", "zoom", "affine", "two_layer"])
def test_scene_ground_truth_is_exact(name):
    """I1(x + gt(x)) == I0(x) on the non-occluded pixels, with frame 1 evaluated analytically at the displaced points."""
    scenes = importlib.import_module("cuda-flow2d_amd.scenes")
    s = scenes.make_scene(name, 96, 80, seed=3)
    h, w = s.shape
    assert s.frame_0.shape == s.frame_1.shape == s.gt_u.shape == s.gt_v.shape == (80, 96)
    assert all(a.dtype == F32 for a in (s.frame_0, s.frame_1, s.gt_u, s.gt_v))
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    i1 = s.frame_1_at(xs + s.gt_u.astype(np.float64), ys + s.gt_v.astype(np.float64))
    noc = np.ones((h, w), bool) if s.occlusion is None else s.occlusion == 0
    assert np.abs(i1 - s.frame_0)[noc].max() < 1e-4
    assert np.array_equal(s.frame_1, s.frame_1_at(xs, ys).astype(F32))  # frame 1 is the analytic frame sampled
    assert np.abs(np.hypot(s.gt_u, s.gt_v)).max() > 0.5                  # a motion worth measuring
    # the same seed gives the same scene, another seed another texture
    again = scenes.make_scene(name, 96, 80, seed=3)
    assert np.array_equal(again.frame_0, s.frame_0) and np.array_equal(again.gt_u, s.gt_u)
    assert not np.array_equal(scenes.make_scene(name, 96, 80, seed=4).frame_0, s.frame_0)


def test_two_layer_occlusion_map():
    """The occluded pixels are the background the square covers in frame 1 and the square's pixels that leave the frame; they
    really do not match (no analytic counterpart at x + gt(x))."""
    scenes = importlib.import_module("cuda-flow2d_amd.scenes")
    s = scenes.make_scene("two_layer", 128, 96, seed=0)
    h, w = s.shape
    occ = s.occlusion != 0
    moving = (s.gt_u != 0) | (s.gt_v != 0)
    assert occ.sum() > 0 and not (occ & moving).any()  # the square stays inside here: only covered background
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    i1 = s.frame_1_at(xs + s.gt_u, ys + s.gt_v)
    assert np.median(np.abs(i1 - s.frame_0)[occ]) > 1.0
    # a square pushed out of the frame: its leaving pixels are occluded too
    edge = scenes._two_layer_scene(40, 40, scenes.Texture(np.random.default_rng(0)), scenes.Texture(np.random.default_rng(1)),
                                   (30.5, 0.0))
    leaving = (edge.gt_u != 0) & (np.mgrid[0:40, 0:40][1] + 30.5 > 39)
    assert leaving.any() and (edge.occlusion[leaving] == 1).all()
    with pytest.raises(ValueError):
        scenes.make_scene("nonsense")
