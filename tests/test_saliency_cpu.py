"""CPU side of the occlusion-sensitivity maps: the grid rule, the numpy oracle's own properties (tests/_saliency_oracle.py -- the kernels
are compared with it for equality in tests/test_gpu_saliency.py), the C ABI's declarations and refusals, and the script's flags."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _saliency_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_CASES = ((8, 3, 2), (8, 8, 8), (7, 3, 3), (9, 4, 3), (5, 1, 1), (13, 5, 5), (84, 21, 7), (256, 32, 16))
ENTRY_POINTS = ("rpe_occlusion_grid", "rpe_occlude_grid_u8", "rpe_pose_displacement", "rpe_saliency_map", "rpe_saliency_overlay_u8")


def _mu():
    from rgb_proprioceptive_pose_estimator_amd.util import model_utils
    return model_utils


@pytest.mark.parametrize("n,p,s", GRID_CASES)
def test_grid_rule(n, p, s):
    mu = _mu()
    g = -(-(n - p) // s) + 1                                # ceil((n - p) / s) + 1
    for hs, ws in ((n, n), (n, 2 * n + 1)):
        gy, gx, tops, lefts = mu.occlusion_grid(hs, ws, p, s)
        assert (gy, gx, tops, lefts) == so.grid(hs, ws, p, s)
        assert gy == g == len(tops) and gx == len(lefts) == -(-(ws - p) // s) + 1
        assert tops == [min(i * s, hs - p) for i in range(gy)] and lefts == [min(i * s, ws - p) for i in range(gx)]
        assert len(set(tops)) == gy and len(set(lefts)) == gx                      # the origins are distinct ...
        assert tops == sorted(tops) and lefts == sorted(lefts)
        assert tops[0] == 0 and lefts[0] == 0 and tops[-1] + p == hs and lefts[-1] + p == ws     # ... and the clamped last one ends at the edge
        cov = so.coverage(hs, ws, p, s)
        assert cov.min() >= 1                                                      # every pixel is covered
        if hs == ws:
            assert 1 <= np.sqrt(cov.max()) <= 3 and cov.max() == cov[tops[1] if gy > 1 else 0:, :].max()
    # a (y, x) pair on both arguments
    gy, gx, tops, lefts = mu.occlusion_grid(n, n + 3, (p, min(p + 1, n + 3)), (s, 1))
    assert gy == g and lefts == list(range(gx)) and lefts[-1] + min(p + 1, n + 3) == n + 3


def test_grid_refusals_in_words():
    mu = _mu()
    for args, word in (((8, 8, 3, 4), "stride"), ((8, 8, (3, 3), (2, 4)), "stride"), ((8, 8, 9, 1), "rectangle"), ((8, 8, (3, 9), 1), "rectangle"),
                       ((8, 8, 0, 1), "rectangle"), ((8, 8, 3, 0), "stride"), ((8, 8, 3, (1, 0)), "stride"), ((0, 8, 1, 1), "frame"), ((8, 0, 1, 1), "frame"),
                       ((8, 8, -1, 1), "rectangle"), ((8, 8, (3, 3, 3), 1), "pair"), ((32768, 32768, 1, 1), "2^31")):
        with pytest.raises(ValueError, match=re.escape(word)):
            mu.occlusion_grid(*args)


# -- the C ABI ------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_and_bound():
    from rgb_proprioceptive_pose_estimator_amd import _lib, ops
    import rgb_proprioceptive_pose_estimator_amd.torch_ops as T
    header = open(os.path.join(ROOT, "include", "rpe_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS and hasattr(_lib.raw, name), name
    end = header.index("} rpe_occlusion_desc;")
    body = re.sub(r"/\*.*?\*/", "", header[header.rindex("typedef struct {", 0, end):end], flags=re.S)
    declared = [n for n in re.findall(r"\b([A-Za-z_]+)(?=(?:\[\d+\])?[,;])", body)]
    assert declared == [n for n, _ in _lib.OcclusionDesc._fields_] == ["Hs", "Ws", "ph", "pw", "sy", "sx", "fill_rgb"]
    assert ctypes.sizeof(_lib.OcclusionDesc) == 28 and _lib.OcclusionDesc.Hs.offset == 0 and _lib.OcclusionDesc.sx.offset == 20
    assert _lib.OcclusionDesc.fill_rgb.offset == 24 and _lib.OcclusionDesc.fill_rgb.size == 3
    assert ops.OCCLUSION_DESC_FIELDS == ("Hs", "Ws", "ph", "pw", "sy", "sx", "fill_r", "fill_g", "fill_b")
    d = ops.occlusion_desc(7, 5, 3, 2, 3, 1, 1, 2, 3)
    assert (d.Hs, d.Ws, d.ph, d.pw, d.sy, d.sx, list(d.fill_rgb)) == (7, 5, 3, 2, 3, 1, [1, 2, 3])
    with pytest.raises(ValueError):
        ops.occlusion_desc(fill_r=256)
    for name in ("occlude_grid_u8", "pose_displacement", "saliency_map", "saliency_overlay_u8"):
        assert name in T.NAMES and getattr(torch.ops.rpe, name).default._schema.name == "rpe::" + name
    s = torch.ops.rpe.occlude_grid_u8.default._schema
    assert [a.name for a in s.arguments] == ["frame", "desc", "B", "k0"] and not any(a.alias_info is not None for a in s.arguments)
    assert [a.name for a in torch.ops.rpe.saliency_overlay_u8.default._schema.arguments] == ["frame", "smap", "minmax", "table", "alpha_q8", "fade"]
    with pytest.raises(NotImplementedError):     # the HIP key only: no CPU kernel to fall back to
        torch.ops.rpe.pose_displacement(torch.zeros(3, 7), torch.zeros(7))
    with pytest.raises(NotImplementedError):
        torch.ops.rpe.occlude_grid_u8(torch.zeros(8, 8, 3, dtype=torch.uint8), [8, 8, 3, 3, 2, 2, 0, 0, 0], 3, 0)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        desc = [7, 5, 3, 2, 3, 1, 124, 116, 104]                                  # Gy, Gx = 3, 4
        frame = torch.empty(7, 5, 3, dtype=torch.uint8, device="cuda")
        out = torch.ops.rpe.occlude_grid_u8(frame, desc, 6, 4)
        assert out.shape == (6, 7, 5, 3) and out.dtype == torch.uint8
        pos, ori = torch.ops.rpe.pose_displacement(torch.empty(2, 6, 7, device="cuda"), torch.empty(7, device="cuda"))
        assert pos.shape == ori.shape == (2, 6) and pos.dtype == ori.dtype == torch.float32
        maps, mm = torch.ops.rpe.saliency_map(torch.empty(2, 12, device="cuda"), desc)
        assert maps.shape == (2, 7, 5) and mm.shape == (2, 2) and maps.dtype == mm.dtype == torch.float32
        maps3, _ = torch.ops.rpe.saliency_map(torch.empty(2, 3, 4, device="cuda"), desc)
        assert maps3.shape == (2, 7, 5)
        pic = torch.ops.rpe.saliency_overlay_u8(frame, maps[0], mm[0], torch.empty(256, 3, dtype=torch.uint8, device="cuda"), 128, True)
        assert pic.shape == (7, 5, 3) and pic.dtype == torch.uint8


def test_rejected_arguments_need_no_device():
    """bad arguments come back as a status before anything is launched"""
    from rgb_proprioceptive_pose_estimator_amd import ops
    from rgb_proprioceptive_pose_estimator_amd._lib import raw
    one = ctypes.c_void_p(16)   # never dereferenced: every call below is refused
    good = dict(Hs=8, Ws=10, ph=3, pw=4, sy=2, sx=3)
    bad_descs = (dict(Hs=0), dict(Ws=0), dict(Hs=-4), dict(ph=0), dict(pw=0), dict(ph=9), dict(pw=11), dict(sy=4), dict(sx=5), dict(sy=0), dict(sx=0),
                 dict(sy=-1), dict(Hs=32768, Ws=32768), dict(Hs=26755, Ws=26755))       # 26755^2 * 3 >= 2^31 > 26754^2 * 3
    ref = lambda d: ctypes.byref(d) if d is not None else None

    # rpe_occlusion_grid: K, or -1
    gy, gx = ctypes.c_int(-7), ctypes.c_int(-7)
    assert raw.rpe_occlusion_grid(ref(ops.occlusion_desc(**good)), ctypes.byref(gy), ctypes.byref(gx)) == 12 and (gy.value, gx.value) == (4, 3)
    assert raw.rpe_occlusion_grid(ref(ops.occlusion_desc(256, 256, 32, 32, 16, 16)), None, None) == 225
    assert raw.rpe_occlusion_grid(ref(ops.occlusion_desc(26754, 26754, 1, 1, 1, 1)), None, None) == 26754 ** 2
    for kw in bad_descs:
        assert raw.rpe_occlusion_grid(ref(ops.occlusion_desc(**dict(good, **kw))), ctypes.byref(gy), ctypes.byref(gx)) == -1, kw
        assert b"occlusion_grid" in raw.rpe_last_error()
    assert raw.rpe_occlusion_grid(None, None, None) == -1 and (gy.value, gx.value) == (4, 3)
    for kw in bad_descs:
        with pytest.raises(ValueError, match="occlusion_grid"):
            ops.occlusion_grid(ops.occlusion_desc(**dict(good, **kw)))

    occ = lambda d, frame=one, out=one, b=4, k0=0: raw.rpe_occlude_grid_u8(frame, out, b, k0, ref(d), None)
    d = ops.occlusion_desc(**good)
    for kw in bad_descs:
        assert occ(ops.occlusion_desc(**dict(good, **kw))) == 1, kw      # RPE_ERR_SHAPE
    assert occ(None) == 1 and occ(d, frame=None) == 1 and occ(d, out=None) == 1 and occ(d, b=0) == 1 and occ(d, b=-3) == 1 and occ(d, k0=-1) == 1
    assert b"occlude_grid_u8" in raw.rpe_last_error()

    disp = lambda pred=one, r=one, n=5, pos=one, ori=one: raw.rpe_pose_displacement(pred, r, n, pos, ori, None)
    assert disp(pred=None) == 1 and disp(r=None) == 1 and disp(pos=None) == 1 and disp(ori=None) == 1 and disp(n=0) == 1 and disp(n=-2) == 1
    assert b"pose_displacement" in raw.rpe_last_error()

    smap = lambda d, scores=one, m=2, maps=one, mm=one: raw.rpe_saliency_map(scores, m, ref(d), maps, mm, None)
    for kw in bad_descs:
        assert smap(ops.occlusion_desc(**dict(good, **kw))) == 1, kw
    assert smap(None) == 1 and smap(d, scores=None) == 1 and smap(d, maps=None) == 1 and smap(d, mm=None) == 1 and smap(d, m=0) == 1 and smap(d, m=-1) == 1
    assert b"saliency_map" in raw.rpe_last_error()

    over = lambda frame=one, m=one, mm=one, table=one, hs=8, ws=10, a=128, fade=0, out=one: raw.rpe_saliency_overlay_u8(frame, m, mm, table, hs, ws, a, fade, out, None)
    assert over(frame=None) == 1 and over(m=None) == 1 and over(mm=None) == 1 and over(table=None) == 1 and over(out=None) == 1
    assert over(hs=0) == 1 and over(ws=0) == 1 and over(hs=-1) == 1 and over(a=-1) == 1 and over(a=257) == 1 and over(hs=32768, ws=32768) == 1
    assert over(hs=26755, ws=26755) == 1
    assert b"saliency_overlay_u8" in raw.rpe_last_error()


# -- the oracle's own properties ------------------------------------------------------------------------------------------------

def test_oracle_occluded_batch_layout():
    rng = np.random.default_rng(0)
    frame = rng.integers(0, 256, (7, 5, 3), dtype=np.uint8)
    patch, stride, fill = (3, 2), (3, 1), (9, 8, 7)
    rects = so.rectangles(7, 5, patch, stride)
    assert len(rects) == 12 and rects[0] == (0, 0) and rects[5] == (3, 1) and rects[-1] == (4, 3)
    out = so.occluded_batch(frame, patch, stride, fill, 6, 9)         # rectangles 9, 10, 11, then two padding rows
    assert out.shape == (6, 7, 5, 3) and np.array_equal(out[0], frame) and np.array_equal(out[4], frame) and np.array_equal(out[5], frame)
    for r, k in ((1, 9), (2, 10), (3, 11)):
        t, l = rects[k]
        changed = np.zeros((7, 5), dtype=bool)
        changed[t:t + 3, l:l + 2] = True
        assert np.array_equal(out[r][changed], np.tile(np.uint8(fill), (6, 1))) and np.array_equal(out[r][~changed], frame[~changed])


def test_oracle_map_properties():
    # K = 1: a constant map equal to the score
    maps, mm = so.saliency_map(np.float32([[0.37], [-2.5]]), 8, 8, 8, 8)
    assert np.array_equal(maps[0], np.full((8, 8), np.float32(0.37))) and np.array_equal(maps[1], np.full((8, 8), np.float32(-2.5)))
    assert mm.tolist() == [[np.float32(0.37)] * 2, [-2.5, -2.5]]
    # a NaN score poisons exactly its rectangle's pixels
    rng = np.random.default_rng(1)
    hs, ws, p, s = 9, 9, 4, 3
    rects = so.rectangles(hs, ws, p, s)
    scores = rng.random((1, len(rects)), dtype=np.float32)
    clean, _ = so.saliency_map(scores, hs, ws, p, s)
    scores[0, 4] = np.nan
    maps, mm = so.saliency_map(scores, hs, ws, p, s)
    t, l = rects[4]
    inside = np.zeros((hs, ws), dtype=bool)
    inside[t:t + p, l:l + p] = True
    assert np.array_equal(np.isnan(maps[0]), inside) and np.array_equal(maps[0][~inside], clean[0][~inside])
    assert mm[0, 0] == maps[0][~inside].min() and mm[0, 1] == maps[0][~inside].max()
    # the stated order: ascending k, one fp32 rounding per add, one for the division
    a, b, c = np.float32(1e8), np.float32(1.0), np.float32(-1e8)
    one_d, _ = so.saliency_map(np.float32([[a, b, c]]), 1, 5, (1, 3), (1, 1))      # pixel 2 is under all three
    assert one_d[0, 0, 2] == np.float32(np.float32(np.float32(a + b) + c) / np.float32(3)) == 0.0
    assert one_d[0, 0, 0] == a and one_d[0, 0, 1] == np.float32(np.float32(a + b) / np.float32(2)) and one_d[0, 0, 4] == c
    # no finite value: (+inf, -inf)
    _, mm = so.saliency_map(np.full((1, 4), np.nan, dtype=np.float32), 4, 4, 2, 2)
    assert mm.tolist() == [[np.inf, -np.inf]]


def test_oracle_overlay_properties():
    rng = np.random.default_rng(2)
    frame = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)
    table = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    smap = rng.random((6, 7), dtype=np.float32)
    lo, hi = smap.min(), smap.max()
    k = np.minimum(255, ((smap - lo) / (hi - lo) * np.float32(256)).astype(np.int64))
    assert k.min() == 0 and k.max() == 255
    for fade in (False, True):
        assert np.array_equal(so.overlay(frame, smap, lo, hi, table, 0, fade), frame)           # alpha = 0: the frame
    assert np.array_equal(so.overlay(frame, smap, lo, hi, table, 256, False), table[k])          # alpha = 1: the table's colour
    faded = so.overlay(frame, smap, lo, hi, table, 256, True)
    assert np.array_equal(faded[k == 0], frame[k == 0])                                          # fade: weight 0 at the map's minimum
    half = so.overlay(frame, smap, lo, hi, table, 128, False)
    assert np.array_equal(half, ((frame.astype(np.int64) + table[k].astype(np.int64)) * 128 + 128 >> 8).astype(np.uint8))
    assert np.array_equal(so.overlay(frame, smap, lo, lo, table, 256, False), np.broadcast_to(table[0], frame.shape))   # hi == lo: index 0
    holes = smap.copy()
    holes[1, 2], holes[3, 3], holes[5, 6] = np.nan, np.inf, -np.inf
    got = so.overlay(frame, holes, lo, hi, table, 256, False)
    bad = ~np.isfinite(holes)
    assert np.array_equal(got[bad], frame[bad]) and np.array_equal(got[~bad], table[k][~bad])     # a non-finite value shows the frame


def test_oracle_displacement():
    q = np.float32([0.1, -0.2, 0.3, 0.9])
    ref = np.concatenate([np.float32([1, 2, 3]), q])
    pred = np.stack([ref, np.concatenate([ref[:3], -q]), np.concatenate([ref[:3] + np.float32([3, 4, 0]), 4 * q]),
                     np.concatenate([ref[:3], np.float32([0.9, -0.3, -0.2, -0.1])]), np.concatenate([ref[:3], np.zeros(4, np.float32)])])
    pos, ori = so.pose_displacement(pred, ref)
    assert pos.tolist() == [0, 0, 5, 0, 0] and ori[:3].tolist() == [0, 0, 0]
    assert ori[3] == np.float32(np.pi) and np.isnan(ori[4])                # <q, q'> = 0: half a turn; a zero quaternion: NaN in ori only
    # (row 2: a quaternion scaled by a power of two normalises to the same bits)
    # against 2 acos |<a, b>| where that is well conditioned
    rng = np.random.default_rng(3)
    a, b = rng.normal(size=(2, 64, 4))
    a, b = a / np.linalg.norm(a, axis=1, keepdims=True), b / np.linalg.norm(b, axis=1, keepdims=True)
    _, ori = so.pose_displacement(np.concatenate([np.zeros((64, 3)), a], 1), np.concatenate([np.zeros(3), b[0]]))
    want = 2 * np.arccos(np.abs(a.astype(np.float32).astype(np.float64) @ b[0].astype(np.float32).astype(np.float64)).clip(0, 1))
    assert np.allclose(ori, want, rtol=0, atol=1e-5)


# -- the script -----------------------------------------------------------------------------------------------------------------

def test_script_flags():
    from rgb_proprioceptive_pose_estimator_amd.scripts import visualize_features as vf
    p = vf.build_vis_parser()
    args = p.parse_args([])
    assert args.saliency is None and args.patch == [32] and args.stride == [16] and args.saliency_alpha == 0.5 and args.saliency_fade is False
    assert args.measurements is None and args.truth is None and vf.build_saliency(args) is None
    args = p.parse_args(["--frames", "f.npy", "--saliency", "both", "--patch", "16", "--stride", "8", "4", "--saliency_alpha", "0.25", "--saliency_fade",
                         "--measurements", "m.npy", "--truth", "t.npy", "--out", "x"])
    assert args.saliency == "both" and args.patch == [16] and args.stride == [8, 4] and args.measurements == "m.npy" and args.truth == "t.npy"
    assert vf.build_saliency(args) == dict(kinds=("position", "orientation"), patch=16, stride=(8, 4), alpha=0.25, fade=True)
    assert vf.build_saliency(p.parse_args(["--frames", "f.npy", "--saliency", "orientation"]))["kinds"] == ("orientation",)
    with pytest.raises(SystemExit):
        p.parse_args(["--saliency", "everything"])
    for flags in (["--saliency", "position", "--frames", "f.npy", "--patch", "1", "2", "3"], ["--saliency", "position", "--frames", "f.npy", "--saliency_alpha", "1.5"],
                  ["--truth", "t.npy"], ["--measurements", "m.npy"]):
        with pytest.raises(SystemExit):
            vf.build_saliency(p.parse_args(flags))


def test_saliency_without_frames_exits_before_any_device_use(monkeypatch):
    from rgb_proprioceptive_pose_estimator_amd.scripts import visualize_features as vf

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(vf, "build_model", no_device)
    with pytest.raises(SystemExit, match="--saliency needs --frames"):
        vf.main(["--model", "no", "--obj_name", "cube", "--saliency", "both"])
