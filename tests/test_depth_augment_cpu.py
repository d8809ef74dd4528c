"""CPU side of the depth augmentation: the numpy oracle (tests/_depth_augment_oracle.py) against known answers, a scalar restatement
in plain Python floats and the specification's properties -- the kernel is compared with the oracle for equality in
tests/test_gpu_depth_augment.py, so statistics are checked here, once -- and the host logic of DepthAugment, train() and
scripts/train_model.py."""
import ctypes
import inspect
import math
import os
import re
import struct
import types

import numpy as np
import pytest
import torch

import _augment_oracle as ao
import _depth_augment_oracle as do

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = 2 ** 32 - 1
T_STD = math.sqrt(2.0 * (2 ** 32 - 1))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _f32(v):
    """a Python float rounded to fp32 (round to nearest even, overflow to inf), as its bit pattern"""
    try:
        return struct.unpack("<I", struct.pack("<f", v))[0]
    except OverflowError:
        return 0x7F800000 if v > 0 else 0xFF800000


def _small():
    """one 3 x 4 frame with the special values of the specification in it"""
    d = np.array([[0.0, -0.0, 1e-45, 1.0], [np.nan, np.inf, -np.inf, 2.5], [0.3, 7.75, 9.999, 10.0]], dtype=np.float32)
    return d.reshape(1, 3, 4, 1)


def test_purposes_are_new_and_T_has_the_stated_variance():
    assert len({0, 1, 2, 0x53414D50, 0x4D45414B, 0x4D454153, do.PURPOSE_COUNT, do.PURPOSE_RECT, do.PURPOSE_PIXEL}) == 9
    assert (do.PURPOSE_COUNT, do.PURPOSE_RECT, do.PURPOSE_PIXEL) == (0x44455048, 0x44455052, 0x44455058)
    # Var T = 4 * 6 * (65536^2 - 1) / 12, exactly
    assert 4 * 6 * (65536 ** 2 - 1) // 12 == 2 * (2 ** 32 - 1) and do.T_STD == T_STD
    assert do.sigma_to_n(1.0, 0.5) == (1.0 / T_STD, 0.5 / T_STD)
    # the extremes of T: all halves 0 / all halves 65535
    z, o = [np.uint64(0)] * 4, [np.uint64(FULL)] * 4
    assert int(do.noise_T(z)) == -6 * 65535 and int(do.noise_T(o)) == 6 * 65535


def test_known_answers_for_one_small_frame():
    """every stage against plain Python double arithmetic on the Philox words, pixel by pixel, and three literal bit patterns"""
    depth = _small()
    n0, n1, n2 = do.sigma_to_n(0.01, 0.02, 0.003)
    desc = do.neutral_desc(seed=0x0123456789ABCDEF, n0=n0, n1=n1, n2=n2, q=0.0078125, inv_q=128.0, lo=0.25, hi=9.5, drop_thresh=1 << 30, hole_value=-1.0)
    step = 7
    out, params = do.augment(depth, desc, step)
    assert params[0] == 7 and params.shape == (1 + 17,)
    got = _bits(out).reshape(-1)
    flat = depth.reshape(-1)
    key = (0x89ABCDEF, 0x01234567)
    dropped = 0
    for p in range(12):
        r = [int(w) for w in ao.philox4x32((p, 0, step, 0x44455058), key)]
        T = 2 * sum((w & 0xFFFF) + (w >> 16) for w in r[:3]) - 6 * 65535
        d = float(flat[p])
        if math.isfinite(d):
            sd = (n0 + n1 * d) + (n2 * d) * d
            v = d + sd * float(T)
            v = float(np.rint(v * 128.0)) * 0.0078125
            v = 0.25 if v < 0.25 else v
            v = 9.5 if v > 9.5 else v
            want = _f32(v)
        else:
            want = int(_bits(flat[p:p + 1])[0])
        if r[3] < (1 << 30):
            want, dropped = _f32(-1.0), dropped + 1
        assert int(got[p]) == want, (p, hex(int(got[p])), hex(want))
    assert 0 < dropped < 12
    # the noise alone on 1.0, 2.5 and 10.0 (literal bit patterns, recorded from this oracle and the scalar form above)
    alone, _ = do.augment(depth, do.neutral_desc(seed=1, n0=n0, n1=n1, n2=n2), 0)
    assert [hex(int(w)) for w in _bits(alone).reshape(-1)[[3, 7, 11]]] == KNOWN_NOISE_BITS


KNOWN_NOISE_BITS = ["0x3f81f041", "0x40226cf8", "0x411c8ed0"]      # 1.0151445, 2.537901, 9.784866


def test_neutral_descriptor_returns_the_input_bits():
    depth = _small()
    assert np.signbit(depth.reshape(-1)[1]) and depth.reshape(-1)[2] > 0 and depth.reshape(-1)[2] < 1e-38      # -0.0 and a denormal are in
    out, params = do.augment(depth, do.neutral_desc(seed=5), 11)
    assert np.array_equal(_bits(out), _bits(depth)) and params[0] == 11
    # a NaN with a payload keeps it, also when stages 1-3 run
    odd = np.array([0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000], dtype=np.uint32).view(np.float32).reshape(1, 2, 2, 1)
    out, _ = do.augment(odd, do.neutral_desc(seed=5, n0=1e-6, q=0.5, inv_q=2.0, lo=0.0, hi=1.0), 11)
    assert np.array_equal(_bits(out), _bits(odd))
    # both layouts are the same memory
    a, _ = do.augment(depth, do.neutral_desc(seed=5, n0=1e-6, drop_thresh=1 << 31), 2)
    b, _ = do.augment(depth.reshape(1, 1, 3, 4), do.neutral_desc(seed=5, n0=1e-6, drop_thresh=1 << 31), 2)
    assert b.shape == (1, 1, 3, 4) and np.array_equal(_bits(a).reshape(-1), _bits(b).reshape(-1))


def test_quantisation_clamp_and_signed_zero():
    d = np.array([0.1249, 0.125, 0.375, -0.01, -0.0, 3.3, 1e-45, 0.0], dtype=np.float32).reshape(1, 2, 4, 1)
    out, _ = do.augment(d, do.neutral_desc(q=0.25, inv_q=4.0), 0)
    # round half even: 0.125 * 4 = 0.5 -> 0, 0.375 * 4 = 1.5 -> 2; -0.01 -> -0.0
    assert out.reshape(-1).tolist() == [0.0, 0.0, 0.5, -0.0, -0.0, 3.25, 0.0, 0.0]
    assert np.signbit(out.reshape(-1)[3]) and np.signbit(out.reshape(-1)[4])
    out, _ = do.augment(d, do.neutral_desc(lo=0.0, hi=3.0), 0)
    assert out.reshape(-1).tolist()[:6] == [np.float32(0.1249), 0.125, 0.375, 0.0, -0.0, 3.0]
    assert np.signbit(out.reshape(-1)[4]) and not np.signbit(out.reshape(-1)[3])      # -0.0 < 0.0 is false: it is not replaced
    assert _bits(out).reshape(-1)[6] == 1                                              # the denormal survives the trip through double


def test_stage_order_later_stages_win():
    depth = np.full((1, 8, 8, 1), 2.0, dtype=np.float32)
    rgb = ao.neutral_desc(seed=3, erase_thresh=FULL, eh_lo=8, eh_hi=8, ew_lo=8, ew_hi=8)         # the whole frame is the occluder
    rgb_params = ao.params_table(rgb, 1, 8, 8, 4)
    assert rgb_params[1 + 3] == 1
    desc = do.neutral_desc(seed=3, drop_thresh=FULL, hole_lo=4, hole_hi=4, hh_lo=8, hh_hi=8, hw_lo=8, hw_hi=8, hole_value=-1.0, occluder_value=5.0,
                           n0=1e-7, q=0.5, inv_q=2.0, lo=0.0, hi=1.0)
    dropped, _ = do.augment(depth, dict(desc, hole_hi=0, hole_lo=0), 4)
    assert (dropped == -1.0).sum() >= 63                             # dropout beats the clamp's 1.0
    holes, _ = do.augment(depth, dict(desc, drop_thresh=0), 4)
    assert (holes == -1.0).all()                                     # a hole beats stages 1-3
    both, _ = do.augment(depth, desc, 4, rgb_params=rgb_params)
    assert (both == 5.0).all()                                       # dropped AND in a hole AND occluded: the occluder's value
    # a stream that does not erase leaves the depth alone
    off = ao.params_table(dict(rgb, erase_thresh=0), 1, 8, 8, 4)
    assert np.array_equal(do.augment(depth, desc, 4, rgb_params=off)[0], do.augment(depth, desc, 4)[0])


def test_holes_rectangles_and_grouping():
    depth = np.arange(6 * 16 * 24, dtype=np.float32).reshape(3, 2, 16, 24, 1) + 1.0
    desc = do.neutral_desc(seed=9, hole_lo=1, hole_hi=4, hh_lo=2, hh_hi=6, hw_lo=3, hw_hi=9, hole_value=0.0)
    out, params = do.augment(depth, desc, 2)
    assert params.shape == (1 + 17 * 6,)
    flat = out.reshape(6, 16, 24)
    for b in range(6):
        row = params[1 + 17 * b:1 + 17 * (b + 1)]
        mask = np.zeros((16, 24), bool)
        assert 1 <= row[0] <= 4
        for j in range(4):
            top, left, h, w = row[1 + 4 * j:5 + 4 * j]
            assert 2 <= h <= 6 and 3 <= w <= 9 and 0 <= top <= 16 - h and 0 <= left <= 24 - w     # all four are drawn and tabled
            if j < row[0]:
                mask[top:top + h, left:left + w] = True
        assert (flat[b][mask] == 0.0).all() and np.array_equal(flat[b][~mask], depth.reshape(6, 16, 24)[b][~mask])
    # group = N: the frames of a window share their holes; noise and dropout stay per frame
    g, pg = do.augment(depth, dict(desc, group=2), 2)
    assert pg.shape == (1 + 17 * 2,) and np.array_equal(pg, params[:35])
    zero = (g.reshape(3, 2, 16, 24) == 0.0)
    assert np.array_equal(zero[0], zero[1]) and np.array_equal(zero[0], zero[2]) and not np.array_equal(zero[:, 0], zero[:, 1])
    same = np.ones_like(depth)
    n, _ = do.augment(same, do.neutral_desc(seed=9, n0=1e-6, drop_thresh=1 << 30, group=2, hole_value=0.0), 2)
    assert not np.array_equal(n[0], n[1])
    # determinism; another step and another seed differ
    assert np.array_equal(do.augment(depth, desc, 2)[0], out)
    assert not np.array_equal(do.augment(depth, desc, 3)[1][1:], params[1:]) and not np.array_equal(do.augment(depth, dict(desc, seed=10), 2)[1], params)


def test_one_seed_gives_draws_independent_of_the_rgb_augmentation():
    """the same seed and step: the depth rectangle words come from other counters than the RGB ones"""
    rgb = ao.stream_params(ao.neutral_desc(seed=4, erase_thresh=FULL, eh_lo=1, eh_hi=32, ew_lo=1, ew_hi=32), 64, 32, 32, 1)
    dep = do.stream_params(do.neutral_desc(seed=4, hole_lo=1, hole_hi=1, hh_lo=1, hh_hi=32, hw_lo=1, hw_hi=32), 64, 32, 32, 1)
    assert not np.array_equal(rgb["h"], dep["h"][:, 0]) and not np.array_equal(rgb["top"], dep["top"][:, 0])


def test_statistics_of_the_draws():
    """n = 65536 pixels (one 256 x 256 frame) for T and the dropout, 4096 streams for the hole count; every bound is five standard
    errors of its estimator at that sample size"""
    n = 65536
    desc = do.neutral_desc(seed=0xC0FFEE, drop_thresh=1 << 30)
    r = do.pixel_words(desc, 1, 256, 256, 5)
    T = do.noise_T(r).astype(np.float64).reshape(-1)
    assert T.size == n
    assert abs(T.mean()) <= 5.0 * T_STD / math.sqrt(n), T.mean()                           # standard error of the mean: sigma / sqrt(n)
    assert abs(T.std() - T_STD) <= 5.0 * T_STD / math.sqrt(2 * n), T.std()                 # of the standard deviation: sigma / sqrt(2 n)
    p = (1 << 30) / 2.0 ** 32
    frac = float((r[3] < np.uint64(1 << 30)).mean())
    assert abs(frac - p) <= 5.0 * math.sqrt(p * (1 - p) / n), frac                          # of a fraction: sqrt(p (1 - p) / n)
    out, _ = do.augment(np.ones((1, 256, 256, 1), np.float32), dict(desc, hole_value=0.0), 5)
    assert float((out == 0.0).mean()) == frac                                               # the oracle's dropout is that word test
    g = 4096
    count = do.stream_params(do.neutral_desc(seed=0xC0FFEE, hole_lo=0, hole_hi=4), g, 64, 64, 5)["count"]
    assert count.min() == 0 and count.max() == 4
    for k in range(5):
        f = float((count == k).mean())
        assert abs(f - 0.2) <= 5.0 * math.sqrt(0.2 * 0.8 / g), (k, f)                       # each of the five values: p = 1 / 5, n = 4096
    # the noise stage's standard deviation follows the range model: sigma(d) = s0 + s1 d + s2 d^2 at d = 2
    n0, n1, n2 = do.sigma_to_n(0.01, 0.02, 0.005)
    noisy, _ = do.augment(np.full((1, 256, 256, 1), 2.0, np.float32), do.neutral_desc(seed=0xC0FFEE, n0=n0, n1=n1, n2=n2), 5)
    sd = 0.01 + 0.02 * 2 + 0.005 * 4
    e = noisy.astype(np.float64).reshape(-1) - 2.0
    # (the fp32 store adds a rounding error of at most 2^-23 per sample: 1.2e-7 beside a bound of 1e-3)
    assert abs(e.mean()) <= 5.0 * sd / math.sqrt(n) + 2.0 ** -23 and abs(e.std() - sd) <= 5.0 * sd / math.sqrt(2 * n) + 2.0 ** -23


# -- host logic -------------------------------------------------------------------------------------------------------------------

def _da():
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import DepthAugment
    return DepthAugment


def test_entry_point_is_declared_and_bound():
    from rgb_proprioceptive_pose_estimator_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "rpe_hip.h")).read()
    assert re.search(r"\brpe_augment_depth_f32\s*\(", header) and "rpe_augment_depth_f32" in _lib.EXPORTS and hasattr(_lib.raw, "rpe_augment_depth_f32")
    assert _lib.ABI_VERSION == 3 and re.search(r"#define\s+RPE_ABI_VERSION\s+3\b", header)
    names = [n for n, _ in _lib.DepthAugmentDesc._fields_]
    start = header.index("} rpe_measure_desc;")
    body = header[header.index("unsigned long long seed;", start):header.index("} rpe_depth_augment_desc;")]
    assert [n for n in re.findall(r"\b([a-z_0-9]+)(?=[,;\[])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))] == names
    assert tuple(names) == ops.DEPTH_AUGMENT_DESC_FIELDS
    assert ctypes.sizeof(_lib.DepthAugmentDesc) == 104 and _lib.DepthAugmentDesc.drop_thresh.offset == 64 and _lib.DepthAugmentDesc.group.offset == 100
    # no new environment switch
    src = open(os.path.join(ROOT, "rgb-proprioceptive-pose-estimator_amd", "csrc", "depth_augment.hip")).read()
    assert "getenv" not in src and "RPE_" not in src.replace("RPE_ERR_", "").replace("RPE_CHECK_LAUNCH", "")


def test_refused_descriptors_need_no_device():
    """bad arguments come back as a status before anything is launched"""
    from rgb_proprioceptive_pose_estimator_amd import ops
    from rgb_proprioceptive_pose_estimator_amd._lib import raw
    one = ctypes.c_void_p(16)   # never dereferenced: every call below is refused
    call = lambda d, b=1, hs=8, ws=8, inp=one, out=one, rgb=None, rgb_group=0: raw.rpe_augment_depth_f32(inp, out, b, hs, ws, ctypes.byref(d), one, one, rgb,
                                                                                                         rgb_group, None)
    for kw in REFUSED:
        assert call(ops.depth_augment_desc(**kw)) == 1, kw      # RPE_ERR_SHAPE
        assert raw.rpe_last_error().startswith(b"augment_depth_f32:")
    good = ops.depth_augment_desc()
    assert call(good, b=0) == 1 and call(good, hs=0) == 1 and call(good, hs=1 << 16, ws=1 << 16) == 1 and call(good, inp=None) == 1
    assert call(ops.depth_augment_desc(group=2), rgb=one, rgb_group=0) == 1 and b"group" in raw.rpe_last_error()
    assert call(good, inp=ctypes.c_void_p(1 << 20), out=ctypes.c_void_p((1 << 20) + 64)) == 1 and b"overlap" in raw.rpe_last_error()
    # rectangle bounds are not looked at while hole_hi == 0
    with pytest.raises(ValueError):
        ops.depth_augment_desc(drop_thresh=2 ** 32)


INF, NAN = float("inf"), float("nan")
REFUSED = (dict(n0=-1e-9), dict(n1=INF), dict(n2=NAN), dict(q=-1.0), dict(q=INF), dict(inv_q=NAN), dict(inv_q=-2.0), dict(lo=1.0, hi=0.5), dict(lo=NAN),
           dict(hi=NAN), dict(hole_lo=2, hole_hi=1), dict(hole_hi=5), dict(hole_lo=-1, hole_hi=1), dict(hole_hi=1, hh_lo=0), dict(hole_hi=1, hh_hi=9),
           dict(hole_hi=1, hw_lo=3, hw_hi=2), dict(hole_hi=1, hw_hi=9), dict(group=-1))


def test_depth_augment_conversion_and_validation():
    DA = _da()
    a = DA(noise=(0.001, 0.02, 0.003), drop_prob=0.25, holes=(1, 3), hole_scale=(0.1, 0.3), hole_value=-1.0, quant=0.01, clamp=(0.0, 1.0), occluder_value=0.5,
           seed=5)
    assert a.n == (0.001 / T_STD, 0.02 / T_STD, 0.003 / T_STD) and a.drop_thresh == 1 << 30
    f = a.desc_fields(64, 100, group=4)
    assert (f["n0"], f["n1"], f["n2"]) == a.n and f["q"] == 0.01 and f["inv_q"] == 1.0 / 0.01 and (f["lo"], f["hi"]) == (0.0, 1.0)
    assert (f["hh_lo"], f["hh_hi"], f["hw_lo"], f["hw_hi"], f["group"], f["seed"]) == (6, 19, 10, 30, 4, 5)
    assert (f["hole_lo"], f["hole_hi"], f["hole_value"], f["occluder_value"], f["drop_thresh"]) == (1, 3, -1.0, 0.5, 1 << 30)
    off = DA()
    assert off.desc_fields(8, 8) == do.neutral_desc(hh_lo=1, hh_hi=1, hw_lo=1, hw_hi=1) and off.share_erase is None and off.per_frame is False
    assert DA(noise=0.5).noise == (0.5, 0.0, 0.0) and DA(noise=(0.1, 0.2)).noise == (0.1, 0.2, 0.0)
    assert DA(drop_prob=1.0).drop_thresh == FULL and DA(hole_scale=(0.01, 0.02)).hole_bounds(5) == (1, 1) and DA(hole_scale=(1.0, 1.0)).hole_bounds(7) == (7, 7)
    assert DA().group_of((3, 2, 8, 8, 1)) == 2 and DA(per_frame=True).group_of((3, 2, 8, 8, 1)) == 0 and DA().group_of((6, 8, 8, 1)) == 0
    for kw in (dict(noise=(-0.1,)), dict(noise=(0.1, 0.2, 0.3, 0.4)), dict(noise=()), dict(noise=(NAN,)), dict(noise=(INF,)), dict(drop_prob=-0.1),
               dict(drop_prob=1.5), dict(holes=(2, 1)), dict(holes=(0, 5)), dict(holes=(-1, 1)), dict(holes=3), dict(hole_scale=(0.0, 0.3)),
               dict(hole_scale=(0.4, 0.3)), dict(hole_scale=(0.1, 1.1)), dict(quant=-1.0), dict(quant=INF), dict(quant=NAN), dict(quant=1e-320),
               dict(clamp=(1.0, 0.0)), dict(clamp=(NAN, 1.0)), dict(seed=-1), dict(seed=2 ** 64), dict(share_erase="yes")):
        with pytest.raises(ValueError):
            DA(**kw)
    for bad in (torch.zeros(2, 8, 8, 1, dtype=torch.float64), torch.zeros(2, 8, 8, 1), torch.zeros(8, 8, 1), torch.zeros(2, 8, 8, 3),
                torch.zeros(2, 8, 8, 2)[..., :1], np.zeros((2, 8, 8, 1), np.float32)):              # wrong dtype; host frames; shapes; strided; numpy
        with pytest.raises(ValueError):
            a(bad)


def test_share_erase_checks_geometry_and_grouping():
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import FrameAugment
    DA = _da()
    fa = FrameAugment(erase_prob=1.0)
    a = DA(share_erase=fa)
    with pytest.raises(ValueError, match="has not run"):
        a.shared_table(8, 8, 6, 2)
    fa.last_params, fa.last_geometry = torch.zeros(17, dtype=torch.int32), (8, 8, 6, 2)      # what a call on (3, 2, 8, 8, 3) frames leaves
    table, group = a.shared_table(8, 8, 6, 2)
    assert table is fa.last_params and group == 2
    for other in ((8, 9, 6, 2), (9, 8, 6, 2), (8, 8, 6, 0), (8, 8, 4, 2)):                    # another Ws, Hs, grouping, batch
        with pytest.raises(ValueError, match="same geometry and grouping"):
            a.shared_table(*other)
    assert DA().shared_table(8, 8, 6, 2) == (None, 0)


def test_state_dict_round_trip():
    DA = _da()
    a = DA(seed=7)
    assert a.step == 0 and a.state_dict() == {"seed": 7, "step": 0}
    a.load_state_dict({"seed": 2 ** 40 + 1, "step": 2 ** 32 - 1})
    assert a.state_dict() == {"seed": 2 ** 40 + 1, "step": 2 ** 32 - 1} and a.desc_fields(8, 8)["seed"] == 2 ** 40 + 1
    b = DA()
    b.load_state_dict(a.state_dict())
    assert b.state_dict() == a.state_dict()
    for bad in ({"seed": -1, "step": 0}, {"seed": 0, "step": 2 ** 32}):
        with pytest.raises(ValueError):
            a.load_state_dict(bad)


def test_train_and_graphed_step_refuse_what_they_cannot_honour():
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import FrameAugment, SyntheticEpisodeDataset
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import GraphedTrainStep, train
    DA = _da()
    ds = SyntheticEpisodeDataset(horizon=2, device="cpu")
    with pytest.raises(ValueError, match="use_depth"):
        train(types.SimpleNamespace(use_depth=False), ds, {}, None, 1, 1, 1, {}, "cuda:0", depth_augment=DA())
    with pytest.raises(ValueError, match="DepthAugment"):
        train(types.SimpleNamespace(use_depth=True), ds, {}, None, 1, 1, 1, {}, "cuda:0", depth_augment=FrameAugment())
    fa = FrameAugment(erase_prob=1.0)
    for other in (None, FrameAugment(erase_prob=1.0)):
        with pytest.raises(ValueError, match="share_erase"):
            train(types.SimpleNamespace(use_depth=True), ds, {}, None, 1, 1, 1, {}, "cuda:0", augment=other, depth_augment=DA(share_erase=fa))
    par = inspect.signature(train).parameters["depth_augment"]
    assert par.default is None and par.kind == inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(GraphedTrainStep.__init__).parameters["depth_augment"].default is None


def test_torch_op_is_registered_for_the_device_only():
    import rgb_proprioceptive_pose_estimator_amd.torch_ops as T
    from rgb_proprioceptive_pose_estimator_amd import ops
    assert "augment_depth_f32" in T.NAMES and torch.ops.rpe.augment_depth_f32.default._schema.name == "rpe::augment_depth_f32"
    assert ops.DEPTH_AUGMENT_DESC_NUMBERS[:3] == ("seed_lo", "seed_hi", "n0") and len(ops.DEPTH_AUGMENT_DESC_NUMBERS) == 19
    with pytest.raises(NotImplementedError):
        torch.ops.rpe.augment_depth_f32(torch.zeros(1, 2, 2, 1), [0.0] * 19, torch.zeros(1, dtype=torch.int32))


def test_script_flags():
    from rgb_proprioceptive_pose_estimator_amd.scripts.train_model import DEPTH_AUGMENT_FLAGS, build_augment, build_depth_augment, build_parser, main
    p = build_parser()
    args = p.parse_args([])
    assert all(getattr(args, k) is None for k in DEPTH_AUGMENT_FLAGS) and args.aug_depth_share_erase is False
    assert build_depth_augment(args) is None                                   # everything off by default
    base = ["--use_depth", "--episodes", "x.npz"]
    flags = ["--aug_depth_noise", "0.001", "0.002", "0.003", "--aug_depth_drop_prob", "0.5", "--aug_depth_holes", "1", "3", "--aug_depth_hole_scale", "0.1", "0.2",
             "--aug_depth_hole_value", "-1", "--aug_depth_quant", "0.01", "--aug_depth_clamp", "0", "1", "--aug_depth_occluder_value", "0.25",
             "--aug_per_frame", "--aug_seed", "40"]
    a = build_depth_augment(p.parse_args(base + flags), rank=2)
    assert a.noise == (0.001, 0.002, 0.003) and a.n == tuple(v / T_STD for v in a.noise) and a.drop_thresh == 1 << 31 and a.holes == (1, 3)
    assert a.hole_scale == (0.1, 0.2) and a.hole_value == -1.0 and a.quant == 0.01 and a.clamp == (0.0, 1.0) and a.occluder_value == 0.25
    assert a.per_frame is True and a.seed == 42 and a.share_erase is None
    one = build_depth_augment(p.parse_args(base + ["--aug_depth_noise", "0.5"]))
    assert one.noise == (0.5, 0.0, 0.0) and one.per_frame is False and one.clamp == (-INF, INF) and one.seed == 0
    # the shared occluder hands over the FrameAugment of the same rank
    shared = p.parse_args(base + ["--aug_depth_share_erase", "--aug_erase_prob", "0.5", "--aug_depth_occluder_value", "1"])
    fa = build_augment(shared, rank=1)
    s = build_depth_augment(shared, rank=1, augment=fa)
    assert s.share_erase is fa and s.occluder_value == 1.0 and s.seed == fa.seed == 1 and s.per_frame is (not fa.per_episode)
    # the three combinations that cannot be honoured stop the run before anything is built
    for argv, word in ((["--episodes", "x.npz", "--aug_depth_noise", "0.1"], "--use_depth"), (["--use_depth", "--aug_depth_drop_prob", "0.1"], "--episodes"),
                       (base + ["--aug_depth_share_erase"], "--aug_erase_prob")):
        with pytest.raises(SystemExit, match=word):
            build_depth_augment(p.parse_args(argv), augment=build_augment(p.parse_args(argv)))
        with pytest.raises(SystemExit, match=word):
            main(argv)
    for bad in (["--aug_depth_noise", "1", "2", "3", "4"], ["--aug_depth_noise", "-1"], ["--aug_depth_holes", "0", "5"], ["--aug_depth_clamp", "1", "0"],
                ["--aug_depth_drop_prob", "2"]):
        with pytest.raises(SystemExit):
            build_depth_augment(p.parse_args(base + bad))
