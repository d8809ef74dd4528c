"""CPU side of the frame augmentation: the numpy oracle (tests/_augment_oracle.py) against the specification's known answers and
properties -- the kernel is compared with it for equality in tests/test_gpu_augment.py, so statistics are checked here, once -- and
the host logic of FrameAugment, train() and scripts/train_model.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _augment_oracle as ao

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q1 = 65536


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox_known_answers():
    assert _hex(ao.philox4x32((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(ao.philox4x32((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(ao.philox4x32((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # arrays of counters give the same words as one counter at a time
    r = ao.philox4x32((np.arange(3), 0, 7, 2), (5, 9))
    assert [int(w[2]) for w in r] == [int(w) for w in ao.philox4x32((2, 0, 7, 2), (5, 9))]


def _ramp(b=2, hs=9, ws=29):
    """a byte ramp through 0 and 255 in every channel"""
    n = b * hs * ws * 3
    return ((np.arange(n, dtype=np.int64) * 7) % 256).astype(np.uint8).reshape(b, hs, ws, 3)


def test_neutral_settings_are_the_identity():
    f = _ramp()
    assert f.min() == 0 and f.max() == 255
    out, params, _ = ao.augment(f, ao.neutral_desc(seed=3), 11)
    assert np.array_equal(out, f)
    assert params[0] == 11 and params.shape == (1 + 8 * 2,)


def test_pinned_factors():
    f = _ramp()
    out, _, _ = ao.augment(f, ao.neutral_desc(qb_lo=2 * Q1, qb_hi=2 * Q1), 0)
    assert np.array_equal(out, np.minimum(2 * f.astype(np.int64), 255).astype(np.uint8)) and (out == 255).any()
    out, _, _ = ao.augment(f, ao.neutral_desc(qs_lo=0, qs_hi=0), 0)
    grey = ao.grey(f.astype(np.int64))
    assert np.array_equal(out, np.repeat(grey[..., None], 3, -1).astype(np.uint8))
    out, _, sums = ao.augment(f, ao.neutral_desc(qc_lo=0, qc_hi=0), 0)
    p = f.shape[1] * f.shape[2]
    for b in range(f.shape[0]):
        m = (int(grey[b].sum()) + p // 2) // p
        assert int(sums[b]) == int(grey[b].sum()) and (out[b] == m).all()


def test_parameter_draws_over_4096_streams():
    hs, ws, g = 48, 64, 4096
    d = ao.neutral_desc(seed=0x123456789ABCDEF, qb_lo=Q1 // 2, qb_hi=3 * Q1 // 2, qc_lo=0, qc_hi=2 * Q1, qs_lo=Q1 - 1000, qs_hi=Q1 + 1000,
                        erase_thresh=1 << 31, eh_lo=5, eh_hi=14, ew_lo=6, ew_hi=19)
    p = ao.stream_params(d, g, hs, ws, step=5)
    for name, lo, hi in (("qb", d["qb_lo"], d["qb_hi"]), ("qc", d["qc_lo"], d["qc_hi"]), ("qs", d["qs_lo"], d["qs_hi"]), ("h", 5, 14), ("w", 6, 19)):
        v = p[name]
        assert v.min() >= lo and v.max() <= hi, name
        mid = (lo + hi) / 2.0
        assert (v < mid).any() and (v > mid).any(), name
    assert (p["top"] >= 0).all() and (p["top"] + p["h"] <= hs).all() and (p["left"] >= 0).all() and (p["left"] + p["w"] <= ws).all()
    assert (p["top"] < (hs - p["h"] + 1) / 2.0).any() and (p["top"] > (hs - p["h"] + 1) / 2.0).any()
    assert (p["left"] < (ws - p["w"] + 1) / 2.0).any() and (p["left"] > (ws - p["w"] + 1) / 2.0).any()
    assert abs(int(p["erase"].sum()) - 2048) <= 6 * 32     # binomial(4096, 0.5): sigma = 32
    # the extremes of the threshold
    assert ao.stream_params(dict(d, erase_thresh=0), g, hs, ws, 5)["erase"].sum() == 0
    assert ao.stream_params(dict(d, erase_thresh=2 ** 32 - 1), g, hs, ws, 5)["erase"].sum() >= g - 1
    # a full-frame rectangle has one position
    full = ao.stream_params(dict(d, eh_lo=hs, eh_hi=hs, ew_lo=ws, ew_hi=ws), 16, hs, ws, 5)
    assert (full["top"] == 0).all() and (full["left"] == 0).all()


def test_noise_statistics():
    noise_q = int(round(65536 * 8 / 147.8005))
    f = np.full((1, 64, 64, 3), 128, dtype=np.uint8)
    out, _, _ = ao.augment(f, ao.neutral_desc(seed=77, noise_q=noise_q), 3)
    n = out.astype(np.float64) - 128.0
    assert out.min() > 0 and out.max() < 255          # no clamp in play: the statistics are the noise's
    for c in range(3):
        assert abs(n[..., c].mean()) <= 0.5, (c, n[..., c].mean())
        assert abs(n[..., c].std() - 8.0) <= 0.8, (c, n[..., c].std())
    assert not np.array_equal(n[..., 0], n[..., 1])   # the channels draw from their own words


def test_determinism_and_grouping():
    f = _ramp(b=6, hs=8, ws=12).reshape(3, 2, 8, 12, 3)      # (S, N)
    d = ao.neutral_desc(seed=9, qb_lo=Q1 // 2, qb_hi=2 * Q1, qc_lo=Q1 // 2, qc_hi=2 * Q1, qs_lo=0, qs_hi=2 * Q1, noise_q=3000, erase_thresh=1 << 31,
                        eh_lo=2, eh_hi=5, ew_lo=2, ew_hi=7, fill_mode=1)
    a, pa, _ = ao.augment(f, d, 4)
    b, pb, _ = ao.augment(f, d, 4)
    c, pc, _ = ao.augment(f, d, 5)
    assert np.array_equal(a, b) and np.array_equal(pa, pb)
    assert not np.array_equal(a, c) and not np.array_equal(pa[1:], pc[1:]) and (pa[0], pc[0]) == (4, 5)
    assert not np.array_equal(ao.augment(f, dict(d, seed=10), 4)[0], a)
    assert pa.shape == (1 + 8 * 6,)
    # per_episode grouping: N = 2 streams, episode n keeps its parameters along S
    g, pg, _ = ao.augment(f, dict(d, group=2), 4)
    assert pg.shape == (1 + 8 * 2,) and np.array_equal(pg, pa[:17])
    # the same frame in every timestep of an episode: without noise the outputs repeat along S
    same = np.broadcast_to(f[:1], f.shape).copy()
    g2, _, _ = ao.augment(same, dict(d, group=2, noise_q=0, fill_mode=0), 4)
    assert np.array_equal(g2[0], g2[1]) and np.array_equal(g2[0], g2[2]) and not np.array_equal(g2[:, 0], g2[:, 1])
    u2, _, _ = ao.augment(same, dict(d, group=0, noise_q=0, fill_mode=0), 4)
    assert not np.array_equal(u2[0], u2[1])
    # the noise is per frame even when the parameters are grouped
    n2, _, _ = ao.augment(same, ao.neutral_desc(seed=9, noise_q=3000, group=2), 4)
    assert not np.array_equal(n2[0], n2[1])


def test_erase_rectangle_and_fills():
    f = _ramp(b=2, hs=16, ws=16)
    d = ao.neutral_desc(seed=1, erase_thresh=2 ** 32 - 1, eh_lo=3, eh_hi=8, ew_lo=3, ew_hi=8, fill_rgb=(1, 2, 3))
    out, params, _ = ao.augment(f, d, 0)
    for b in range(2):
        qb, qc, qs, erase, top, left, h, w = params[1 + 8 * b:9 + 8 * b]
        assert erase == 1
        mask = np.zeros((16, 16), bool)
        mask[top:top + h, left:left + w] = True
        assert (out[b][mask] == (1, 2, 3)).all() and np.array_equal(out[b][~mask], f[b][~mask])
    rnd, _, _ = ao.augment(f, dict(d, fill_mode=1), 0)
    changed = (rnd != f).any(-1)
    assert changed.sum() > 0 and np.array_equal(rnd[~changed], f[~changed])


# -- host logic -------------------------------------------------------------------------------------------------------------------

def _fa():
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import FrameAugment
    return FrameAugment


def test_entry_point_is_declared_and_bound():
    from rgb_proprioceptive_pose_estimator_amd import _lib
    header = open(os.path.join(ROOT, "include", "rpe_hip.h")).read()
    assert re.search(r"\brpe_augment_frames_u8\s*\(", header) and "rpe_augment_frames_u8" in _lib.EXPORTS and hasattr(_lib.raw, "rpe_augment_frames_u8")
    # the ctypes mirror of rpe_augment_desc: field order as in the header, the C layout (8-byte seed first, the fill bytes padded)
    names = [n for n, _ in _lib.AugmentDesc._fields_]
    body = header[header.index("unsigned long long seed;"):header.index("} rpe_augment_desc;")]
    assert [n for n in re.findall(r"\b([a-z_]+)(?=[,;\[])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))] == names
    assert ctypes.sizeof(_lib.AugmentDesc) == 72 and _lib.AugmentDesc.group.offset == 64 and _lib.AugmentDesc.erase_thresh.offset == 36


def test_rejected_arguments_need_no_device():
    """bad arguments come back as a status before anything is launched"""
    from rgb_proprioceptive_pose_estimator_amd import ops
    from rgb_proprioceptive_pose_estimator_amd._lib import raw
    one = ctypes.c_void_p(16)   # never dereferenced: every call below is refused
    call = lambda d, b=1, hs=8, ws=8, inp=one, out=one: raw.rpe_augment_frames_u8(inp, out, b, hs, ws, ctypes.byref(d), one, one, one, None)
    for kw in (dict(qb_lo=-1), dict(qb_lo=70000, qb_hi=65536), dict(qc_hi=4 * Q1 + 1), dict(qs_lo=5, qs_hi=4), dict(noise_q=-1), dict(noise_q=4 * Q1 + 1),
               dict(eh_lo=0), dict(eh_hi=9), dict(ew_lo=3, ew_hi=2), dict(ew_hi=9), dict(fill_mode=2), dict(group=-1)):
        assert call(ops.augment_desc(**kw)) == 1, kw      # RPE_ERR_SHAPE
    good = ops.augment_desc()
    assert call(good, b=0) == 1 and call(good, hs=0) == 1 and call(good, hs=1 << 16, ws=1 << 16) == 1
    assert call(good, inp=None) == 1
    assert call(good, inp=ctypes.c_void_p(1 << 20), out=ctypes.c_void_p((1 << 20) + 64)) == 1          # partial overlap
    assert b"overlap" in raw.rpe_last_error()
    with pytest.raises(ValueError):
        ops.augment_desc(fill_r=256)


def test_frame_augment_validation_and_q16():
    FA = _fa()
    a = FA(brightness=0.2, contrast=0.5, saturation=1.5, noise_std=8.0, erase_prob=0.25, erase_scale=(0.1, 0.3), erase_fill="noise", seed=5)
    assert a.qb == (round(65536 * 0.8), round(65536 * 1.2)) and a.qc == (32768, 98304) and a.qs == (0, 163840)
    assert a.noise_q == round(65536 * 8.0 / 147.8005) and a.erase_thresh == 1 << 30 and a.fill_mode == 1
    assert FA(erase_prob=1.0).erase_thresh == 2 ** 32 - 1 and FA().erase_thresh == 0
    f = a.desc_fields(64, 100, group=4)
    assert (f["eh_lo"], f["eh_hi"], f["ew_lo"], f["ew_hi"], f["group"], f["seed"]) == (6, 19, 10, 30, 4, 5)
    assert FA(erase_scale=(0.01, 0.02)).erase_bounds(5) == (1, 1) and FA(erase_scale=(1.0, 1.0)).erase_bounds(7) == (7, 7)
    off = FA()
    assert (off.qb, off.qc, off.qs, off.noise_q, off.erase_thresh, off.fill_rgb) == ((Q1, Q1), (Q1, Q1), (Q1, Q1), 0, 0, (124, 116, 104))
    assert FA(erase_fill=(1, 2, 3)).fill_rgb == (1, 2, 3) and FA(erase_fill=(1, 2, 3)).fill_mode == 0
    for kw in (dict(brightness=-0.1), dict(contrast=3.5), dict(saturation=float("nan")), dict(noise_std=-1.0), dict(noise_std=1e4), dict(erase_prob=1.5),
               dict(erase_scale=(0.0, 0.3)), dict(erase_scale=(0.4, 0.3)), dict(erase_scale=(0.1, 1.1)), dict(erase_fill="black"), dict(erase_fill=(1, 2)),
               dict(erase_fill=(1, 2, 300)), dict(seed=-1)):
        with pytest.raises(ValueError):
            FA(**kw)
    for bad in (torch.zeros(2, 8, 8, 3), torch.zeros(2, 8, 8, 3, dtype=torch.uint8),                       # float frames; host frames
                torch.zeros(2, 3, 8, 8, dtype=torch.uint8), torch.zeros(8, 8, 3, dtype=torch.uint8), np.zeros((2, 8, 8, 3), np.uint8)):
        with pytest.raises(ValueError):
            a(bad)


def test_frame_augment_state_dict_round_trip():
    FA = _fa()
    a = FA(seed=7)
    assert a.step == 0 and a.state_dict() == {"seed": 7, "step": 0}
    a.load_state_dict({"seed": 2 ** 40 + 1, "step": 2 ** 32 - 1})
    assert a.state_dict() == {"seed": 2 ** 40 + 1, "step": 2 ** 32 - 1} and a.desc_fields(8, 8)["seed"] == 2 ** 40 + 1
    b = FA()
    b.load_state_dict(a.state_dict())
    assert b.state_dict() == a.state_dict()
    for bad in ({"seed": -1, "step": 0}, {"seed": 0, "step": 2 ** 32}):
        with pytest.raises(ValueError):
            a.load_state_dict(bad)


def test_train_refuses_augment_without_uint8_frames():
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import SyntheticEpisodeDataset
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import GraphedTrainStep, train
    ds = SyntheticEpisodeDataset(horizon=2, device="cpu")
    with pytest.raises(ValueError, match="uint8"):
        train(None, ds, {}, None, 1, 1, 1, {}, "cuda:0", augment=_fa()())
    import inspect
    assert inspect.signature(train).parameters["augment"].default is None and inspect.signature(train).parameters["augment"].kind == inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(GraphedTrainStep.__init__).parameters["augment"].default is None


def test_script_flags():
    from rgb_proprioceptive_pose_estimator_amd.scripts.train_model import build_augment, build_parser
    p = build_parser()
    args = p.parse_args([])
    assert all(getattr(args, k) is None for k in ("aug_brightness", "aug_contrast", "aug_saturation", "aug_noise_std", "aug_erase_prob", "aug_erase_scale",
                                                    "aug_erase_fill", "aug_seed")) and args.aug_per_frame is False
    assert build_augment(args) is None                                   # everything off by default
    flags = ["--aug_brightness", "0.2", "--aug_contrast", "0.3", "--aug_saturation", "0.4", "--aug_noise_std", "2", "--aug_erase_prob", "0.5",
             "--aug_erase_scale", "0.2", "0.4", "--aug_erase_fill", "10,20,30", "--aug_per_frame", "--aug_seed", "40"]
    with pytest.raises(SystemExit, match="--episodes"):
        build_augment(p.parse_args(flags))
    with pytest.raises(SystemExit, match="--episodes"):
        build_augment(p.parse_args(["--aug_per_frame"]))
    a = build_augment(p.parse_args(flags + ["--episodes", "x.npz"]), rank=2)
    assert a.qb == (round(65536 * 0.8), round(65536 * 1.2)) and a.qc[0] == round(65536 * 0.7) and a.qs[1] == round(65536 * 1.4)
    assert a.noise_q == round(65536 * 2 / 147.8005) and a.erase_thresh == 1 << 31 and a.erase_scale == (0.2, 0.4)
    assert a.fill_rgb == (10, 20, 30) and a.per_episode is False and a.seed == 42
    assert build_augment(p.parse_args(["--episodes", "x.npz", "--aug_erase_prob", "1", "--aug_erase_fill", "noise"])).fill_mode == 1
    for bad in (["--aug_erase_fill", "red"], ["--aug_brightness", "-1"]):
        with pytest.raises(SystemExit):
            build_augment(p.parse_args(["--episodes", "x.npz"] + bad))
