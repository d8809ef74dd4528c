"""Head dropout without a GPU: the host-side constants, the properties of the rule as tests/_dropout_oracle.py restates it, the
validation of PoseModelBase.set_dropout, the script's flags and the registration of the two entry points."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _dropout_oracle as do
from _helpers import CASES, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 7


# -- host-side constants ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p, thresh, scale", [
    (0.0, 0, 1.0),
    (2.0 ** -32, 1, 1.0),                                     # 1 / (1 - 2^-32) rounds to 1 in fp32
    (0.1, 429496730, np.float32(1.0 / 0.9)),                  # round(0.1 * 2^32) = round(429496729.6)
    (0.5, 2 ** 31, 2.0),
    (1.0 - 2.0 ** -24, 2 ** 32 - 256, 2.0 ** 24),
])
def test_thresh_and_scale(p, thresh, scale):
    from rgb_proprioceptive_pose_estimator_amd import ops
    d = ops.dropout_desc(p, seed=2 ** 64 - 1)
    assert (d.seed, d.thresh) == (2 ** 64 - 1, thresh) and np.float32(d.scale) == np.float32(scale)
    assert np.float32(d.scale).view(np.uint32) == np.float32(1.0 / (1.0 - p)).view(np.uint32)      # divided in double, rounded once
    assert do.thresh_scale(p) == (thresh, np.float32(scale))


def test_thresh_is_capped_and_p_is_checked():
    from rgb_proprioceptive_pose_estimator_amd import ops
    assert ops.dropout_desc(np.nextafter(1.0, 0.0)).thresh == 2 ** 32 - 1      # round(p 2^32) = 2^32 there: the cap
    for bad in (-1e-9, -0.5, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.dropout_desc(bad)
        with pytest.raises(ValueError):
            do.thresh_scale(bad)
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            ops.dropout_desc(0.1, seed=bad)


# -- the rule --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [0.1, 0.5])
def test_kept_fraction(p):
    """65 536 elements: the kept count is binomial(65 536, q) with q = 1 - thresh 2^-32; five standard deviations"""
    n = 65536
    keep = do.keep_mask(SEED, 0, 0, 256, 0, 256, p)
    q = 1.0 - do.thresh_scale(p)[0] / 2.0 ** 32
    assert keep.size == n and abs(int(keep.sum()) - n * q) <= 5.0 * np.sqrt(n * q * (1.0 - q)), (int(keep.sum()), n * q)


def test_sites_and_steps_draw_different_masks():
    masks = {(site, step): do.keep_mask(SEED, step, site, 64, 0, 64, 0.5) for site in (0, 1, 2) for step in (3, 4)}
    keys = list(masks)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            # two unrelated fair masks of 4096 elements agree in 2048 +- 32 places: far from all of them
            agree = int((masks[a] == masks[b]).sum())
            assert abs(agree - 2048) <= 5 * 32, (a, b, agree)
    assert not np.array_equal(do.keep_mask(SEED, 3, 0, 64, 0, 64, 0.5), do.keep_mask(SEED + 1, 3, 0, 64, 0, 64, 0.5))      # ... and seeds
    assert not np.array_equal(do.keep_mask(SEED, 3, 0, 64, 0, 64, 0.5), do.keep_mask(SEED + 2 ** 32, 3, 0, 64, 0, 64, 0.5))   # the high key word counts
    assert np.array_equal(do.keep_mask(SEED, 2 ** 32 + 3, 0, 64, 0, 64, 0.5), masks[(0, 3)])      # the step is a 32-bit word


def test_mask_of_an_element_does_not_depend_on_the_range_or_the_row_count():
    full = do.keep_mask(SEED, 5, 1, 37, 0, 64, 0.5)
    for c0, c1 in ((0, 50), (3, 61), (5, 6), (4, 8), (63, 64)):
        for n in (1, 5, 37):
            assert np.array_equal(do.keep_mask(SEED, 5, 1, n, c0, c1, 0.5), full[:n, c0:c1]), (c0, c1, n)
    # one Philox call per aligned group of four columns: the four words of a group are the four outputs of ONE counter
    from _augment_oracle import philox4x32
    w = philox4x32((np.uint64(9), np.uint64(3), 5, do.PURPOSE + 1), (SEED, 0))
    assert [int(x) for x in w] == do.words(SEED, 5, 1, [9], range(12, 16))[0].tolist()


def test_oracle_select_and_columns():
    x = np.arange(1, 33, dtype=np.float32).reshape(4, 8)
    x[0, 2], x[1, 3], x[2, 4], x[3, 5] = np.nan, np.inf, -np.inf, -0.0
    x[0, 3], x[1, 4], x[2, 5], x[3, 2] = np.nan, np.inf, -np.inf, -0.0
    got = do.dropout_rows(x, SEED, 0, 0, 0.5, 2, 6)
    keep = do.keep_mask(SEED, 0, 0, 4, 2, 6, 0.5)
    assert keep.any() and not keep.all()
    assert np.array_equal(do.bits(got[:, :2]), do.bits(x[:, :2])) and np.array_equal(do.bits(got[:, 6:]), do.bits(x[:, 6:]))
    inner, src = got[:, 2:6], x[:, 2:6]
    assert (do.bits(inner)[~keep] == 0).all()                                    # +0.0 whatever stood there
    assert np.array_equal(do.bits(inner)[keep], do.bits(src * np.float32(2.0))[keep])
    sent = np.full_like(x, -7.5)
    out = do.dropout_rows(x, SEED, 0, 0, 0.5, 2, 6, out=sent)
    assert np.array_equal(do.bits(out[:, 2:6]), do.bits(inner)) and (out[:, :2] == -7.5).all() and (out[:, 6:] == -7.5).all()
    assert np.array_equal(do.bits(do.dropout_rows(x, SEED, 0, 0, 0.0)), do.bits(x * np.float32(1.0)))     # p = 0 keeps everything
    for kw in (dict(c0=-1), dict(c1=9), dict(c0=4, c1=4)):
        with pytest.raises(ValueError):
            do.dropout_rows(x, SEED, 0, 0, 0.5, **kw)
    with pytest.raises(ValueError):
        do.words(SEED, 0, 4, [0], [0])


def test_purpose_words_are_this_file_s_own():
    """0x44524F50 .. +3 occur in no other generator of the library"""
    csrc = os.path.join(ROOT, "rgb-proprioceptive-pose-estimator_amd", "csrc")
    mine = set(range(do.PURPOSE, do.PURPOSE + do.SITES))
    for name in ("augment.hip", "depth_augment.hip", "sample.hip", "measure.hip"):
        text = open(os.path.join(csrc, name)).read()
        used = {int(h, 16) for h in re.findall(r"Purpose\s*=\s*(0x[0-9A-Fa-f]+)u", text)}
        assert not (used & mine), (name, used & mine)
    assert min(mine) > 2       # augment.hip's purposes are the small integers 0..2
    assert "0x%08X" % do.PURPOSE in open(os.path.join(csrc, "dropout.hip")).read()


# -- the C ABI -------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_and_bound():
    from rgb_proprioceptive_pose_estimator_amd import _lib
    header = open(os.path.join(ROOT, "include", "rpe_hip.h")).read()
    for name in ("rpe_dropout_begin", "rpe_dropout_rows_f32"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS and hasattr(_lib.raw, name), name
    assert _lib.ABI_VERSION == 3 and _lib.raw.rpe_abi_version() == 3      # additive: the version stays
    D = _lib.DropoutDesc
    assert ctypes.sizeof(D) == 16 and (D.seed.offset, D.thresh.offset, D.scale.offset) == (0, 8, 12)
    body = header[header.rindex("typedef struct {", 0, header.index("} rpe_dropout_desc;")):header.index("} rpe_dropout_desc;")]
    assert re.findall(r"\b([a-z_]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [n for n, _ in D._fields_] == ["seed", "thresh", "scale"]


def test_rejected_arguments_need_no_device():
    """bad arguments come back as a status before anything is launched"""
    from rgb_proprioceptive_pose_estimator_amd import ops
    from rgb_proprioceptive_pose_estimator_amd._lib import raw
    one, two = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)   # never dereferenced: every call below is refused
    d = ops.dropout_desc(0.5, 1)
    good = dict(x=one, out=two, n=4, ld=8, c0=0, c1=8, site=0, picks=one, d=ctypes.byref(d))
    call = lambda **kw: raw.rpe_dropout_rows_f32(*[dict(good, **kw)[k] for k in ("x", "out", "n", "ld", "c0", "c1", "site", "picks", "d")], None)
    for kw in (dict(n=0), dict(n=-3), dict(n=2 ** 32), dict(c0=-1), dict(c1=9), dict(c0=8), dict(c0=5, c1=5), dict(c0=6, c1=2), dict(site=-1), dict(site=4),
               dict(x=None), dict(out=None), dict(picks=None), dict(d=None), dict(out=ctypes.c_void_p((1 << 20) + 32))):
        assert call(**kw) == 1, kw      # RPE_ERR_SHAPE
        assert b"dropout_rows_f32" in raw.rpe_last_error()
    assert raw.rpe_dropout_begin(None, one, None) == 1 and raw.rpe_dropout_begin(one, None, None) == 1 and b"dropout_begin" in raw.rpe_last_error()


def test_torch_ops_raise_for_cpu_tensors():
    import rgb_proprioceptive_pose_estimator_amd.torch_ops as T
    for name in ("dropout_begin", "dropout_rows"):
        assert name in T.NAMES and getattr(torch.ops.rpe, name).default._schema.name == "rpe::" + name
    s = torch.ops.rpe.dropout_begin.default._schema
    assert [a.name for a in s.arguments if a.alias_info is not None and a.alias_info.is_write] == ["state", "picks"]
    state, picks = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(NotImplementedError):     # the HIP key only: no CPU kernel to fall back to
        torch.ops.rpe.dropout_begin(state, picks)
    with pytest.raises(NotImplementedError):
        torch.ops.rpe.dropout_rows(torch.ones(2, 8), [7.0, 0.0, 0.5], picks, 0, 0, 8)
    assert state.item() == 0
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty(5, 12, device="cuda")
        y = torch.ops.rpe.dropout_rows(x, [7.0, 0.0, 0.5], torch.empty(1, dtype=torch.int32, device="cuda"), 1, 3, 9)
        assert y.shape == (5, 12) and y.dtype == torch.float32
    from rgb_proprioceptive_pose_estimator_amd import ops
    with pytest.raises(ValueError):     # the wrappers refuse a CPU tensor before any device work
        ops.dropout_rows(torch.ones(2, 8), ops.dropout_desc(0.5), picks)
    with pytest.raises(ValueError):
        ops.dropout_begin(state, picks)


# -- the models ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(CASES))
def test_set_dropout_validation_and_state_dict(kind):
    cfg = CASES[kind][0]
    plain = build(kind, cfg, torch.float32)
    keys = list(plain.state_dict())
    model = build(kind, cfg, torch.float32)
    sequence = kind in ("td", "tdo", "tdo_v2")
    assert model._drop_p == (0.0, 0.0) and model._drop_desc == {} and model._drop_state is None      # off by default
    assert model.HIDDEN_DROPOUT_SITES == {"td": (1, 2), "tdo": (1,), "tdo_v2": (1, 2)}.get(kind, ())
    assert model.set_dropout(feature=0.5, seed=7) is model
    assert sorted(model._drop_desc) == [0] and model._drop_desc[0].thresh == 2 ** 31 and model._drop_desc[0].seed == 7
    if sequence:
        model.set_dropout(feature=0.25, hidden=0.5, seed=9)
        assert sorted(model._drop_desc) == [0] + list(model.HIDDEN_DROPOUT_SITES)
        assert model._drop_desc[0].thresh == 2 ** 30 and all(model._drop_desc[s].thresh == 2 ** 31 for s in model.HIDDEN_DROPOUT_SITES)
        model.set_dropout(hidden=0.5)
        assert sorted(model._drop_desc) == list(model.HIDDEN_DROPOUT_SITES)
    else:
        with pytest.raises(ValueError, match="feature"):
            model.set_dropout(feature=0.5, hidden=0.1)
        assert sorted(model._drop_desc) == [0]      # a refused call changes nothing
        model.set_dropout(feature=0.5, hidden=0.0)
    for kw in (dict(feature=-0.1), dict(feature=1.0), dict(hidden=1.0), dict(hidden=-1.0), dict(feature=float("nan")), dict(seed=-1), dict(seed=2 ** 64)):
        with pytest.raises(ValueError):
            model.set_dropout(**kw)
    assert list(model.state_dict()) == keys and [n for n, _ in model.named_buffers()] == [n for n, _ in plain.named_buffers()]
    model.set_dropout()
    assert model._drop_desc == {} and model._drop_state is None      # zeros: off again; nothing on the device for a CPU model
    assert list(model.state_dict()) == keys


def test_constructor_signatures_are_unchanged():
    from rgb_proprioceptive_pose_estimator_amd import models as M
    want = {
        "NaiveEndEffectorStateEstimator": ["hidden_dims_pre_measurement", "hidden_dims_post_measurement", "num_resnet_layers", "latent_dim", "feature_extract",
                                           "compute_dtype"],
        "NaiveObjectStateEstimator": ["object_name", "hidden_dims", "num_resnet_layers", "latent_dim", "feature_extract", "feature_layer_nums", "use_depth",
                                      "use_pretrained", "no_proprioception", "compute_dtype"],
        "TemporallyDependentStateEstimator": ["hidden_dim_pre_measurement", "hidden_dim_post_measurement", "num_resnet_layers", "latent_dim", "sequence_length",
                                              "dropout_prob", "feature_extract", "feature_layer_nums", "use_depth", "use_pretrained", "device", "compute_dtype"],
        "TemporallyDependentObjectStateEstimator": ["object_name", "hidden_dim", "num_resnet_layers", "latent_dim", "sequence_length", "dropout_prob",
                                                    "feature_extract", "feature_layer_nums", "use_depth", "use_pretrained", "no_proprioception", "device",
                                                    "compute_dtype"],
        "TemporallyDependentObjectStateEstimatorV2": ["object_name", "img_hidden_dim", "proprio_hidden_dim", "num_resnet_layers", "latent_dim", "sequence_length",
                                                      "dropout_prob", "feature_extract", "feature_layer_nums", "use_depth", "use_pretrained", "device",
                                                      "compute_dtype"],
    }
    for name, params in want.items():
        sig = inspect.signature(getattr(M, name).__init__)
        assert list(sig.parameters)[1:] == params, name
        if "dropout_prob" in params:
            assert sig.parameters["dropout_prob"].default == 0.10      # accepted and unused, as in the reference
    assert list(inspect.signature(M.NaiveObjectStateEstimator.set_dropout).parameters) == ["self", "feature", "hidden", "seed"]


class _Recorder:
    HIDDEN_DROPOUT_SITES = (1,)

    def __init__(self):
        self.calls = []

    def set_dropout(self, **kw):
        self.calls.append(kw)
        return self


def test_script_flags():
    from rgb_proprioceptive_pose_estimator_amd.scripts import train_model as tm
    args = tm.build_parser().parse_args(["--model", "tdo"])
    assert (args.feature_dropout, args.hidden_dropout, args.dropout_seed) == (0.0, 0.0, 0)      # off by default
    rec = _Recorder()
    assert tm.apply_dropout(args, rec) is rec and rec.calls == []      # off: set_dropout is not even called
    args = tm.build_parser().parse_args(["--model", "tdo", "--feature_dropout", "0.25", "--hidden_dropout", "0.5", "--dropout_seed", "11"])
    assert (args.feature_dropout, args.hidden_dropout, args.dropout_seed) == (0.25, 0.5, 11)
    tm.apply_dropout(args, rec, rank=3)
    assert rec.calls == [dict(feature=0.25, hidden=0.5, seed=14)]      # a replica uses seed + rank
    for argv in (["--feature_dropout", "1.0"], ["--hidden_dropout", "-0.1"], ["--feature_dropout", "0.1", "--dropout_seed", "-1"]):
        with pytest.raises(SystemExit):
            tm.apply_dropout(tm.build_parser().parse_args(["--model", "tdo"] + argv))
    with pytest.raises(SystemExit, match="hidden_dropout"):      # the classes without an LSTM
        tm.apply_dropout(tm.build_parser().parse_args(["--model", "no", "--hidden_dropout", "0.1"]))
