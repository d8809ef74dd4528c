"""CPU side of the device measurement noise: the numpy oracle (tests/_measure_oracle.py) against the specification's known answers and
statistical properties -- the kernels are compared with it in tests/test_gpu_measure.py, so the distribution is checked here, once --
and the host logic of ops.measure_desc, MeasurementNoise, train(), GraphedTrainStep and scripts/train_model.py.

Every statistical bound is five standard errors of its estimator under the specification (n independent standard normals: mean
1/sqrt(n), variance sqrt(2/n), excess kurtosis sqrt(24/n), a correlation 1/sqrt(n), a binomial count sqrt(n p (1 - p)))."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import _measure_oracle as mo
from _augment_oracle import philox4x32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


# -- the oracle -------------------------------------------------------------------------------------------------------------------

def test_known_answers():
    # Philox4x32-10 itself: the published known answers of the Random123 distribution
    assert [int(w) for w in philox4x32((0, 0, 0, 0), (0, 0))] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(w) for w in philox4x32((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2)] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    # row 11, component 4, step 7 under SEED: counter (11, 4, 7, "MEAS"), key (0x89ABCDEF, 0x01234567) -> words 0x1621076F, 0xA088997C
    # (worked with Python integers, outside numpy); u1 = (r0 + 0.5) 2^-32, u2 = r1 2^-32, z = sqrt(-2 ln u1) cos(2 pi u2)
    r = philox4x32((11, 4, 7, 0x4D454153), (0x89ABCDEF, 0x01234567))
    assert (int(r[0]), int(r[1])) == (0x1621076F, 0xA088997C)
    u1, u2 = mo.uniforms(SEED, [11], 7)
    assert u1[0, 4] == (0x1621076F + 0.5) / 2.0 ** 32 == 0.0864414832321927 and u2[0, 4] == 0xA088997C / 2.0 ** 32 == 0.6270843436941504
    z = mo.normals(SEED, [11], 7)[0, 4]
    assert abs(z - math.sqrt(-2.0 * math.log(0.0864414832321927)) * math.cos(2.0 * math.pi * 0.6270843436941504)) <= 4e-16
    assert abs(z - -1.5440750683037825) <= 4e-16
    # the scale of lane 5 at step 7, three scales: word 0 at counter (5, 0, 7, "MEAK") is 0x04688B09 -> (r0 * 3) >> 32 = 0
    assert int(philox4x32((5, 0, 7, 0x4D45414B), (0x89ABCDEF, 0x01234567))[0]) == 0x04688B09
    assert mo.scale_picks(SEED, 6, 3, 7).tolist() == [2, 2, 2, 0, 2, 0]
    assert mo.scale_picks(SEED, 6, 1, 7).tolist() == [0] * 6      # one scale: no draw
    # the extremes of the two uniforms stay inside the domain of log: u1 in (0, 1), u2 in [0, 1)
    assert (0.5 / 2.0 ** 32 > 0.0) and ((2.0 ** 32 - 0.5) / 2.0 ** 32 < 1.0)


def test_moments():
    z = mo.normals(1, np.arange(40000), 0).ravel()
    n = z.size
    assert n == 280000 and np.isfinite(z).all()
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var ** 2 - 3.0
    print("mean %.5f var %.5f excess kurtosis %.5f" % (mean, var, kurt))
    assert abs(mean) <= 5.0 / math.sqrt(n)
    assert abs(var - 1.0) <= 5.0 * math.sqrt(2.0 / n)
    assert abs(kurt) <= 5.0 * math.sqrt(24.0 / n)


def test_steps_seeds_and_components_are_uncorrelated():
    rows = np.arange(40000)
    a = mo.normals(1, rows, 0)
    n = a.size
    bound = 5.0 / math.sqrt(n)
    for name, b in (("step", mo.normals(1, rows, 1)), ("seed", mo.normals(2, rows, 0)), ("high seed word", mo.normals(1 + 2 ** 32, rows, 0)),
                    ("step wrap", mo.normals(1, rows, 2 ** 32 - 1))):
        assert not np.array_equal(a, b) and abs(_corr(a, b)) <= bound, (name, _corr(a, b))
    cbound = 5.0 / math.sqrt(len(rows))
    for c in range(7):
        for c2 in range(c + 1, 7):
            assert abs(_corr(a[:, c], a[:, c2])) <= cbound, (c, c2)
    assert abs(_corr(a[:-1], a[1:])) <= bound           # neighbouring rows
    assert np.array_equal(mo.normals(1, rows[:8], 5), mo.normals(1, rows[:8], 5 + 2 ** 32))      # the step enters modulo 2^32


def test_scale_picks_hit_every_index_evenly():
    n = 30000
    for step in (0, 1):
        k = mo.scale_picks(9, n, 3, step)
        counts = np.bincount(k, minlength=3)
        assert counts.shape == (3,) and counts.sum() == n
        assert (np.abs(counts - n / 3.0) <= 5.0 * math.sqrt(n * (1 / 3.0) * (2 / 3.0))).all(), counts
    assert not np.array_equal(mo.scale_picks(9, n, 3, 0), mo.scale_picks(9, n, 3, 1))
    assert set(mo.scale_picks(9, 4000, 8, 0).tolist()) == set(range(8))
    # the picks are independent of the normals drawn for the same lane
    assert abs(_corr(mo.scale_picks(9, n, 3, 0).astype(np.float64), mo.normals(9, np.arange(n), 0)[:, 0])) <= 5.0 / math.sqrt(n)


def test_ar1_is_stationary_with_the_asked_correlation():
    s, lanes = 50, 4000
    e = mo.unit_noise(3, s, lanes, 0.9, 0)
    n = lanes * 7
    for t in (0, s - 1):
        assert abs(e[t].var() - 1.0) <= 5.0 * math.sqrt(2.0 / n), (t, e[t].var())
    lag1 = _corr(e[:-1], e[1:])
    print("lag-1 correlation %.4f" % lag1)
    assert abs(lag1 - 0.9) <= 5.0 / math.sqrt(lanes)
    z = mo.normals(3, np.arange(s * lanes), 0).reshape(s, lanes, 7)
    assert np.array_equal(e[0], z[0])
    assert np.array_equal(e[1], 0.9 * z[0] + np.sqrt(1.0 - 0.9 * 0.9) * z[1])
    assert np.array_equal(mo.unit_noise(3, s, lanes, 0.0, 0), z)      # rho = 0: the white draw, exactly


def _poses(shape, seed=0):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=shape + (4,))
    return np.concatenate([rng.random(shape + (3,)), q / np.linalg.norm(q, axis=-1, keepdims=True)], -1).astype(np.float32)


def test_scale_zero_returns_x0_with_the_quaternion_renormalised():
    x0 = _poses((3, 5))
    x0[..., 3:] *= 1.5          # not unit: the division shows
    out, picks = mo.measure(x0, 4, [0.0], 0.0, 2)
    x = x0.astype(np.float64)
    a, b, c, d = (x[..., i] for i in (3, 4, 5, 6))
    want = np.concatenate([x[..., :3], x[..., 3:] / np.sqrt(a * a + b * b + c * c + d * d)[..., None]], -1).astype(np.float32)
    assert out.dtype == np.float32 and out.shape == x0.shape and np.array_equal(out[..., :3], x0[..., :3])
    assert np.array_equal(out, want) and mo.compare(out, want) == (0, 0)
    assert np.abs(np.linalg.norm(out[..., 3:].astype(np.float64), axis=-1) - 1.0).max() <= 1e-6
    assert picks.tolist() == [2, 0, 0, 0, 0, 0]


def test_measure_layout_and_scales():
    x0 = _poses((4, 6))
    out, picks = mo.measure(x0, 7, [0.0, 0.04], 0.5, 3)
    k = mo.scale_picks(7, 6, 2, 3)
    assert picks.dtype == np.int32 and picks.tolist() == [3] + k.tolist() and set(k.tolist()) == {0, 1}
    e = mo.unit_noise(7, 4, 6, 0.5, 3)
    for lane in range(6):      # one scale per lane, shared along S
        moved = np.abs(out[:, lane, :3] - x0[:, lane, :3]).max()
        if k[lane] == 0:
            assert moved == 0.0
        else:
            assert np.array_equal(out[:, lane, :3], (x0[:, lane, :3].astype(np.float64) + 0.2 * e[:, lane, :3]).astype(np.float32))
    assert np.abs(np.linalg.norm(out[..., 3:].astype(np.float64), axis=-1) - 1.0).max() <= 1e-6
    flat, fpicks = mo.measure(x0.reshape(24, 7), 7, [0.04], 0.0, 3)      # a flat batch is S = 1: lanes = rows
    assert flat.shape == (24, 7) and fpicks.shape == (25,)
    one, _ = mo.measure(x0[:1].reshape(6, 7), 7, [0.04], 0.0, 3)
    assert np.array_equal(one, flat[:6])
    assert mo.measure(x0, 7, [0.04], 0.0, 2 ** 32 - 1)[1][0] == -1       # the counter is stored as 32 bits
    with np.errstate(all="ignore"):
        z = np.zeros((1, 7), dtype=np.float32)
        assert np.isnan(mo.measure(z, 0, [0.0], 0.0, 0)[0][0, 3:]).all()      # a zero norm: what IEEE division yields


# -- the C ABI ------------------------------------------------------------------------------------------------------------------

def test_entry_point_is_declared_and_bound():
    from rgb_proprioceptive_pose_estimator_amd import _lib
    import rgb_proprioceptive_pose_estimator_amd.torch_ops as T
    header = open(os.path.join(ROOT, "include", "rpe_hip.h")).read()
    assert re.search(r"\brpe_measurement_noise\s*\(", header) and "rpe_measurement_noise" in _lib.EXPORTS and hasattr(_lib.raw, "rpe_measurement_noise")
    assert _lib.ABI_VERSION == 3 and _lib.raw.rpe_abi_version() == 3      # additive: the version stays
    body = header[header.rindex("typedef struct {", 0, header.index("} rpe_measure_desc;")):header.index("} rpe_measure_desc;")]
    names = re.findall(r"\b([A-Za-z_]+)(?=(?:\[8\])?[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in _lib.MeasureDesc._fields_] == ["seed", "S", "N", "num_scales", "sigma", "rho"]
    M = _lib.MeasureDesc
    assert ctypes.sizeof(M) == 96 and (M.S.offset, M.N.offset, M.num_scales.offset, M.sigma.offset, M.rho.offset) == (8, 12, 16, 24, 88)
    assert "measurement_noise" in T.NAMES
    s = torch.ops.rpe.measurement_noise.default._schema
    assert s.name == "rpe::measurement_noise" and [a.name for a in s.arguments] == ["x0", "desc", "state"]
    assert [a.name for a in s.arguments if a.alias_info is not None and a.alias_info.is_write] == ["state"]
    with pytest.raises(NotImplementedError):     # the HIP key only: no CPU kernel to fall back to
        torch.ops.rpe.measurement_noise(torch.zeros(2, 7), [0.0, 0.0, 1.0, 2.0, 0.0, 0.001], torch.zeros(1, dtype=torch.int32))
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x0 = torch.empty(4, 6, 7, device="cuda")
        out = torch.ops.rpe.measurement_noise(x0, [1.0, 0.0, 4.0, 6.0, 0.5, 0.001, 0.01], torch.empty(1, dtype=torch.int32, device="cuda"))
        assert out.shape == (4, 6, 7) and out.dtype == torch.float32


def _raw_desc(seed=1, S=2, N=3, num_scales=2, sigma=(0.1, 0.2), rho=0.5):
    from rgb_proprioceptive_pose_estimator_amd._lib import MeasureDesc
    d = MeasureDesc()
    d.seed, d.S, d.N, d.num_scales, d.rho = seed, S, N, num_scales, rho
    for k, v in enumerate(sigma):
        d.sigma[k] = v
    return d


BAD_DESCS = [dict(S=0), dict(N=0), dict(S=-1), dict(N=-4), dict(S=2 ** 16, N=2 ** 15), dict(S=2 ** 30, N=2), dict(num_scales=0), dict(num_scales=9),
             dict(num_scales=-1), dict(sigma=(-0.1, 0.2)), dict(sigma=(0.1, float("inf"))), dict(sigma=(float("nan"), 0.2)), dict(sigma=(0.1, -1e-300)),
             dict(rho=-0.01), dict(rho=1.0), dict(rho=1.5), dict(rho=float("nan")), dict(rho=float("inf"))]


def test_rejected_arguments_need_no_device():
    """bad arguments come back as a status before anything is launched"""
    from rgb_proprioceptive_pose_estimator_amd._lib import raw
    one, two = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20)   # never dereferenced: every call below is refused
    call = lambda d, x0=one, out=two, state=one, picks=one: raw.rpe_measurement_noise(x0, out, ctypes.byref(d) if d is not None else None, state, picks, None)
    for kw in BAD_DESCS:
        assert call(_raw_desc(**kw)) == 1, kw      # RPE_ERR_SHAPE
        assert b"measurement_noise" in raw.rpe_last_error()
    d = _raw_desc()
    assert call(None) == 1 and call(d, x0=None) == 1 and call(d, out=None) == 1 and call(d, state=None) == 1 and call(d, picks=None) == 1
    assert call(d, out=ctypes.c_void_p((1 << 20) + 28)) == 1 and b"overlap" in raw.rpe_last_error()      # shifted by one row: neither equal nor disjoint


def test_measure_desc():
    from rgb_proprioceptive_pose_estimator_amd import ops
    d = ops.measure_desc(seed=2 ** 64 - 1, S=4, N=64, scales=[0.25, 4.0, 0.0], correlation=0.9)
    assert (d.seed, d.S, d.N, d.num_scales, d.rho) == (2 ** 64 - 1, 4, 64, 3, 0.9) and list(d.sigma)[:4] == [0.5, 2.0, 0.0, 0.0]
    d = ops.measure_desc(scales=0.001)
    assert (d.seed, d.S, d.N, d.num_scales, d.rho) == (0, 1, 1, 1, 0.0) and d.sigma[0] == math.sqrt(0.001)      # sigma in double
    assert ops.measure_desc(scales=np.float32(0.5)).sigma[0] == math.sqrt(0.5)
    for kw in (dict(seed=-1), dict(seed=2 ** 64), dict(S=0), dict(N=0), dict(S=2 ** 16, N=2 ** 15), dict(scales=[]), dict(scales=[0.1] * 9), dict(scales=[-0.1]),
               dict(scales=-1e-9), dict(scales=[0.1, float("inf")]), dict(scales=float("nan")), dict(correlation=-0.1), dict(correlation=1.0),
               dict(correlation=float("nan"))):
        with pytest.raises(ValueError):
            ops.measure_desc(**kw)
    assert ops.MEASURE_DESC_NUMBERS == ("seed_lo", "seed_hi", "S", "N", "correlation") and ops.MEASURE_MAX_SCALES == 8


# -- host logic -------------------------------------------------------------------------------------------------------------------

def test_measurement_noise_validation_and_state_dict():
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import MeasurementNoise
    n = MeasurementNoise()
    assert (n.scales, n.correlation, n.seed, n.step, n.last_picks) == ((0.001,), 0.0, 0, 0, None)
    n = MeasurementNoise([0.001, 0.01], correlation=0.5, seed=2 ** 64 - 1)
    assert n.scales == (0.001, 0.01) and n.desc_fields(4, 6) == dict(seed=2 ** 64 - 1, S=4, N=6, scales=(0.001, 0.01), correlation=0.5)
    assert MeasurementNoise(0.0).scales == (0.0,) and MeasurementNoise((0.5,) * 8).scales == (0.5,) * 8
    for kw in (dict(scale=-0.001), dict(scale=float("inf")), dict(scale=float("nan")), dict(scale=[]), dict(scale=[0.1] * 9), dict(scale=[0.1, -0.1]),
               dict(correlation=-0.1), dict(correlation=1.0), dict(correlation=float("nan")), dict(seed=-1), dict(seed=2 ** 64)):
        with pytest.raises(ValueError):
            MeasurementNoise(**kw)
    # anything but a contiguous fp32 device tensor (B, 7) / (S, N, 7) is refused before any device work
    for bad in (torch.zeros(3, 7), torch.zeros(2, 3, 7), torch.zeros(3, 7, dtype=torch.float64), torch.zeros(3, 7, dtype=torch.float16), torch.zeros(3, 6),
                torch.zeros(7), torch.zeros(2, 2, 3, 7), torch.zeros(0, 7), torch.zeros(7, 3).t(), np.zeros((3, 7), dtype=np.float32), None):
        with pytest.raises(ValueError):
            n(bad)
    with pytest.raises(ValueError, match="device only"):
        n(torch.zeros(3, 7))
    assert n.step == 0 and n.state_dict() == {"seed": 2 ** 64 - 1, "step": 0}      # a refused call does not count
    n.load_state_dict({"seed": 5, "step": 2 ** 32 - 1})
    assert n.state_dict() == {"seed": 5, "step": 2 ** 32 - 1} and n.desc_fields(1, 2)["seed"] == 5
    m = MeasurementNoise()
    m.load_state_dict(n.state_dict())
    assert m.state_dict() == n.state_dict()
    for bad in ({"seed": -1, "step": 0}, {"seed": 2 ** 64, "step": 0}, {"seed": 0, "step": 2 ** 32}, {"seed": 0, "step": -1}):
        with pytest.raises(ValueError):
            n.load_state_dict(bad)
    assert n.state_dict() == {"seed": 5, "step": 2 ** 32 - 1}


def test_train_and_graphed_step_signatures_and_refusals():
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import SyntheticEpisodeDataset
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import GraphedTrainStep, train
    p = inspect.signature(train).parameters["measurement_noise"]
    assert p.default is None and p.kind == inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(GraphedTrainStep.__init__).parameters["measurement_noise"].default is None
    for bad in (0.001, [0.001], "on", object()):      # (refused before the model, the optimizer or the device are touched)
        with pytest.raises(ValueError, match="MeasurementNoise"):
            train(None, SyntheticEpisodeDataset(horizon=2, device="cpu"), {}, None, 1, 1, 1, {}, "cuda:0", measurement_noise=bad)


def test_script_flags():
    from rgb_proprioceptive_pose_estimator_amd.scripts.train_model import build_measurement_noise, build_parser
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import MeasurementNoise
    p = build_parser()
    args = p.parse_args([])
    assert args.meas_noise_device is False and args.meas_noise_scales is None and args.meas_noise_correlation is None and args.meas_noise_seed is None
    assert build_measurement_noise(args) is None
    n = build_measurement_noise(p.parse_args(["--meas_noise_device"]))
    assert isinstance(n, MeasurementNoise) and (n.scales, n.correlation, n.seed) == ((0.001,), 0.0, 0)      # [--noise_scale]
    n = build_measurement_noise(p.parse_args(["--meas_noise_device", "--noise_scale", "0.02"]))
    assert n.scales == (0.02,)
    n = build_measurement_noise(p.parse_args(["--meas_noise_scales", "0.001", "0.01", "0.1", "--meas_noise_correlation", "0.8", "--meas_noise_seed", "7"]), rank=2)
    assert (n.scales, n.correlation, n.seed) == ((0.001, 0.01, 0.1), 0.8, 9)      # rank r uses K + r
    assert build_measurement_noise(p.parse_args(["--meas_noise_correlation", "0.5"])).correlation == 0.5      # needs no other flag
    assert build_measurement_noise(p.parse_args(["--meas_noise_seed", str(2 ** 64 - 1)])).seed == 2 ** 64 - 1
    for flags, name in ((["--meas_noise_scales", "-0.1"], "--meas_noise_scales"), (["--meas_noise_scales", "0.1", "inf"], "--meas_noise_scales"),
                        (["--meas_noise_scales", "nan"], "--meas_noise_scales"), (["--meas_noise_scales"] + ["0.1"] * 9, "--meas_noise_scales"),
                        (["--meas_noise_device", "--noise_scale", "-1"], "--noise_scale"),
                        (["--meas_noise_correlation", "1.0"], "--meas_noise_correlation"), (["--meas_noise_correlation", "-0.5"], "--meas_noise_correlation"),
                        (["--meas_noise_correlation", "nan"], "--meas_noise_correlation"),
                        (["--meas_noise_seed", "-1"], "--meas_noise_seed"), (["--meas_noise_seed", str(2 ** 64)], "--meas_noise_seed")):
        with pytest.raises(SystemExit, match=name):
            build_measurement_noise(p.parse_args(flags))
    with pytest.raises(SystemExit, match="--meas_noise_seed"):
        build_measurement_noise(p.parse_args(["--meas_noise_seed", str(2 ** 64 - 1)]), rank=1)
