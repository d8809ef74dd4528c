"""Self-tests of the telemetry reference (tests/_telemetry_oracle.py) and the host side of the feature, on the CPU.

- reference: the oracle equals torch.linalg.vector_norm on finite inputs and counts planted inf / NaN / +-0 exactly;
- soundness: the oracle evaluated in other summation orders (forward, reversed, pairwise) stays at <= 0.5 of every bound;
- host: the three entry points in the header, the library and _lib's table; the row-count function; the table builder against
  ParamArena; constructor validation; state_dict compatibility both ways; the dispatcher entry; train() and the script's flags."""
import math
import os

import numpy as np
import pytest
import torch

import _telemetry_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rpe_param_stats_rows", "rpe_param_stats", "rpe_param_stats_finalize")
HP = dict(b1=0.9, b2=0.999, eps=1e-8)


def _case(n, seed, scale=1.0):
    r = np.random.default_rng(seed)
    p, g = r.standard_normal(n).astype(np.float32), (r.standard_normal(n) * scale).astype(np.float32)
    m, v = (r.standard_normal(n) * 0.1 * scale).astype(np.float32), (r.random(n) * 0.01 * scale * scale).astype(np.float32)
    return p, g, m, v


def _chunk():
    """C: the largest numel that takes one row"""
    from rgb_proprioceptive_pose_estimator_amd import _lib
    rows = _lib.lib.rpe_param_stats_rows
    lo, hi = 1, 1 << 30
    assert rows(lo) == 1 and rows(hi) > 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if rows(mid) == 1 else (lo, mid - 1)
    return lo


# ------------------------------------------------------------------ the reference
def test_oracle_matches_torch_norms_and_counts_planted_values():
    for n, scale in ((1, 1.0), (3, 1.0), (5, 1e-3), (1025, 1.0), (8195, 30.0)):
        p, g, m, v = _case(n, n, scale)
        row, _ = TO.tensor_row(p, g, m, v, 3, **HP)
        for got, t in ((row[0], g), (row[1], p)):
            want = float(torch.linalg.vector_norm(torch.from_numpy(t).double()))
            assert abs(math.sqrt(got) - want) <= 1e-14 * want
        d = (torch.from_numpy(m).double() / (1 - 0.9 ** 3)) / (torch.from_numpy(v).double().sqrt() / math.sqrt(1 - 0.999 ** 3) + 1e-8)
        assert abs(math.sqrt(row[2]) - float(torch.linalg.vector_norm(d))) <= 1e-13 * float(torch.linalg.vector_norm(d))
        assert row[3] == float(np.abs(g).max()) and row[4] == float(np.abs(p).max()) and not row[5:8].any()
    p, g, m, v = _case(40, 7)
    clean, _ = TO.tensor_row(p, g, m, v, 2, **HP)
    g2, p2 = g.copy(), p.copy()
    g2[[1, 2, 3]] = (np.inf, -np.inf, np.nan)
    g2[[4, 5]] = (0.0, -0.0)
    p2[9] = np.inf
    row, _ = TO.tensor_row(p2, g2, m, v, 2, **HP)
    assert row[5:8].tolist() == [3.0, 2.0, 1.0]
    keep = np.ones(40, bool)
    keep[[1, 2, 3, 4, 5]] = False
    assert row[0] == math.fsum((g[keep].astype(np.float64) ** 2).tolist()), "a planted inf must not hide the rest of the tensor"
    assert row[2] == clean[2], "d does not read g"
    assert TO.tensor_row(p, g, m, v, 2, skip=True, **HP)[0][2] == 0.0
    out, _ = TO.table_ref(p2, g2, m, v, [(0, 8), (8, 32)], 4, **HP)
    assert out[:, 8].tolist() == [4.0, 4.0] and out[:, 9].tolist() == [4.0, 4.0]
    later, _ = TO.table_ref(p, g, m, v, [(0, 8), (8, 32)], 6, prev=out, **HP)
    assert later[:, 8].tolist() == [6.0, 6.0] and later[:, 9].tolist() == [4.0, 4.0], "column 9 is sticky"


def test_other_summation_orders_stay_within_half_the_bound():
    """the gate of tests/test_clip_cpu.py: forward, reversed and pairwise sums of the same terms at <= 0.5 of every bound, from n = 64 on
    (below n = 5 one ulp of the sum is more than half the bound: _telemetry_oracle's docstring), at steps where 1 - b^t is small and
    where it is not, for unit, tiny and huge gradients"""
    C = _chunk()
    worst = 0.0
    for n in (64, 65, 1025, C + 1, 2 * C + 3):
        for step in (1, 2, 10, 1000):
            for scale in (1.0, 1e-20, 1e18):
                p, g, m, v = _case(n, n + step, scale)
                ref, bnd = TO.tensor_row(p, g, m, v, step, **HP)
                assert np.isfinite(bnd).all() and (bnd[:3] > 0).all()
                for order in ("forward", "reversed", "pairwise"):
                    alt, _ = TO.tensor_row(p, g, m, v, step, order=order, **HP)
                    ratio = np.abs(alt[:3] - ref[:3]) / bnd[:3]
                    assert (ratio <= 0.5).all(), (n, step, scale, order, ratio)
                    assert (alt[3:] == ref[3:]).all()
                    worst = max(worst, float(ratio.max()))
    print("soundness: worst err/bound over the summation orders %.4f" % worst)
    # small tensors: the full bound
    for n in (1, 2, 3, 4, 5, 63):
        p, g, m, v = _case(n, 100 + n)
        ref, bnd = TO.tensor_row(p, g, m, v, 3, **HP)
        for order in ("forward", "reversed", "pairwise"):
            alt, _ = TO.tensor_row(p, g, m, v, 3, order=order, **HP)
            assert (np.abs(alt[:3] - ref[:3]) <= bnd[:3]).all(), (n, order)
    assert TO.tensor_row(*_case(1, 1), 3, **HP)[1][:2].tolist() == [0.0, 0.0], "one element: the squares are exact"
    # the per-term bound: a handful of roundings where nothing cancels, and 1 / (1 - b2) of pow's share at the first step
    assert 10 * TO.U64 < TO.direction_rel_bound(1000, 0.9, 0.999) < 64 * TO.U64
    assert 1000 * TO.U64 < TO.direction_rel_bound(1, 0.9, 0.999) < 1e5 * TO.U64
    assert TO.direction_rel_bound(0, 0.9, 0.999) == math.inf


# ------------------------------------------------------------------ the C ABI without a device
def test_entry_points_are_declared_built_and_bound():
    from rgb_proprioceptive_pose_estimator_amd import _lib
    header = open(os.path.join(ROOT, "include", "rpe_hip.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert name in _lib._SPEC and name in _lib.EXPORTS
        assert getattr(_lib.raw, name) is not None
    assert "#define RPE_PARAM_STATS_COLS %d" % _lib.PARAM_STATS_COLS in header and _lib.PARAM_STATS_COLS == TO.COLS
    assert "#define RPE_PARAM_STATS_PART_COLS %d" % _lib.PARAM_STATS_PART_COLS in header
    assert _lib.ABI_VERSION == 3 and _lib.lib.rpe_abi_version() == 3 and "#define RPE_ABI_VERSION 3" in header


def test_param_stats_rows_is_monotone_and_device_independent():
    from rgb_proprioceptive_pose_estimator_amd import _lib, ops
    rows = _lib.lib.rpe_param_stats_rows
    assert "rpe_param_stats_rows" in _lib._NOT_STATUS
    ns = sorted(set(range(0, 20000, 7)) | {2 ** k + d for k in range(2, 41) for d in (-1, 0, 1)})
    vals = [rows(n) for n in ns]
    assert min(vals) >= 1 and vals[0] == 1 and all(a <= b for a, b in zip(vals, vals[1:]))
    assert vals == [rows(n) for n in ns], "a function of n alone"
    C = _chunk()
    assert C % 4 == 0 and rows(C) == 1 and rows(C + 1) == 2 and rows(2 * C + 3) == 3 and ops.param_stats_rows(2 * C) == 2
    assert rows(1 << 40) == (1 << 40) // C, "no cap: a row never takes more than one chunk"


def test_refusals_without_a_device():
    """the host side of the ABI checks the table before any launch: nothing here reaches a device"""
    import ctypes
    from rgb_proprioceptive_pose_estimator_amd._lib import raw
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    tab = lambda *rows: (ctypes.c_long * (3 * len(rows)))(*[x for r in rows for x in r])
    call = lambda t, T=1, every=1, p=ptr, host=True: raw.rpe_param_stats(p, ptr, ptr, ptr, ptr, ctypes.cast(t, ctypes.c_void_p) if host else None, T, ptr,
                                                                      0.9, 0.999, 1e-8, ptr, every, None)
    good = tab((0, 5, 0))
    assert call(good, T=0) == 1 and call(good, T=-1) == 1 and call(good, every=0) == 1 and call(good, p=None) == 1 and call(good, host=False) == 1
    assert call(tab((2, 5, 0))) == 3 and b"multiple of 4" in raw.rpe_last_error()
    assert call(tab((0, 5, 0), (8, 5, 2)), T=2) == 1, "first_row must be the running row count"
    assert call(tab((-4, 5, 0))) == 1 and call(tab((0, -1, 0))) == 1
    assert call(good, p=ctypes.c_void_p(ptr.value + 4)) == 3
    fin = lambda T=1, every=1, out=ptr: raw.rpe_param_stats_finalize(ptr, ptr, T, out, ptr, every, None)
    assert fin(T=0) == 1 and fin(every=0) == 1 and fin(out=None) == 1


# ------------------------------------------------------------------ table builder, optimizer, train(), script
def _toy_module():
    C = _chunk()
    torch.manual_seed(0)
    mod = torch.nn.Module()
    for name, n in (("a", 1), ("b", 7), ("c", 10), ("d", C + 5), ("e", 6)):
        mod.register_parameter(name, torch.nn.Parameter(torch.randn(n)))
    mod.c.requires_grad_(False)
    return mod, C


def test_table_builder_agrees_with_the_arena():
    from rgb_proprioceptive_pose_estimator_amd import ops
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.params import ParamArena
    mod, C = _toy_module()
    arena = ParamArena(mod)
    assert arena.offsets == [0, 4, 12, 24, 24 + C + 8]
    opt = FusedAdam([dict(params=[mod.a, mod.b, mod.c]), dict(params=[mod.d, mod.e], betas=(0.8, 0.99))], telemetry=2)
    assert opt.param_stats is None and opt.param_stats_groups() is None
    plans = opt._telemetry_plans(arena, opt._groups(arena))
    (t0, h0, part0, out0), (t1, h1, part1, out1) = plans
    assert h0.tolist() == [[0, 1, 0], [4, 7, 1]], "the frozen parameter has no row"
    assert h1.tolist() == [[24, C + 5, 0], [24 + C + 8, 6, 2]]
    assert torch.equal(t0, h0) and torch.equal(t1, h1) and h0.dtype == torch.int64
    assert tuple(part0.shape) == (2, 8) and tuple(part1.shape) == (3, 8) and part0.dtype == torch.float64
    assert tuple(opt.param_stats.shape) == (4, TO.COLS) and opt.param_stats.dtype == torch.float64 and not opt.param_stats.any()
    assert out0.data_ptr() == opt.param_stats.data_ptr() and out1.data_ptr() == opt.param_stats[2:].data_ptr()
    assert opt.param_stats_names(mod) == ["a", "b", "d", "e"] and opt.param_stats_groups() == [0, 0, 1, 1]
    assert opt._telemetry_plans(arena, opt._groups(arena)) is plans, "built once"
    opt.param_stats[:, 9] = 5.0
    opt.reset_param_stats()
    assert not opt.param_stats[:, 9].any()
    assert ops.param_stats_total_rows(h1) == 3
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.param_stats_table([(0, 3), (3, 5)])
    with pytest.raises(ValueError):
        ops.param_stats_table([])


def _params():
    torch.manual_seed(0)
    return list(torch.nn.Linear(3, 2).parameters())


def test_constructor_validation():
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam, FusedAdamW
    for cls in (FusedAdam, FusedAdamW):
        for bad in (0, -1, 1.5, "x", True):
            with pytest.raises(ValueError, match="telemetry"):
                cls(_params(), telemetry=bad)
        assert cls(_params()).telemetry is None and cls(_params(), telemetry=50).telemetry == 50
        assert cls(_params(), telemetry=1).param_stats is None


def test_state_dict_is_unchanged_by_the_option():
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    plain, tele = FusedAdam(_params(), lr=2e-3), FusedAdam(_params(), lr=5e-4, telemetry=3)
    assert set(plain.state_dict()) == set(tele.state_dict()), "telemetry is not a state_dict key"
    assert all("telemetry" not in g for g in tele.state_dict()["param_groups"])
    tele.load_state_dict(plain.state_dict())
    assert tele.telemetry == 3 and tele.param_groups[0]["lr"] == 2e-3
    other = FusedAdam(_params(), lr=5e-4, telemetry=3)
    plain.load_state_dict(other.state_dict())
    assert plain.telemetry is None and plain.param_groups[0]["lr"] == 5e-4


def test_dispatcher_entry_is_for_the_device_only():
    import rgb_proprioceptive_pose_estimator_amd.torch_ops as T
    assert "param_stats" in T.NAMES and torch.ops.rpe.param_stats.default._schema.name == "rpe::param_stats"
    z = torch.zeros(8)
    tab = torch.tensor([[0, 8, 0]])
    with pytest.raises(NotImplementedError):
        torch.ops.rpe.param_stats(z, z, z, z, tab, tab, torch.zeros(1, 8, dtype=torch.float64), torch.zeros(1, 10, dtype=torch.float64), 0.9, 0.999, 1e-8, z, 1)


def test_train_needs_an_optimizer_with_the_option():
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import telemetry_report, train
    for opt in (torch.optim.Adam(_params()), FusedAdam(_params()), FusedAdam(_params(), telemetry=2)):
        with pytest.raises(ValueError, match="telemetry"):
            train(None, None, {}, opt, 1, 1, 1, {}, "cuda:0", telemetry=1)
    with pytest.raises(ValueError, match="telemetry_log"):
        train(None, None, {}, FusedAdam(_params()), 1, 1, 1, {}, "cuda:0", telemetry_log=[])
    assert "Adam term only".lower() in telemetry_report.__doc__.lower()


def test_train_script_flags():
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam, FusedAdamW
    from rgb_proprioceptive_pose_estimator_amd.scripts.train_model import build_optimizer, build_parser
    parse = lambda *a: build_parser().parse_args(list(a))
    assert parse().telemetry is None and parse().telemetry_out is None
    assert parse("--telemetry").telemetry == 1 and parse("--telemetry", "50").telemetry == 50
    assert parse("--telemetry", "--lr", "0.01").telemetry == 1
    opt = build_optimizer(parse("--telemetry"), _params())
    assert type(opt) is FusedAdam and opt.telemetry == 1
    opt = build_optimizer(parse("--telemetry", "50", "--weight_decay", "0.02", "--telemetry_out", "t.npz"), _params())
    assert type(opt) is FusedAdamW and opt.telemetry == 50
    assert build_optimizer(parse(), _params()).telemetry is None
    with pytest.raises(SystemExit, match="telemetry"):
        build_optimizer(parse("--optimizer", "torch", "--dtype", "f32", "--telemetry"), _params())
    with pytest.raises(SystemExit, match="telemetry_out"):
        build_optimizer(parse("--telemetry_out", "t.npz"), _params())
    with pytest.raises(ValueError):
        build_optimizer(parse("--telemetry", "0"), _params())
