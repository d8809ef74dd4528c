"""Self-tests of the learning-rate schedule / weight-average references (tests/_sched_bounds.py) and the host side of the feature,
on the CPU.

- rule: optim.lr_factor equals torch's own schedulers (LinearLR, SequentialLR + CosineAnnealingLR, StepLR, ConstantLR) stepped on a
  one-parameter torch.optim.Adam, for every kind x configuration of tests/_sched_cases.py at every e in 0 .. T; beyond T the cosine
  holds fmin; the average's reference equals torch.optim.swa_utils.get_ema_multi_avg_fn in fp64;
- soundness: the fp32 statements of the kernels stay at <= 0.5 of every bound, and the bounds are not needlessly loose;
- power: eight wrong statements are each rejected;
- host: constructor validation, state_dict with and without the new keys, the param-group key set, one global max_grad_norm,
  ParamArena.trainable_segments(params), the command-line flags, util.model_utils.lr_param_groups."""
import math
import warnings

import pytest
import torch

import _bounds as B
import _sched_bounds as SB
import _sched_cases as S

F32 = torch.float32


def _f(x):
    return torch.tensor(x, dtype=F32)


# ------------------------------------------------------------------ the rule against torch's schedulers
def _torch_factors(kind, cfg):
    """lr / base lr of a one-parameter Adam under torch's schedulers after e = 0 .. T scheduler steps"""
    W, s, T, fmin, step_size, gamma = cfg
    base = 0.5
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=base)
    L = torch.optim.lr_scheduler
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if kind == "cosine":
            main = L.CosineAnnealingLR(opt, T_max=T - W, eta_min=fmin * base)
        elif kind == "step":
            main = L.StepLR(opt, step_size=step_size, gamma=gamma)
        else:
            main = L.ConstantLR(opt, factor=1.0, total_iters=1)
        sched = main if W == 0 else L.SequentialLR(opt, [L.LinearLR(opt, start_factor=s, total_iters=W), main], milestones=[W])
        out = []
        for e in range(T + 1):
            out.append(opt.param_groups[0]["lr"] / base)
            opt.step()
            sched.step()
    return out


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("cfg", S.CONFIGS)
def test_lr_factor_is_torchs_rule(kind, cfg):
    from rgb_proprioceptive_pose_estimator_amd.optim import lr_factor
    sch = S.schedule(kind, cfg)
    want = _torch_factors(kind, cfg)
    worst = 0.0
    for e, w in enumerate(want):
        got = lr_factor(sch, e)
        if w == 0.0:
            assert abs(got) <= 1e-14, (kind, cfg, e, got)
        else:
            worst = max(worst, abs(got - w) / abs(w))
            assert abs(got - w) <= 1e-14 * abs(w), (kind, cfg, e, got, w)
    print("rule %-8s %s worst relative difference %.2e" % (kind, cfg, worst))
    W, T, fmin = cfg[0], cfg[2], cfg[3]
    if kind == "cosine":       # beyond T it holds fmin (torch's recursion does not: the difference is deliberate)
        for e in (T, T + 1, T + 2, 2 * T - W, 2 * T, T + 1000):
            assert lr_factor(sch, e) == lr_factor(sch, T) and abs(lr_factor(sch, e) - fmin) <= 1e-15
    if W:
        assert lr_factor(sch, 0) == cfg[1]
    with pytest.raises(ValueError):
        lr_factor(sch, -1)


@pytest.mark.parametrize("decay", S.EMA_DECAYS)
def test_average_reference_is_torchs_ema(decay):
    from torch.optim.swa_utils import get_ema_multi_avg_fn
    p, g, m, v, ema = S.sched_case(1025, 10)
    ref = SB.adamw_sched_ref(p, g, m, v, ema, 10, 1.0, ema_decay=decay, **S.HP)
    avg = [ema.double().clone()]
    get_ema_multi_avg_fn(decay)(avg, [ref["p"][0]], None)
    assert float((avg[0] - ref["ema"][0]).abs().max()) <= 1e-14


# ------------------------------------------------------------------ fp32 statements of the kernels (and wrong ones)
def factor_f32(sch, e, mutant=None):
    """lr_schedule_kernel: the closed form in fp64, one rounding to fp32"""
    W, s, T, fmin = sch.warmup_steps, sch.warmup_start_factor, sch.total_steps, sch.min_factor
    if mutant == "e off by one":
        e = e + 1
    if mutant == "start factor ignored":
        s = 0.0
    if e < W:
        f = s + (1.0 - s) * e / W
    elif sch.kind == "cosine":
        ec = e if mutant == "cosine not clamped" else min(e, T)
        f = fmin + (1.0 - fmin) * (1.0 + math.cos(math.pi * (ec - W) / (T - W))) / 2.0
    elif sch.kind == "step":
        k = round((e - W) / sch.step_size) if mutant == "round for the floor" else (e - W) // sch.step_size
        f = sch.gamma ** k
    else:
        f = 1.0
    return torch.tensor(f, dtype=torch.float64).to(F32)


def sched_f32(p, g, m, v, ema, step, factor, lr, b1, b2, eps, wd, ema_decay, mutant=None):
    """adamw_sched_kernel's statement in torch fp32, scalars formed in double -> (p, m, v, ema)"""
    lr_eff = lr * float(factor)
    bc1, bc2s = _f(1.0 - b1 ** step), _f(math.sqrt(1.0 - b2 ** step))
    decay = _f(1.0 - (lr if mutant == "factor missing from the decay" else lr_eff) * wd)
    m2 = m + (g - m) * _f(1.0 - b1)
    v2 = v * _f(b2) + g * g * _f(1.0 - b2)
    p2 = p * decay - (_f(lr_eff) / bc1) * (m2 / (torch.sqrt(v2) / bc2s + _f(eps)))
    src = p if mutant == "average from the old p" else p2
    omd = _f(ema_decay if mutant == "decay and 1 - decay exchanged" else 1.0 - ema_decay)
    return p2, m2, v2, ema + (src - ema) * omd


FACTOR_MUTANTS = ["e off by one", "start factor ignored", "cosine not clamped", "round for the floor"]
UPDATE_MUTANTS = ["factor missing from the decay", "average from the old p", "decay and 1 - decay exchanged"]
F37 = float(_f(S.FACTOR))


def _factor_ratio(kind, cfg, e, mutant=None):
    sch = S.schedule(kind, cfg)
    ref, bnd = SB.factor_ref(sch, e).out()
    return float((factor_f32(sch, e, mutant).double() - ref).abs() / bnd)


def _factor_cases():
    return [(kind, cfg, e) for kind in S.KINDS for cfg in S.CONFIGS for e in sorted(set(range(cfg[2] + 4)) | {cfg[2] + 1000})]


def _update_ratios(n, step, wd, decay, mutant=None):
    p, g, m, v, ema = S.sched_case(n, step)
    got = sched_f32(p, g, m, v, ema, step, F37, wd=wd, ema_decay=decay, mutant=mutant, **S.HP)
    ref = SB.adamw_sched_ref(p, g, m, v, ema, step, F37, wd=wd, ema_decay=decay, **S.HP)
    return {k: B.check(t, *ref[k], k)[1] for k, t in zip(("p", "m", "v", "ema"), got)}


def _update_cases():
    return [(n, step, wd, d) for n in (5, 1025) for step in S.STEPS for wd in S.WDS for d in S.EMA_DECAYS]


def test_fp32_statements_stay_within_half_the_bound():
    worst = {"factor": max(_factor_ratio(*c) for c in _factor_cases())}
    for c in _update_cases():
        for k, r in _update_ratios(*c).items():
            worst[k] = max(worst.get(k, 0.0), r)
    for k, w in sorted(worst.items()):
        print("soundness %-6s worst err/bound %.3f" % (k, w))
    assert all(w <= 0.5 for w in worst.values()), worst
    assert min(worst.values()) > 0.1, "a bound is needlessly loose: %s" % worst


def test_factor_one_without_average_is_the_clip_reference():
    """factor 1: the values and bounds of _clip_bounds.adamw_clip_ref (the kernel is then bit-identical to rpe_adamw_step_clip)"""
    import _clip_bounds as CB
    p, g, m, v, _ = S.sched_case(1025, 10)
    a, b = CB.adamw_clip_ref(p, g, m, v, 10, None, wd=1e-2, **S.HP), SB.adamw_sched_ref(p, g, m, v, None, 10, 1.0, wd=1e-2, **S.HP)
    assert set(b) == {"p", "m", "v"}
    for k in "pmv":
        assert torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1])


@pytest.mark.parametrize("mutant", FACTOR_MUTANTS)
def test_factor_mutants_are_rejected(mutant):
    worst = max(_factor_ratio(*c, mutant=mutant) for c in _factor_cases())
    print("mutant factor %-24s worst err/bound %.3g" % (mutant, worst))
    assert not worst <= 1.0, mutant


@pytest.mark.parametrize("mutant", UPDATE_MUTANTS)
def test_update_mutants_are_rejected(mutant):
    worst = max(max(_update_ratios(*c, mutant=mutant).values()) for c in _update_cases() if c[2] > 0.0)
    print("mutant update %-32s worst err/bound %.3g" % (mutant, worst))
    assert not worst <= 1.0, mutant


@pytest.mark.parametrize("mutant", [None, "group 1 updated with group 0's rate"])
def test_two_groups_each_at_its_own_rate(mutant):
    """two groups (lr 1e-3 / 1e-4, wd 0 / 1e-2) over the halves of one buffer: the statement that gives each group its own rate is
    within the bounds; the one that updates group 1 with group 0's rate is not"""
    n, step = 1025, 10
    p, g, m, v, ema = S.sched_case(n, step)
    groups = [(slice(0, 512), 1e-3, 0.0), (slice(512, n), 1e-4, 1e-2)]
    worst = 0.0
    for sl, lr, wd in groups:
        hp = dict(S.HP, lr=groups[0][1] if mutant else lr)
        got = sched_f32(p[sl], g[sl], m[sl], v[sl], ema[sl], step, F37, wd=wd, ema_decay=0.9, **hp)
        ref = SB.adamw_sched_ref(p[sl], g[sl], m[sl], v[sl], ema[sl], step, F37, wd=wd, ema_decay=0.9, **dict(S.HP, lr=lr))
        worst = max(worst, max(B.check(t, *ref[k], k)[1] for k, t in zip(("p", "m", "v", "ema"), got)))
    assert (worst <= 0.5) if mutant is None else (not worst <= 1.0), worst


# ------------------------------------------------------------------ host logic
def _params():
    torch.manual_seed(0)
    return list(torch.nn.Linear(3, 2).parameters())


BAD_SCHEDULES = [dict(kind="linear"), dict(warmup_steps=-1), dict(warmup_steps=1.5), dict(warmup_start_factor=-0.1), dict(warmup_start_factor=1.1),
                 dict(kind="cosine"), dict(kind="cosine", warmup_steps=5, total_steps=5), dict(kind="cosine", total_steps=7.0),
                 dict(min_factor=-0.1), dict(min_factor=1.5), dict(kind="step"), dict(kind="step", step_size=0), dict(step_size=0),
                 dict(gamma=0.0), dict(gamma=1.5), dict(gamma=float("nan")), dict(warmup_start_factor=float("nan"))]


@pytest.mark.parametrize("kw", BAD_SCHEDULES, ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_schedule_validation(kw):
    from rgb_proprioceptive_pose_estimator_amd.optim import LRSchedule
    with pytest.raises(ValueError):
        LRSchedule(**kw)


def test_schedule_is_a_value_object():
    from rgb_proprioceptive_pose_estimator_amd.optim import LRSchedule
    d = LRSchedule()
    assert d.state_dict() == dict(kind="constant", warmup_steps=0, warmup_start_factor=0.1, total_steps=None, min_factor=0.0, step_size=None, gamma=0.1)
    a = LRSchedule("cosine", warmup_steps=3, warmup_start_factor=0.2, total_steps=10, min_factor=0.05)
    b = LRSchedule()
    assert a != b
    b.load_state_dict(a.state_dict())
    assert a == b and "cosine" in repr(b)
    with pytest.raises(ValueError):
        b.load_state_dict(dict(a.state_dict(), gamma=2.0))
    assert a.c_args() == (1, 3, 0.2, 10, 0.05, 1, 0.1)
    assert LRSchedule("step", step_size=4, gamma=0.5).c_args() == (2, 0, 0.1, 0, 0.0, 4, 0.5)


def test_constructor_validation():
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam, FusedAdamW, LRSchedule
    for kw in (dict(ema_decay=-0.1), dict(ema_decay=1.0), dict(ema_decay=float("nan")), dict(lr_schedule="cosine"), dict(lr_schedule=dict(kind="cosine"))):
        for cls in (FusedAdam, FusedAdamW):
            with pytest.raises(ValueError):
                cls(_params(), **kw)
    a = FusedAdam(_params())
    assert a.lr_schedule is None and a.ema_decay is None and a.lr_factor is None and a.steps_scheduled is None and a.ema_parameters() is None
    sch = LRSchedule("step", step_size=2)
    w = FusedAdamW(_params(), lr_schedule=sch, ema_decay=0.0)
    assert w.lr_schedule is sch and w.ema_decay == 0.0 and w.defaults["weight_decay"] == 1e-2
    with pytest.raises(RuntimeError, match="ema_decay"):
        with a.averaged_weights():
            pass


def test_new_options_stay_out_of_the_param_groups():
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam, LRSchedule
    opt = FusedAdam(_params(), lr_schedule=LRSchedule(warmup_steps=2), ema_decay=0.99)
    assert set(opt.param_groups[0]) - {"params"} == {"lr", "betas", "eps", "weight_decay", "max_grad_norm"}
    assert set(opt.defaults) == {"lr", "betas", "eps", "weight_decay", "max_grad_norm"}
    assert set(opt.state_dict()["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "max_grad_norm"}


def test_state_dict_round_trip():
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam, LRSchedule
    sch = LRSchedule("cosine", warmup_steps=2, total_steps=9, min_factor=0.1)
    opt = FusedAdam(_params(), lr_schedule=sch, ema_decay=0.9)
    opt._ema = torch.arange(8.0)
    sd = opt.state_dict()
    assert sd["lr_schedule"] == sch.state_dict() and torch.equal(sd["ema"], torch.arange(8.0))
    fresh = FusedAdam(_params(), ema_decay=0.5)
    fresh.load_state_dict(sd)
    assert fresh.lr_schedule == sch and fresh.lr_schedule is not sch and fresh.ema_decay == 0.5
    assert torch.equal(fresh._ema, torch.arange(8.0)) and fresh._ema is not sd["ema"]
    # without the options there are no such keys, and a checkpoint without them keeps the constructor's values
    plain = FusedAdam(_params()).state_dict()
    assert "lr_schedule" not in plain and "ema" not in plain
    keep = FusedAdam(_params(), lr_schedule=sch, ema_decay=0.9)
    keep._ema = torch.ones(8)
    keep.load_state_dict(plain)
    assert keep.lr_schedule is sch and keep.ema_decay == 0.9 and keep._ema is None      # the average restarts from the weights
    # an optimizer without an average ignores a saved one
    none = FusedAdam(_params())
    none.load_state_dict(sd)
    assert none._ema is None and none.ema_decay is None and none.lr_schedule == sch


def test_max_grad_norm_is_one_global_norm():
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    w, b = _params()
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdam([{"params": [w], "max_grad_norm": 1.0}, {"params": [b]}])
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdam([{"params": [w], "max_grad_norm": 1.0}, {"params": [b], "max_grad_norm": 2.0}], max_grad_norm=1.0)
    opt = FusedAdam([{"params": [w], "lr": 1e-4}], lr=1e-3, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.add_param_group({"params": [b], "max_grad_norm": 0.5})
    assert len(opt.param_groups) == 1
    with pytest.raises(ValueError):
        opt.add_param_group({"params": [b], "weight_decay": -1.0})
    opt.add_param_group({"params": [b], "weight_decay": 0.1})
    assert [g["lr"] for g in opt.param_groups] == [1e-4, 1e-3] and [g["max_grad_norm"] for g in opt.param_groups] == [1.0, 1.0]
    assert opt.max_grad_norm == 1.0


def test_trainable_segments_of_some_parameters():
    """interleaved, frozen and odd-length parameters: sizes 1, 7, 10, 33, 4, 5 at offsets 0, 4, 12, 24, 60, 64; the third frozen"""
    from rgb_proprioceptive_pose_estimator_amd.params import ParamArena
    mod = torch.nn.Module()
    for name, n in (("a", 1), ("b", 7), ("c", 10), ("d", 33), ("e", 4), ("f", 5)):
        mod.register_parameter(name, torch.nn.Parameter(torch.randn(n)))
    mod.c.requires_grad_(False)
    arena = ParamArena(mod)
    assert arena.offsets == [0, 4, 12, 24, 60, 64] and arena.numel == 72
    assert arena.trainable_segments() == arena.trainable_segments(None) == [(0, 12), (24, 72)]
    assert arena.trainable_segments(list(mod.parameters())) == [(0, 12), (24, 72)]
    assert arena.trainable_segments([mod.a, mod.d, mod.f]) == [(0, 4), (24, 60), (64, 72)]       # interleaved: nothing merges across b and e
    assert arena.trainable_segments([mod.e, mod.b]) == [(4, 12), (60, 64)]                        # arena order, whatever the list's
    assert arena.trainable_segments([mod.b, mod.c]) == [(4, 12)] and arena.trainable_segments([mod.c]) == []
    assert arena.trainable_segments([mod.d, mod.e, mod.f]) == [(24, 72)] and arena.trainable_segments([]) == []
    with pytest.raises(ValueError):
        arena.trainable_segments([torch.nn.Parameter(torch.zeros(3))])
    a, b = arena.trainable_segments([mod.a, mod.b]), arena.trainable_segments([mod.d, mod.e, mod.f])
    assert sorted(a + b) == arena.trainable_segments()


def test_train_script_flags():
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam, FusedAdamW, LRSchedule
    from rgb_proprioceptive_pose_estimator_amd.scripts.train_model import build_optimizer, build_parser
    parse = lambda *a: build_parser().parse_args(list(a))
    d = parse()
    for flag in ("lr_schedule", "warmup_steps", "warmup_start_factor", "lr_total_steps", "lr_min_factor", "lr_step_size", "lr_gamma", "trunk_lr_scale", "ema_decay"):
        assert getattr(d, flag) is None, flag
    opt = build_optimizer(d, _params())
    assert type(opt) is FusedAdam and opt.lr_schedule is None and opt.ema_decay is None and len(opt.param_groups) == 1
    opt = build_optimizer(parse("--lr_schedule", "cosine", "--warmup_steps", "5", "--warmup_start_factor", "0.2", "--lr_total_steps", "50",
                                "--lr_min_factor", "0.01", "--ema_decay", "0.99", "--weight_decay", "0.02"), _params())
    assert type(opt) is FusedAdamW and opt.ema_decay == 0.99
    assert opt.lr_schedule == LRSchedule("cosine", warmup_steps=5, warmup_start_factor=0.2, total_steps=50, min_factor=0.01)
    opt = build_optimizer(parse("--lr_schedule", "step", "--lr_step_size", "7", "--lr_gamma", "0.5"), _params())
    assert opt.lr_schedule == LRSchedule("step", step_size=7, gamma=0.5) and opt.ema_decay is None
    assert build_optimizer(parse("--warmup_steps", "3"), _params()).lr_schedule == LRSchedule("constant", warmup_steps=3)
    # group dicts: lr_scale becomes lr * scale, and is no key of the group
    w, b = _params()
    opt = build_optimizer(parse("--lr", "0.01"), [{"params": [w], "lr_scale": 0.1}, {"params": [b]}])
    assert [g["lr"] for g in opt.param_groups] == [pytest.approx(1e-3), 0.01]
    assert all(set(g) - {"params"} == {"lr", "betas", "eps", "weight_decay", "max_grad_norm"} for g in opt.param_groups)
    flags = {"lr_schedule": "constant", "warmup_steps": "2", "warmup_start_factor": "0.5", "lr_total_steps": "9", "lr_min_factor": "0.1",
             "lr_step_size": "2", "lr_gamma": "0.5", "trunk_lr_scale": "0.1", "ema_decay": "0.9"}
    for flag, value in flags.items():
        with pytest.raises(SystemExit, match=flag):
            build_optimizer(parse("--optimizer", "torch", "--dtype", "f32", "--" + flag, value), _params())
    with pytest.raises(SystemExit, match="lr_total_steps"):
        build_optimizer(parse("--lr_schedule", "cosine"), _params())
    with pytest.raises(SystemExit, match="lr_step_size"):
        build_optimizer(parse("--lr_schedule", "step"), _params())
    with pytest.raises(ValueError):
        build_optimizer(parse("--ema_decay", "1.0"), _params())
    with pytest.raises(ValueError):
        build_optimizer(parse("--lr_schedule", "cosine", "--lr_total_steps", "3", "--warmup_steps", "3"), _params())


def test_lr_param_groups_partition_the_parameters():
    from _helpers import CASES, build
    from rgb_proprioceptive_pose_estimator_amd.util.model_utils import lr_param_groups
    for kind in ("no", "td"):
        model = build(kind, CASES[kind][0], torch.float32)
        params = list(model.parameters())
        for scale in (None, 1, 1.0):
            plain = lr_param_groups(model, scale)
            assert len(plain) == len(params) and all(a is b for a, b in zip(plain, params))
        groups = lr_param_groups(model, 0.1)
        assert len(groups) == 2 and groups[0]["lr_scale"] == 0.1 and set(groups[0]) == {"params", "lr_scale"} and set(groups[1]) == {"params"}
        ids = [id(p) for g in groups for p in g["params"]]
        assert len(ids) == len(set(ids)) and sorted(ids) == sorted(id(p) for p in params)       # exactly once, nothing else
        trunk = {id(p) for p in model.trunk.parameters()}
        assert {id(p) for p in groups[0]["params"]} == trunk and not trunk & {id(p) for p in groups[1]["params"]}
        assert groups[1]["params"], "the heads / fc tail form the second group"
        with pytest.raises(ValueError):
            lr_param_groups(model, 0.0)
