"""Self-tests of the gradient-clipping / AdamW references (tests/_clip_bounds.py) and the host side of the feature, on the CPU.

- reference: clip_ref and adamw_clip_ref equal torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW run in fp64;
- soundness: the fp32 statement of the kernels (squares and their sum in fp64, one rounding; the update as adamw_clip_kernel
  states it) stays at <= 0.5 of every bound on every input of tests/_clip_cases.py;
- power: eight wrong statements each exceed the bound at one listed input at least, at weight decay 1e-2 and 0.1;
- host: constructor validation, the two hyper-parameters through state_dict / load_state_dict (and a checkpoint without them),
  the command-line flags, the row-count function of the C ABI."""
import argparse
import math

import pytest
import torch

import _bounds as B
import _clip_bounds as CB
import _clip_cases as C

F32 = torch.float32


def _f(x):
    return torch.tensor(x, dtype=F32)


# ------------------------------------------------------------------ fp32 statements of the kernels (and wrong ones)
def clip_f32(segments, max_norm, mutant=None):
    """grad_sumsq_kernel + clip_coef_kernel: every element widened to fp64 before the square, fp64 sums, sqrt and quotient, one
    rounding to fp32 -> (norm, coef) as fp32 scalars"""
    if mutant == "squares taken in fp32":
        total = sum((s * s).double().sum() for s in segments)
    else:
        total = sum((s.double() * s.double()).sum() for s in segments)
    norm = total if mutant == "sqrt missing" else torch.sqrt(total)
    c = max_norm / (norm + (0.0 if mutant == "1e-6 missing" else 1e-6))
    coef = c if mutant == "clamp missing" else torch.where(c > 1.0, torch.ones_like(c), c)
    return norm.to(F32), coef.to(F32)


def adamw_f32(p, g, m, v, step, coef, lr, b1, b2, eps, wd, mutant=None):
    """adamw_clip_kernel's statement in torch fp32, scalars formed in double -> (p, m, v)"""
    bc1, bc2s = _f(1.0 - b1 ** step), _f(math.sqrt(1.0 - b2 ** step))
    omb1, omb2 = _f(1.0 - b1), _f(1.0 - b2)
    decay = _f(1.0 if mutant in ("no decay", "coupled L2 decay") else 1.0 - lr * wd)
    gc = g * coef
    if mutant == "coupled L2 decay":
        gc = gc + _f(wd) * p
    m = m + (gc - m) * omb1
    gv = g if mutant == "v from the unclipped gradient" else gc
    v = v * _f(b2) + gv * gv * omb2
    upd = (_f(lr) / bc1) * (m / (torch.sqrt(v) / bc2s + _f(eps)))
    if mutant == "decay after the update":
        return (p - upd) * decay, m, v
    return p * decay - upd, m, v


CLIP_MUTANTS = ["squares taken in fp32", "1e-6 missing", "clamp missing", "sqrt missing"]
ADAMW_MUTANTS = ["coupled L2 decay", "no decay", "decay after the update", "v from the unclipped gradient"]


def _ratio(got, fx):
    """err / bound of one fp32 scalar or tensor against an Fx; inf where the non-finite patterns differ"""
    ref, bnd = fx.out()
    got = got.double()
    if not torch.equal(torch.isnan(got), torch.isnan(ref)) or not torch.equal(torch.isinf(got), torch.isinf(ref)):
        return float("inf")
    if (torch.sign(got[torch.isinf(ref)]) != torch.sign(ref[torch.isinf(ref)])).any():
        return float("inf")
    fin = torch.isfinite(ref)
    return float(((got[fin] - ref[fin]).abs() / bnd[fin]).max()) if fin.any() else 0.0


def _cases():
    """(n, step, kind, max_norm) of every listed input"""
    return [(n, step, kind, mx) for n in C.CLIP_NS for step in C.STEPS for kind in C.KINDS for mx in C.max_norms(kind)]


def _ratios(n, step, kind, max_norm, wd, clip_mutant=None, adamw_mutant=None):
    """{norm, coef, p, m, v: err / bound} of the (possibly wrong) fp32 statement on one input.  The update is given the statement's
    own fp32 coefficient, as the kernel reads it from the state block, and is held to the reference that carries clip_ref's bound."""
    p, g, m, v = C.clip_case(n, step, kind)
    norm, coef = clip_f32([g], max_norm, clip_mutant)
    rn, rc = CB.clip_ref([g], max_norm)
    out = {"norm": _ratio(norm, rn), "coef": _ratio(coef, rc)}
    if clip_mutant is None:
        got = adamw_f32(p, g, m, v, step, coef, wd=wd, mutant=adamw_mutant, **C.HP)
        ref = CB.adamw_clip_ref(p, g, m, v, step, rc, wd=wd, **C.HP)
        out.update({k: B.check(t, *ref[k], k)[1] for k, t in zip("pmv", got)})
    return out


# ------------------------------------------------------------------ the references against torch in fp64
@pytest.mark.parametrize("kind", C.KINDS)
def test_references_match_torch_fp64(kind):
    """clip_ref + adamw_clip_ref == clip_grad_norm_ + AdamW on fp64 copies of the operands, three parameters (segments) at once"""
    for n in (5, 1025):
        for step in (1, 10):
            for mx in C.max_norms(kind):
                for wd in C.WDS:
                    p, g, m, v = C.clip_case(n, step, kind)
                    cuts = [0, n // 3, n // 2, n]
                    params = [torch.nn.Parameter(p[a:b].double()) for a, b in zip(cuts, cuts[1:])]
                    for q, a, b in zip(params, cuts, cuts[1:]):
                        q.grad = g[a:b].double()
                    opt = torch.optim.AdamW(params, lr=C.HP["lr"], betas=(C.HP["b1"], C.HP["b2"]), eps=C.HP["eps"], weight_decay=wd, foreach=False)
                    for q, a, b in zip(params, cuts, cuts[1:]):
                        opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=m[a:b].double(), exp_avg_sq=v[a:b].double())
                    t_norm = torch.nn.utils.clip_grad_norm_(params, mx, foreach=False)
                    opt.step()
                    rn, rc = CB.clip_ref([g[a:b] for a, b in zip(cuts, cuts[1:])], mx)
                    ref = CB.adamw_clip_ref(p, g, m, v, step, rc.v, wd=wd, **C.HP)
                    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()) + 1e-300
                    assert close(rn.v, t_norm), (kind, n, mx, float(rn.v), float(t_norm))
                    assert close(torch.cat([q.grad for q in params]), g.double() * rc.v), "coefficient"
                    assert close(ref["p"][0], torch.cat([q.data for q in params])), (kind, n, step, mx, wd)
                    assert close(ref["m"][0], torch.cat([opt.state[q]["exp_avg"] for q in params]))
                    assert close(ref["v"][0], torch.cat([opt.state[q]["exp_avg_sq"] for q in params]))


def test_clip_ref_non_finite_and_measure_only():
    """an inf element: norm inf, coefficient 0; a NaN element: both NaN (torch, error_if_nonfinite=False); zero gradients: norm 0 and
    coefficient exactly 1; max_norm None / inf: coefficient 1 whatever the norm"""
    for kind, want in (("inf", (float("inf"), 0.0)), ("nan", (float("nan"), float("nan")))):
        g = C.grad_case(1025, kind)
        q = torch.nn.Parameter(torch.zeros(1025, dtype=torch.float64))
        q.grad = g.double()
        t_norm = torch.nn.utils.clip_grad_norm_([q], 1.0, foreach=False)
        rn, rc = CB.clip_ref([g], 1.0)
        for got, t in ((rn.v, t_norm), (rc.v, torch.tensor(want[1]))):
            assert torch.equal(torch.isnan(got), torch.isnan(t)) and (torch.isnan(t) or float(got) == float(t))
        n32, c32 = clip_f32([g], 1.0)
        assert _ratio(n32, rn) == 0.0 and _ratio(c32, rc) == 0.0
    rn, rc = CB.clip_ref([C.grad_case(7, "zero")], 1e-3)
    assert float(rn.v) == 0.0 and float(rc.v) == 1.0
    for mx in (None, float("inf"), 0.0):
        assert float(CB.clip_ref([C.grad_case(7, "unit")], mx)[1].v) == 1.0


# ------------------------------------------------------------------ soundness and power
def test_fp32_statement_stays_within_half_the_bound():
    """the gate of tests/test_bounds_cpu.py: the correct fp32 statement at <= 0.5 of every bound, on every listed input and at every
    weight decay -- and not needlessly far below"""
    worst = {}
    for n, step, kind, mx in _cases():
        for wd in C.WDS:
            for k, r in _ratios(n, step, kind, mx, wd).items():
                if r > worst.get(k, (0.0,))[0]:
                    worst[k] = (r, n, step, kind, mx, wd)
    for k, w in sorted(worst.items()):
        print("soundness %-5s worst err/bound %.3f at n=%d step=%d %s max_norm=%g wd=%g" % ((k,) + w))
    bad = {k: w for k, w in worst.items() if not w[0] <= 0.5}
    assert not bad, bad
    assert max(w[0] for w in worst.values()) > 0.1, "the bounds are needlessly loose"


@pytest.mark.parametrize("mutant", CLIP_MUTANTS)
def test_clip_mutants_are_rejected(mutant):
    worst = max(max(_ratios(n, step, kind, mx, 0.0, clip_mutant=mutant).values()) for n, step, kind, mx in _cases() if step == 1)
    print("mutant clip %-24s worst err/bound %.3g" % (mutant, worst))
    assert not worst <= 1.0, mutant


@pytest.mark.parametrize("wd", [1e-2, 0.1])
@pytest.mark.parametrize("mutant", ADAMW_MUTANTS)
def test_adamw_mutants_are_rejected(mutant, wd):
    worst = max(max(_ratios(n, step, kind, mx, wd, adamw_mutant=mutant).values()) for n, step, kind, mx in _cases())
    print("mutant adamw wd=%g %-30s worst err/bound %.3g" % (wd, mutant, worst))
    assert not worst <= 1.0, mutant


def test_without_options_the_reference_is_adam_ref():
    """wd = 0 and no coefficient: the same values as _bounds.adam_ref, and a bound that is never below it (p (1 - 0) adds a product)"""
    p, g, m, v = C.clip_case(1025, 10, "unit")
    a, b = B.adam_ref(p, g, m, v, 10, **C.HP), CB.adamw_clip_ref(p, g, m, v, 10, None, wd=0.0, **C.HP)
    for k in "pmv":
        assert torch.equal(a[k][0], b[k][0]) and (b[k][1] >= a[k][1]).all()


# ------------------------------------------------------------------ host logic
def _params():
    torch.manual_seed(0)
    return list(torch.nn.Linear(3, 2).parameters())


def test_constructor_validation():
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam, FusedAdamW
    for kw in (dict(weight_decay=-1e-3), dict(weight_decay=float("nan")), dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(max_grad_norm=float("nan"))):
        for cls in (FusedAdam, FusedAdamW):
            with pytest.raises(ValueError):
                cls(_params(), **kw)
    a, w = FusedAdam(_params()), FusedAdamW(_params(), max_grad_norm=2.0)
    assert a.defaults["weight_decay"] == 0.0 and a.defaults["max_grad_norm"] is None and a.max_grad_norm is None
    assert w.defaults["weight_decay"] == torch.optim.AdamW(_params()).defaults["weight_decay"] == 1e-2
    assert isinstance(w, FusedAdam) and w.max_grad_norm == 2.0 and w.grad_norm is None and w.clip_coef is None
    assert FusedAdam(_params(), max_grad_norm=float("inf")).max_grad_norm == float("inf")     # measure only


def test_state_dict_carries_both_hyperparameters():
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam, FusedAdamW
    sd = FusedAdamW(_params(), lr=3e-4, weight_decay=0.05, max_grad_norm=0.5).state_dict()
    assert sd["param_groups"][0]["weight_decay"] == 0.05 and sd["param_groups"][0]["max_grad_norm"] == 0.5
    fresh = FusedAdam(_params())
    fresh.load_state_dict(sd)
    g = fresh.param_groups[0]
    assert (g["lr"], g["weight_decay"], g["max_grad_norm"], fresh.max_grad_norm) == (3e-4, 0.05, 0.5, 0.5)
    # a checkpoint written before the two options existed: they keep the constructor's values
    old = FusedAdam(_params(), lr=2e-3).state_dict()
    for k in ("weight_decay", "max_grad_norm"):
        del old["param_groups"][0][k]
    assert set(old["param_groups"][0]) == {"lr", "betas", "eps"}
    for opt, want in ((FusedAdam(_params()), (0.0, None)), (FusedAdamW(_params(), max_grad_norm=1.0), (1e-2, 1.0))):
        opt.load_state_dict(old)
        g = opt.param_groups[0]
        assert (g["lr"], g["weight_decay"], g["max_grad_norm"]) == (2e-3,) + want


def test_train_script_flags():
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam, FusedAdamW
    from rgb_proprioceptive_pose_estimator_amd.scripts.train_model import build_optimizer, build_parser
    parse = lambda *a: build_parser().parse_args(list(a))
    d = parse()
    assert d.max_grad_norm is None and d.weight_decay == 0.0
    opt = build_optimizer(d, _params())
    assert type(opt) is FusedAdam and opt.max_grad_norm is None and opt.defaults["weight_decay"] == 0.0
    opt = build_optimizer(parse("--max_grad_norm", "0.5"), _params())
    assert type(opt) is FusedAdam and opt.max_grad_norm == 0.5
    opt = build_optimizer(parse("--weight_decay", "0.02", "--max_grad_norm", "3", "--lr", "0.01"), _params())
    assert type(opt) is FusedAdamW and (opt.defaults["weight_decay"], opt.max_grad_norm, opt.defaults["lr"]) == (0.02, 3.0, 0.01)
    assert type(build_optimizer(parse("--optimizer", "torch", "--dtype", "f32"), _params())) is torch.optim.Adam
    opt = build_optimizer(parse("--optimizer", "torch", "--weight_decay", "0.02"), _params())
    assert type(opt) is torch.optim.AdamW and opt.defaults["weight_decay"] == 0.02
    with pytest.raises(SystemExit, match="max_grad_norm"):
        build_optimizer(parse("--optimizer", "torch", "--max_grad_norm", "1"), _params())
    with pytest.raises(SystemExit, match="f16"):
        build_optimizer(parse("--optimizer", "torch", "--dtype", "f16"), _params())
    with pytest.raises(ValueError):
        build_optimizer(parse("--max_grad_norm", "-1"), _params())
    assert isinstance(d, argparse.Namespace)


def test_grad_sumsq_rows_is_monotone_and_device_independent():
    """rpe_grad_sumsq_rows: a pure function of n (it runs here, without a device), >= 1 and monotone; ceil(n / per-block elements) up to
    a cap, which is what _clip_cases.full_pass_n reads off it"""
    from rgb_proprioceptive_pose_estimator_amd import _lib
    rows = _lib.lib.rpe_grad_sumsq_rows
    assert "rpe_grad_sumsq_rows" in _lib._NOT_STATUS
    ns = sorted(set(range(0, 5000)) | {2 ** k + d for k in range(12, 41) for d in (-1, 0, 1)})
    vals = [rows(n) for n in ns]
    assert min(vals) >= 1 and vals[0] == vals[1] == 1
    assert all(a <= b for a, b in zip(vals, vals[1:]))
    assert rows(1 << 40) == rows(1 << 50) == max(vals)
    n_full = C.full_pass_n(rows)
    assert rows(n_full) == max(vals) and n_full * 4 <= 64 << 20, "the full-pass test size must stay small"
