"""fp64 references, with bounds, of the on-device learning-rate schedule and the scheduled AdamW update with its weight average
(rpe_lr_schedule, rpe_adamw_step_sched), in the terms of tests/_bounds.py (class Fx: an fp64 value and a bound on the error of its
fp32 evaluation), like tests/_clip_bounds.py.

The factor is an fp64 result rounded ONCE to fp32 by the kernel: half an ulp, at most u32 relative; the bound allows 2 u32 |f| (the
half-bound gate of tests/test_sched_cpu.py) plus 8 fp64 ulps of 1 absolute: near e = T the cosine schedule forms 1 + cos(x) with cos(x)
= -1 + O(1e-16), so two correct fp64 evaluations (another cos, a fused multiply-add in the argument) differ by a few 2^-53 whatever f is
-- at f = fmin = 0 the relative term allows nothing.

The update follows _clip_bounds.adamw_clip_ref at the rate lr f with f the fp32 value the kernel reads (an exact operand): the rate and
the decay factor 1 - lr f wd are formed in double and reach the arithmetic rounded once, which is what adamw_clip_ref states for lr and
1 - lr wd.  The average's two operations on the NEW p':
    ema' = ema + (p' - ema)(1 - decay)
carry p's bound through the difference and the product, with 1 - decay a double rounded once.
References run on the device of their operands."""
import _clip_bounds as CB
from _bounds import U32, Fx

U64 = 2.0 ** -53
FACTOR_ABS = 8.0 * U64


def factor_ref(schedule, e):
    """lr_factor(schedule, e) -> Fx with the bound 2 u32 |f| + 8 * 2^-53"""
    from rgb_proprioceptive_pose_estimator_amd.optim import lr_factor
    f = lr_factor(schedule, e)
    return Fx(f, 2.0 * U32 * abs(f) + FACTOR_ABS)


def adamw_sched_ref(p, g, m, v, ema, step, factor, coef=None, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, ema_decay=None):
    """One scheduled AdamW step in fp64 from the fp32 operands -> {p, m, v[, ema]: (reference, bound)}.  factor: the fp32 value in
    sched[0], as a Python float (exact).  coef as in adamw_clip_ref.  ema / ema_decay None: no average."""
    ref = CB.adamw_clip_ref(p, g, m, v, step, coef, lr=lr * float(factor), b1=b1, b2=b2, eps=eps, wd=wd)
    if ema is not None:
        P = Fx(*ref["p"])
        E = Fx(ema.double())
        ref["ema"] = (E + (P - E) * Fx.const(1.0 - ema_decay)).out()
    return ref
