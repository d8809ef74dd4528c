"""fp64 references, with bounds, of the gradient-norm clip and the AdamW update (rpe_grad_sumsq + rpe_clip_coef,
rpe_adamw_step_clip), in the terms of tests/_bounds.py (class Fx: an fp64 value and a bound on the error of its fp32 evaluation).

Norm and coefficient are fp64 results rounded ONCE to fp32 by the kernel (the squares are taken and summed in fp64), so their true
error is half an ulp, at most u32 relative; the bound allows 2 u32 -- headroom for the fp64 summation order and the half-bound gate of
tests/test_clip_cpu.py, not a measurement.  torch's own fp32 clip_grad_norm_ does not meet it (1.2 - 1.5 of it on N(0,1) gradients,
0 or inf where the squares leave fp32's range): it is no yardstick for the norm.

The update follows _bounds.adam_ref with G = g coef and the decayed p:
    m' = m + (G - m)(1 - b1);  v' = v b2 + G G (1 - b2);  p' = p (1 - lr wd) - (lr / bc1) (m' / (sqrt(v') / sqrt(bc2) + eps))
References run on the device of their operands."""
import math

import torch

from _bounds import U32, Fx

CLIP_EPS = 1e-6      # torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1


def clip_ref(segments, max_norm):
    """Global l2 norm of the fp32 gradient `segments` and torch's clip coefficient min(1, max_norm / (norm + 1e-6)) in fp64 ->
    (norm, coef) as Fx, each with a relative bound of 2 u32.  max_norm None, <= 0 or inf: measure only, coefficient 1.  A NaN norm
    gives a NaN coefficient and an infinite norm 0, as torch does with error_if_nonfinite=False."""
    total = sum((s.double() * s.double()).sum() for s in segments)
    norm = torch.sqrt(total)
    if max_norm is None or not max_norm > 0.0 or math.isinf(max_norm):
        coef = torch.ones_like(norm)
    else:
        coef = torch.clamp(max_norm / (norm + CLIP_EPS), max=1.0)      # (clamp keeps NaN)
    return Fx(norm, 2.0 * U32 * norm.abs()), Fx(coef, 2.0 * U32 * coef.abs())


def adamw_clip_ref(p, g, m, v, step, coef=None, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0):
    """One AdamW step on the clipped gradient in fp64 from the fp32 operands -> {p, m, v: (reference, bound)}.  coef: None (no
    clip), the fp32 value the kernel reads (exact), or clip_ref's Fx, whose bound then travels through both moments into p.  The
    decay factor 1 - lr wd is formed in double and reaches the kernel rounded once to fp32; it multiplies the OLD p."""
    P, G, M, V = Fx(p.double()), Fx(g.double()), Fx(m.double()), Fx(v.double())
    if coef is not None:
        G = G * Fx.of(coef)
    bc1, bc2s = Fx.const(1.0 - b1 ** step), Fx.const(math.sqrt(1.0 - b2 ** step))
    M, Mt = M + (G - M) * Fx.const(1.0 - b1), M * Fx.const(b1) + G * Fx.const(1.0 - b1)
    M = Fx(M.v, torch.maximum(M.e, Mt.e))          # torch's own statement m b1 + g (1 - b1) is as correct: whichever allows more
    V = V * Fx.const(b2) + G * G * Fx.const(1.0 - b2)
    upd = (Fx.const(lr) / bc1) * (M / (V.sqrt() / bc2s + Fx.const(eps)))
    return dict(p=(P * Fx.const(1.0 - lr * wd) - upd).out(), m=M.out(), v=V.out())
