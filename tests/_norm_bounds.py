"""fp64 references, with element-wise bounds, of the BatchNorm train-step kernels of csrc/norm.hip.

Every reference is computed from the operands the kernel reads (never from a kernel's own intermediate), on the device of those
operands.  The bounds are built from tests/_bounds.py as it stands -- Fx (first-order propagation through the fp32 operations, EW u32
of the magnitudes combined per operation), sum_bound (fp32 partial sums, LAM), U_OUT and FLOOR -- and introduce no constant:

- a value formed in double and stored as fp32 (the finalize functors) carries ONE operation's worth, EW u32 |v| (`_store`);
- the partial sums handed to a reduce_finalize launch are inputs and are summed in double: their fp64 sum is the reference and has no
  accumulation term;
- pass 1 of rpe_bn_backward sums in fp32: sum_bound with rows = the launcher's rows per block;
- a 16-bit output adds e_out |ref| (e_out = 2 u_out) and the type's floor: out_bound.

test_norm_cpu.py holds torch-fp32 restatements of the kernels to <= 0.5 of each of these, and shows the faults they reject."""
import torch

import _bounds as B
from _bounds import Fx


def _store(v):
    """a double rounded once into an fp32 store: one Fx operation"""
    return Fx.of(v) * 1.0


def _f32(x):
    return float(torch.tensor(float(x), dtype=torch.float32))


def out_bound(ref, e, dtype):
    """bound of a value with fp32 evaluation error e stored in dtype"""
    eo = 2.0 * B.U_OUT[dtype]
    return eo * ref.abs() + (1.0 + eo) * e + B.FLOOR[dtype]


# ------------------------------------------------------------------ finalize
def finalize_ref(part, count, gamma, beta, rm, rv, momentum, eps):
    """BnFwdFin from the partial sums [tiles, 2, C] -> {scale, shift, mean, invstd, rm, rv: (reference, bound)} (rm / rv only with
    running statistics) and `var` (fp64, clamped).  mean, var and 1 / sqrt(var + eps) are formed in double by the kernel; the fp32
    operations behind them: the stores of mean and invstd, g invstd, beta - mean scale, (1 - m) r + m v."""
    p = part.double()
    s, q = p[:, 0].sum(0), p[:, 1].sum(0)
    n = float(count)
    mean = s / n
    var = (q / n - mean * mean).clamp_min(0.0)
    invstd = _store((var + _f32(eps)).rsqrt())
    meanf = _store(mean)
    scale = Fx(gamma.double()) * invstd
    shift = Fx(beta.double()) - meanf * scale
    r = dict(scale=scale.out(), shift=shift.out(), mean=meanf.out(), invstd=invstd.out(), var=var)
    if rm is not None:
        m = _f32(momentum)
        keep = Fx(1.0) - Fx(m)
        unb = var * n / (n - 1.0) if n > 1.0 else var
        r["rm"] = (keep * Fx(rm.double()) + Fx(m) * meanf).out()
        r["rv"] = (keep * Fx(rv.double()) + Fx(m) * _store(unb)).out()
    return r


def eval_affine_ref(gamma, beta, rm, rv, eps):
    """scale = gamma / sqrtf(rv + eps), shift = beta - rm scale"""
    sc = Fx(gamma.double()) / (Fx(rv.double()) + Fx(_f32(eps))).sqrt()
    return dict(scale=sc.out(), shift=(Fx(beta.double()) - Fx(rm.double()) * sc).out())


# ------------------------------------------------------------------ apply
def apply_ref(y, scale, shift, res, res_scale, res_shift, relu, dtype):
    """out = [relu](y scale + shift (+ res | + res res_scale + res_shift)) -> dict(ref, bnd, pre (fp64 pre-activation), slack (the
    non-rounding share of the bound -- the fp32 evaluation's, without the output type's floor: the mask is taken from the fp32 value --
    where |pre| exceeds it the sign of pre is decided))"""
    t = Fx(y.double()) * Fx(scale.double())
    if res_scale is not None:
        t = (t + (Fx(shift.double()) + Fx(res_shift.double()))) + Fx(res.double()) * Fx(res_scale.double())
    elif res is not None:
        t = (t + Fx(shift.double())) + Fx(res.double())
    else:
        t = t + Fx(shift.double())
    ref = t.v.clamp_min(0.0) if relu else t.v
    bnd = out_bound(ref, t.e, dtype)
    return dict(ref=ref, bnd=bnd, pre=t.v, slack=(1.0 + 2.0 * B.U_OUT[dtype]) * t.e + B.F32_FLOOR)


def mask_errors(bits, out, r, dtype, zeros=()):
    """bits [rows, C] bool (the unpacked mask), out the kernel's output -> (wrong decided bits, set bits over a zero output whose fp64
    pre-activation is not under the type's floor, undecided elements among the random ones: `zeros` lists the constructed exact zeros,
    which have a rule of their own)"""
    decided = r["pre"].abs() > r["slack"]
    wrong = int((decided & (bits != (r["pre"] > 0))).sum())
    ghost = int((bits & (out.double() == 0) & ~(r["pre"] < B.FLOOR[dtype])).sum())
    und = ~decided
    for (row, ch) in zeros:
        und[row, ch] = False
    return wrong, ghost, int(und.sum())


# ------------------------------------------------------------------ backward
def reduce_ref(dz, y, mean, invstd, count, rpb):
    """pass 1 + 2 of rpe_bn_backward from dz (exact), y, mean, invstd -> {dbeta, dgamma, c1, c2: Fx}: the fp32 sums of dz and
    dz xhat over blocks of `rpb` rows (sum_bound), then stored / divided by count in double"""
    d = dz.double()
    term = Fx(d) * ((Fx(y.double()) - Fx(mean.double())) * Fx(invstd.double()))
    s1 = Fx(d.sum(0), B.sum_bound(d, torch.zeros_like(d), rows=rpb))
    s2 = Fx(term.v.sum(0), B.sum_bound(term.v, term.e, rows=rpb))
    return sums_to_coeffs(s1, s2, count)


def sums_to_coeffs(s1, s2, count):
    """BnBwdFin: dbeta = (float) s, dgamma = (float) q, c1 = (float)(s / count), c2 = (float)(q / count)"""
    n = float(count)
    return dict(dbeta=_store(s1), dgamma=_store(s2), c1=_store(Fx(s1.v / n, s1.e / n)), c2=_store(Fx(s2.v / n, s2.e / n)))


def coeffs_ref(part, count):
    """rpe_bn_backward_coeffs (and the first half of _from_dz): the partial sums are inputs summed in double"""
    p = part.double()
    return sums_to_coeffs(Fx(p[:, 0].sum(0)), Fx(p[:, 1].sum(0)), count)


def coeffs_t_ref(part, t, w, mean, invstd, count):
    """BnBwdFinT: s = sum of the first halves, d = rowdot(T, W) in double, q = invstd (d - mean s)"""
    s = Fx(part[:, 0].double().sum(0))
    d = Fx((t.double() * w.double()).sum(1))
    q = Fx(invstd.double()) * (d - Fx(mean.double()) * s)
    n = float(count)
    return dict(dbeta=_store(s), dgamma=_store(q), c1=_store(Fx(s.v / n, s.e / n)), c2=q * (1.0 / n))


def dy_ref(dz, y, mean, invstd, gamma, c1, c2, dtype):
    """dy = gamma invstd (dz - c1 - xhat c2) in fp64 (c1, c2: Fx -- exact when passed in, the reduction's bounds when the kernel formed
    them) -> (reference, bound).  The bound follows the streaming form k0 dz + (k2 y + k1), k0 = gamma invstd, k2 = -k0 invstd c2,
    k1 = -k0 c1 - k2 mean: |k2 y| and |k2 mean| enter separately, which also covers the generic pass 3."""
    g, i, mu = Fx(gamma.double()), Fx(invstd.double()), Fx(mean.double())
    k0 = g * i
    k2 = -(k0 * i * c2)
    k1 = -(k0 * c1) - k2 * mu
    f = k0 * Fx(dz.double()) + (k2 * Fx(y.double()) + k1)
    ref = gamma.double() * invstd.double() * (dz.double() - c1.v - (y.double() - mean.double()) * invstd.double() * c2.v)
    return ref, out_bound(ref, f.e, dtype)
