"""fp64 references, with element-wise bounds, of the pooling and stem-backward kernels of csrc/norm.hip.

Every reference is computed from the operands the kernel reads (never from a kernel's own output), on the device of those operands.
The bounds are built from tests/_bounds.py and tests/_norm_bounds.py as they stand -- Fx (first-order propagation through the fp32
operations), sum_bound (fp32 partial sums), out_bound (one rounding into the output type), sums_to_coeffs -- and introduce no constant:

- the max pool's forward does no arithmetic: value and winner tap are compared exactly;
- its backward adds up to five values in fp32 (the addend, then the windows that name the pixel in ascending tap order) and rounds
  once: one Fx add per value actually added, then out_bound.  A pixel that no window names is the addend, bit for bit;
- the stem backward's dz is the same gather (at most four windows), the aux head's g w[c] at its winner pixel (Fx products) and the
  ReLU mask from the sign of the fp64 pre-activation; where that sign is within the pre-activation's own fp32 error the element is
  `undecided`: its dz enters the sums' bound with its whole magnitude, and its dy is not compared;
- the stem's sums are fp32 per block of rpb pooled rows = rpb 2 W pixels (sum_bound with that many rows), the blocks meet in double;
- the average pool is one fp32 sum over HW pixels (sum_bound, one tile) times 1 / HW.

test_pool_cpu.py holds torch-fp32 restatements of the kernels to <= 0.5 of each of these, and shows the faults they reject."""
import torch

import _bounds as B
import _norm_bounds as NB
from _bounds import Fx


def pooled(n):
    return (n - 1) // 2 + 1


def _taps(x, fill):
    """x [B, H, W, C] -> [9, B, Ho, Wo, C]: tap kh * 3 + kw of every window, `fill` outside the image"""
    b, h, w, c = x.shape
    ho, wo = pooled(h), pooled(w)
    xp = x.new_full((b, 2 * ho + 1, 2 * wo + 1, c), fill)
    xp[:, 1:h + 1, 1:w + 1] = x
    return torch.stack([xp[:, kh:kh + 2 * ho:2, kw:kw + 2 * wo:2] for kh in range(3) for kw in range(3)], 0)


def _untap(v, k, h, w):
    """v [B, Ho, Wo, C] of the windows -> [B, H, W, C]: v at the pixel that is tap k of its window, 0 elsewhere"""
    b, ho, wo, c = v.shape
    p = v.new_zeros((b, 2 * ho + 1, 2 * wo + 1, c))
    p[:, k // 3:k // 3 + 2 * ho:2, k % 3:k % 3 + 2 * wo:2] = v
    return p[:, 1:h + 1, 1:w + 1]


# ------------------------------------------------------------------ max pool
def maxpool_ref(x):
    """nn.MaxPool2d(3, 2, 1) on x [B, H, W, C] (any float type) -> (out in x's type, idx uint8), exactly: the padding never wins; among
    equal values the first in-image tap in (kh, kw) order; with NaNs in the window the last NaN tap; a window of nothing but -inf names
    its first in-image tap (-inf == -inf: the same rule).  out is the winner's stored value, bit for bit.  Every element is decided:
    the comparison is on stored values, there is no tolerance."""
    v = _taps(x.double(), 0.0)
    inside = _taps(torch.ones_like(x[..., :1], dtype=torch.float64), 0.0) > 0
    k = torch.arange(9, device=x.device).view(9, 1, 1, 1, 1)
    nan = torch.isnan(v) & inside
    m = torch.where(inside & ~nan, v, torch.full_like(v, float("-inf"))).max(0).values
    first = (((v == m) & inside) * (9 - k)).argmax(0)           # the weights make the maximum unique: the smallest k
    last_nan = (nan * (k + 1)).argmax(0)
    idx = torch.where(nan.any(0), last_nan, first)
    out = _taps(x, 0.0).gather(0, idx[None])[0]
    return out, idx.to(torch.uint8)


def _gather(dout, idx, h, w, start, order=range(9)):
    """start (Fx [B, H, W, C]) plus, per pixel, dout of the windows whose idx names it, added in `order` of the taps -- an Fx add only
    where a value is added -> (Fx, named: bool [B, H, W, C])"""
    d, i = dout.double(), idx.long()
    t, named = start, torch.zeros_like(start.v, dtype=torch.bool)
    for k in order:
        hit = _untap((i == k).double(), k, h, w) > 0
        t = Fx.where(hit, t + Fx(_untap(torch.where(i == k, d, torch.zeros_like(d)), k, h, w)), t)
        named |= hit
    return t, named


def maxpool_bwd_ref(dout, idx, addend, hw, dtype):
    """rpe_maxpool3x3s2_bwd -> (reference [B, H, W, C], bound, named): named is False at the pixels no window names, which must hold
    the addend bit for bit (+0 without one)"""
    h, w = hw
    b, _, _, c = dout.shape
    zero = torch.zeros(b, h, w, c, dtype=torch.float64, device=dout.device)
    t, named = _gather(dout, idx, h, w, Fx(zero if addend is None else addend.double()))
    return t.v, NB.out_bound(t.v, t.e, dtype), named


# ------------------------------------------------------------------ stem backward
def stem_dz_ref(d):
    """dz of rpe_stem_bwd from its operands (a case of _pool_cases.stem_case, on any device) -> (dz: Fx [B, H, W, 64], undecided: bool,
    off: bool -- the mask decided off or the constructed +0: dz is exactly +0 there)"""
    y = d["y"].double()
    b, h, w, _ = y.shape
    ho, wo = h // 2, w // 2
    # (the kernel adds the own window first, then the right, lower and diagonal neighbours: descending taps)
    t, _ = _gather(d["dpool"], d["pool_idx"], h, w, Fx(torch.zeros_like(y)), order=range(8, -1, -1))
    if d["aux_dout"] is not None:
        n = ho * wo
        g = Fx(d["aux_dout"][:, :n].double().reshape(b, ho, wo, 1))
        if d["depth_feat"] is not None:
            g = g * Fx(d["depth_feat"].double().reshape(b, ho, wo, 1))
        gw = g * Fx(d["aux_w"].double())
        win = d["aux_idx"].long().reshape(b, ho, wo, 1)
        fv, fe, hit = torch.zeros_like(y), torch.zeros_like(y), torch.zeros_like(y, dtype=torch.bool)
        for k in range(4):
            m = (win == k).expand_as(gw.v)
            fv[:, k // 2::2, k % 2::2] = torch.where(m, gw.v, torch.zeros_like(gw.v))
            fe[:, k // 2::2, k % 2::2] = torch.where(m, gw.e, torch.zeros_like(gw.e))
            hit[:, k // 2::2, k % 2::2] = m
        t = Fx.where(hit, t + Fx(fv, fe), t)
    pre = Fx(y) * Fx(d["scale"].double()) + Fx(d["shift"].double())
    und = pre.v.abs() <= pre.e
    zb, zh, zw, zc = d["zero"]
    assert float(pre.v[zb, zh, zw, zc]) == 0.0 and float(pre.e[zb, zh, zw, zc]) == 0.0, "the constructed pre-activation is not exactly 0"
    und[zb, zh, zw, zc] = False
    on = pre.v > 0
    z = torch.zeros_like(y)
    dz = Fx(torch.where(on, t.v, z), torch.where(und, t.v.abs() + t.e, torch.where(on, t.e, z)))
    return dz, und, ~on & ~und


def stem_ref(d, rpb, dtype):
    """rpe_stem_bwd -> dict(dbeta, dgamma, c1, c2: Fx [64]; dy: (reference, bound); dz: Fx; undecided, off: bool [B, H, W, 64];
    plain: (reference, bound) of round_T(k1 + k2 y), what dy must be wherever dz is off)"""
    y = d["y"].double()
    b, h, w, _ = y.shape
    m = b * h * w
    dz, und, off = stem_dz_ref(d)
    mu, iv = Fx(d["mean"].double()), Fx(d["invstd"].double())
    dz2 = Fx(dz.v.reshape(m, 64), dz.e.reshape(m, 64))
    term = dz2 * ((Fx(y.reshape(m, 64)) - mu) * iv)
    rows = rpb * 2 * w
    r = NB.sums_to_coeffs(Fx(dz2.v.sum(0), B.sum_bound(dz2.v, dz2.e, rows=rows)), Fx(term.v.sum(0), B.sum_bound(term.v, term.e, rows=rows)), m)
    k0 = Fx(d["gamma"].double()) * iv
    k2 = -(k0 * iv * r["c2"])
    k1 = -(k0 * r["c1"]) - k2 * mu
    rest = k2 * Fx(y) + k1
    f = k0 * dz + rest
    r.update(dy=(f.v, NB.out_bound(f.v, f.e, dtype)), plain=(rest.v, NB.out_bound(rest.v, f.e, dtype)), dz=dz, undecided=und, off=off)
    return r


# ------------------------------------------------------------------ average pool
def avgpool_ref(x):
    """rpe_avgpool_fwd on x [B, HW, C] -> (reference [B, C], bound) of the fp32 output: one fp32 sum over the HW pixels, times 1 / HW"""
    b, hw, c = x.shape
    v = x.double().permute(1, 0, 2).reshape(hw, b * c)
    s = Fx(v.sum(0), B.sum_bound(v, torch.zeros_like(v), rows=hw))
    ref, bnd = (s * (Fx(1.0) / Fx(float(hw)))).out()
    return ref.view(b, c), bnd.view(b, c)


def avgpool_bwd_ref(dout, hw, dtype):
    """rpe_avgpool_bwd: dx [B, HW, C] = dout [B, C] * (1 / HW) in dtype -> (reference, bound)"""
    b, c = dout.shape
    f = Fx(dout.double()) * (Fx(1.0) / Fx(float(hw)))
    ref = f.v.view(b, 1, c).expand(b, hw, c).contiguous()
    return ref, NB.out_bound(ref, f.e.view(b, 1, c).expand(b, hw, c), dtype)
