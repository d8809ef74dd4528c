"""Self-tests of the element-wise bound helper (tests/_bounds.py), on the CPU.

- reference: the fp64 im2col builders equal F.conv2d, its autograd gradients and F.linear for every conv shape of the op tests;
- soundness: emulated correct kernels (fp32 sums in three orders, one round-to-nearest-even into the output type) stay at
  <= 0.5 of the bound -- this is what fixes _bounds.LAM;
- power: emulated precision faults (an extra rounding, a lost term, a wrong pad pixel, truncation) are rejected, where the old
  single-number metric max|got - ref| / max|ref| passes them."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bounds as B
import _scalar_cases as C
from oracle import pose_oracle as po
from test_gpu_ops import CONVS

OLD_TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}


def old_metric(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max()))


# ------------------------------------------------------------------ reference builders
@pytest.mark.parametrize("cfg", CONVS)
def test_reference_builders_match_torch(cfg):
    b, h, ci, co, k, s, p = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    x = torch.randn(b, ci, h, h, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(co, ci, k, k, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, s, p)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    x, w, y = x.detach(), w.detach(), y.detach()
    r = B.conv_fwd_ref(x, w, s, p)
    assert r.K == ci * k * k and _close(r.acc, y.permute(0, 2, 3, 1))
    r = B.conv_dgrad_ref(dy, w, (h, h), s, p)
    assert r.K == co * math.ceil(k / s) ** 2 and _close(r.acc, dx.permute(0, 2, 3, 1))
    r = B.conv_wgrad_ref(x, dy, k, s, p)
    assert r.K == dy.shape[0] * dy.shape[2] * dy.shape[3] and _close(r.acc, dw.permute(0, 2, 3, 1))


def test_reference_q_and_linear():
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(37, 300, generator=g, dtype=torch.float64), torch.randn(19, 300, generator=g, dtype=torch.float64)
    r = B.linear_ref(x, w)
    assert _close(r.acc, F.linear(x, w)) and r.K == 300
    prod = x[:, None, :] * w[None, :, :]
    assert _close(r.Q, (prod * prod).sum(-1).sqrt())
    assert (r.acc.abs() <= math.sqrt(r.K) * r.Q * (1 + 1e-12)).all()         # Cauchy-Schwarz
    t = B.gemm_ref_tn(x.t().contiguous(), w.t().contiguous())                  # the row-reduction form of the same product
    assert _close(t.acc, r.acc) and _close(t.Q, r.Q) and t.K == 300
    # chunked == unchunked
    old = B.CHUNK_BYTES
    try:
        B.CHUNK_BYTES = 8 * 300 * 5
        rc = B.linear_ref(x, w)
        xi = torch.randn(5, 16, 9, 9, generator=g, dtype=torch.float64)
        wi = torch.randn(8, 16, 3, 3, generator=g, dtype=torch.float64)
        fc, wc = B.conv_fwd_ref(xi, wi, 2, 1), B.conv_wgrad_ref(xi, torch.randn(5, 8, 5, 5, generator=g, dtype=torch.float64), 3, 2, 1)
    finally:
        B.CHUNK_BYTES = old
    assert _close(rc.acc, r.acc)
    assert _close(fc.acc, B.conv_fwd_ref(xi, wi, 2, 1).acc)
    assert wc.acc.shape == (8, 3, 3, 16)


# ------------------------------------------------------------------ emulated kernels
def _operands(kind, m, n, k, dtype, g):
    a, b = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g)
    if kind == "relu":             # post-ReLU activations against positive-mean weights: sums that grow with K
        a, b = F.relu(a + 0.5), b + 0.7
    q = torch.bfloat16 if dtype == torch.float32 else dtype
    if dtype != torch.float32:
        a, b = a.to(q).float(), b.to(q).float()
    return a, b


def _seq(p):
    """sequential fp32 sum over the last dim (an explicit loop: torch's CPU reductions accumulate float in double)"""
    s = torch.zeros(p.shape[:-1])
    for i in range(p.shape[-1]):
        s = s + p[..., i]
    return s


def _blocks(p, w=32):
    k = p.shape[-1]
    kp = (k + w - 1) // w * w
    pp = torch.zeros(p.shape[:-1] + (kp,))
    pp[..., :k] = p
    parts = torch.zeros(p.shape[:-1] + (kp // w,))
    for j in range(w):                                      # each 32-wide block summed in order, all blocks at once
        parts = parts + pp[..., j::w]
    return _seq(parts)


def _slabs(p, s=8):
    return _seq(torch.stack([_seq(c) for c in p.chunk(s, -1)], -1))


ORDERS = {"sequential": _seq, "blocks32": _blocks, "slabs8": _slabs}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_correct_kernels_stay_within_half_the_bound(dtype):
    g = torch.Generator().manual_seed(7)
    worst = 0.0
    for kind in ("randn", "relu"):
        for k in (36, 576, 4608, 9408):
            a, b = _operands(kind, 48, 48, k, dtype, g)
            r = B.gemm_ref(a, b)
            p = a[:, None, :] * b[None, :, :]            # fp32 products (exact for 16-bit operands)
            bnd = B.bound(r, dtype)
            for name, f in ORDERS.items():
                got = f(p).to(dtype)                     # one round-to-nearest-even into the output type
                n_bad, ratio, msg = B.check(got, r.acc, bnd, "%s K=%d %s" % (kind, k, name))
                print("soundness %-9s %-6s K=%-5d %-10s worst err/bound %.3f" % (str(dtype)[6:], kind, k, name, ratio))
                assert ratio <= 0.5, msg
                worst = max(worst, ratio)
    assert worst > 0.02, "the bound is needlessly loose (worst %.3f)" % worst


# ------------------------------------------------------------------ emulated faults
def _rne16(t, dtype):
    return t.to(dtype).double()


def _rtz_bf16(t):
    bits = t.float().view(torch.int32) & ~0xFFFF                  # drop the low 16 bits: round toward zero
    return bits.view(torch.float32).double()


def _round_bits(t, bits):
    """round-to-nearest-even to `bits` significant bits (bf16 has 8: 7 is an output that lost a bit)"""
    q = torch.exp2(torch.floor(torch.log2(t.abs().clamp_min(1e-300))) - (bits - 1))
    return torch.round(t / q) * q


def _report(name, got, ref, bnd, dtype):
    n_bad, ratio, _ = B.check(got, ref, bnd, name)
    old = old_metric(got, ref)
    bias = B.rounding_bias(got, ref, dtype, bnd) if dtype != torch.float32 and ref.numel() >= B.BIAS_MIN_ELEMS else 0.0
    once = float(B.rounding_excess(got, ref, dtype, bnd).max()) if dtype != torch.float32 else 0.0
    by = "bound" if n_bad else ("bias" if abs(bias) > B.BIAS_TOL else ("rounds-once" if once > 1.0 else "NO"))
    passes_old = [str(d)[6:] for d in (torch.bfloat16, torch.float16) if old < OLD_TOL[d]]
    print("mutant %-58s old rel_err %.2e (passes old %s bar)  new worst err/bound %8.2f  bias %+.3f  once %6.2f  rejected: %s" % (
        name, old, "/".join(passes_old) or "no", ratio, bias, once, by))
    return by != "NO"


def _wgrad_case():
    """the 1x1 weight gradient of (3, 56, 56, 64 -> 64): dW = dy^T x over 9 408 rows, bf16-exact operands, fp32 output"""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3 * 56 * 56, 64, generator=g).bfloat16().double()
    dy = torch.randn(3 * 56 * 56, 64, generator=g).bfloat16().double()
    return x, dy, B.gemm_ref_tn(dy, x)


def test_mutants_are_rejected():
    rejected = {}
    x, dy, r = _wgrad_case()
    bnd = B.bound(r, torch.float32)
    correct = (dy.float().t() @ x.float()).double()
    assert B.check(correct, r.acc, bnd, "fp32")[1] <= 0.5
    slabs = [dy[i:i + 1176].t() @ x[i:i + 1176] for i in range(0, 9408, 1176)]
    for dt in (torch.bfloat16, torch.float16):
        got = sum(_rne16(s, dt) for s in slabs)
        rejected["wgrad 1x1: 8 split-K slab partials stored in %s" % str(dt)[6:]] = _report(
            "wgrad 1x1: 8 split-K slab partials stored in %s" % str(dt)[6:], got, r.acc, bnd, torch.float32)
    run = torch.zeros(64, 64, dtype=torch.float64)
    for i in range(0, 9408, 256):
        run = _rne16(run + dy[i:i + 256].t() @ x[i:i + 256], torch.bfloat16)
    rejected["wgrad running sum"] = _report("wgrad 1x1: running sum held in bf16 every 256 rows", run, r.acc, bnd, torch.float32)
    dropped = r.acc - dy[5000:5001].t() @ x[5000:5001]
    rejected["wgrad pixel"] = _report("wgrad 1x1: one pixel dropped from the reduction", dropped, r.acc, bnd, torch.float32)

    # the forward of the same layer: y = x W^T, bf16 output, 9 408 x 64 elements
    g = torch.Generator().manual_seed(12)
    w = (torch.randn(64, 64, generator=g) / 8).bfloat16().double()
    rf = B.gemm_ref(x, w)
    bf = B.bound(rf, torch.bfloat16)
    assert B.check(_rne16(rf.acc, torch.bfloat16), rf.acc, bf, "fwd")[1] <= 0.5
    assert abs(B.rounding_bias(_rne16(rf.acc, torch.bfloat16), rf.acc, torch.bfloat16, bf)) < 0.01
    assert float(B.rounding_excess(_rne16(rf.acc, torch.bfloat16), rf.acc, torch.bfloat16, bf).max()) <= 1.0
    rejected["lost bit"] = _report("fwd 1x1 bf16: output rounded to 7 significant bits (RNE)", _round_bits(rf.acc, 7), rf.acc, bf,
                                   torch.bfloat16)
    rejected["f16 bf16"] = _report("fwd 1x1 bf16: rounded to fp16, then to bf16", _rne16(_rne16(rf.acc, torch.float16), torch.bfloat16),
                                   rf.acc, bf, torch.bfloat16)
    rejected["rtz"] = _report("fwd 1x1 bf16: output rounded toward zero", _rtz_bf16(rf.acc), rf.acc, bf, torch.bfloat16)
    # affine epilogue rounded twice: bf16(bf16(acc) * scale + shift), shifts of the accumulator's size
    scale = torch.rand(64, generator=g).double() + 0.5
    shift = torch.randn(64, generator=g).double()
    ref = rf.acc * scale + shift
    ba = B.bound(rf, torch.bfloat16, out=ref, gain=scale, epi=(rf.acc * scale).abs() + shift.abs())
    assert B.check(_rne16(ref, torch.bfloat16), ref, ba, "affine")[1] <= 0.5
    assert float(B.rounding_excess(_rne16(ref, torch.bfloat16), ref, torch.bfloat16, ba).max()) <= 1.0
    twice = _rne16(_rne16(rf.acc, torch.bfloat16) * scale + shift, torch.bfloat16)
    rejected["double"] = _report("fwd 1x1 bf16 + affine: bf16(bf16(acc) * scale + shift)", twice, ref, ba, torch.bfloat16)
    ref0 = rf.acc * scale                                          # the same without a shift: no cancellation to help
    b0 = B.bound(rf, torch.bfloat16, out=ref0, gain=scale)
    assert float(B.rounding_excess(_rne16(ref0, torch.bfloat16), ref0, torch.bfloat16, b0).max()) <= 1.0
    rejected["double no shift"] = _report("fwd 1x1 bf16 * scale: bf16(bf16(acc) * scale)", _rne16(_rne16(rf.acc, torch.bfloat16) * scale,
                                          torch.bfloat16), ref0, b0, torch.bfloat16)
    # one reduction term dropped in one 128-row tile
    drop = rf.acc.clone()
    drop[256:384] -= x[256:384, 17:18] * w[:, 17][None, :]
    rejected["tile"] = _report("fwd 1x1 bf16: one K term dropped in one 128-row tile", _rne16(drop, torch.bfloat16), rf.acc, bf, torch.bfloat16)

    # a 3x3 / pad 1 forward that reads one padded pixel (image 0, above row 0, left of column 0) as the first real pixel
    xi = torch.randn(2, 64, 14, 14, generator=g).bfloat16().double()
    wi = (torch.randn(64, 64, 3, 3, generator=g) / 24).bfloat16().double()
    rc = B.conv_fwd_ref(xi, wi, 1, 1)
    bc = B.bound(rc, torch.bfloat16)
    xp = F.pad(xi, (1, 1, 1, 1))
    xp[0, :, 0, 0] = xi[0, :, 0, 0]
    bad = F.conv2d(xp, wi).permute(0, 2, 3, 1)
    rejected["pad"] = _report("fwd 3x3 bf16: one padded tap read as a real pixel", _rne16(bad, torch.bfloat16), rc.acc, bc, torch.bfloat16)
    missed = [k for k, v in rejected.items() if not v]
    assert not missed, "mutants not rejected: %s" % missed


@pytest.mark.parametrize("rows", [4608, 200704])
def test_stats_sums(rows):
    """BN partial sums (sum_bound): a kernel summing its fp32 accumulators in 128-row tiles, the tile partials then added in fp32,
    stays at <= 0.5; summing the values rounded to 16 bits, or storing the tile partials in 16 bits, is rejected -- in bf16 and
    fp16, at a few thousand rows and at 200 704 (layer-1 rows at batch 64)."""
    g = torch.Generator().manual_seed(rows)
    a = torch.randn(rows, 576, generator=g).bfloat16().double()
    b = (torch.randn(16, 576, generator=g) / 24 + 0.02).bfloat16().double()
    r = B.gemm_ref(a, b)
    eb = B.bound(r, torch.float32)
    y = r.acc.float()                                             # the fp32 accumulators (one rounding here stands for the sum's)
    t = (rows + 127) // 128
    yp = torch.zeros(t * 128, 16)
    yp[:rows] = y

    def tiled(v, store=None):
        v = v.view(t, 128, 16)
        part = torch.zeros(t, 16)
        for i in range(128):                                      # in-tile: sequential fp32
            part = part + v[:, i]
        if store is not None:
            part = part.to(store).float()
        return _seq(part.t()).double()                            # across tiles: sequential fp32

    ref = r.acc.sum(0)
    bnd = B.sum_bound(r.acc, eb)
    ok = B.check(tiled(yp), ref, bnd, "stats")[1]
    print("stats rows=%d correct: worst err/bound %.3f" % (rows, ok))
    assert ok <= 0.5
    for dt in (torch.bfloat16, torch.float16):
        for name, got in (("values rounded to %s" % str(dt)[6:], tiled(yp.to(dt).float())),
                          ("tile partials stored in %s" % str(dt)[6:], tiled(yp, dt))):
            n_bad, ratio, _ = B.check(got, ref, bnd, name)
            print("mutant stats rows=%-6d %-36s old rel_err %.2e  new worst err/bound %8.2f" % (rows, name, old_metric(got, ref), ratio))
            assert n_bad > 0, name


def test_correct_fp32_kernel_at_benchmark_counts():
    """lam at the element counts of the GPU cases: a sequential fp32 sum (the least favourable order) of fp32 products for the
    3.2 M outputs of the fp32 resnet18 layer2.0.conv1 case at batch 32 (K = 576, 25 088 x 128)"""
    g = torch.Generator().manual_seed(3)
    a = torch.randn(25088, 576, generator=g)
    b = torch.randn(128, 576, generator=g) / 24
    r = B.gemm_ref(a, b)
    s = torch.zeros(25088, 128)
    for k in range(576):
        s += a[:, k:k + 1] * b[:, k]
    ratio = B.check(s, r.acc, B.bound(r, torch.float32), "fp32 sequential")[1]
    print("fp32 sequential, 3.2 M outputs, K = 576: worst err/bound %.3f" % ratio)
    assert ratio <= 0.5


def test_gram_stats_bound():
    """gram_stats_ref: statistics formed as the kernel does (fp32 S and s1, centred quadratic form in double) stay at <= 0.5"""
    g = torch.Generator().manual_seed(4)
    x = F.relu(torch.randn(9408, 64, generator=g) * 1.2 + 0.3).bfloat16().float()
    w = (torch.randn(256, 64, generator=g) / 8).bfloat16().double()
    gamma, beta = torch.rand(256, generator=g).double() + 0.5, torch.randn(256, generator=g).double() * 0.3
    S = (x.t() @ x).double()
    s1 = _seq(x.t()).double()
    m = x.shape[0]
    mean = (w @ s1) / m
    var = ((w @ (S - torch.outer(s1, s1) / m)) * w).sum(1) / m
    invstd = (var + 1e-5).rsqrt().float().double()
    scale = (gamma * invstd).float().double()
    got = (scale, (beta - mean * scale).float().double(), mean.float().double(), invstd)
    worst = B.assert_gram_stats(got, x.double(), w, gamma, beta, "gram stats")
    assert worst <= 0.5


# ------------------------------------------------------------------ the fp32 scalar kernels: LSTM cell, pose loss, Adam
# Plain torch-fp32 statements of the kernels (from the formulas of oracle/pose_oracle.py: lstm_forward, pose_loss, adam_update), with
# switches for the faults the bounds must reject.  Each runs on the inputs of the GPU tests (tests/_scalar_cases.py).
def lstm_fwd_f32(gates, b_ih, b_hh, c_prev, mutant=None):
    """-> (activated gates [N, 4 Hd], c, h)"""
    g = gates + b_ih if mutant == "b_hh omitted" else gates + b_ih + b_hh
    i, f, gg, o = g.chunk(4, dim=-1)
    if mutant == "f and o swapped":
        f, o = o, f
    i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
    cp = torch.zeros_like(i) if c_prev is None or mutant == "c_prev ignored" else c_prev
    c = f * cp + i * gg
    return torch.cat([i, f, gg, o], -1), c, o * torch.tanh(c)


def lstm_bwd_f32(act, c_prev, c_cur, dh, dc_in, mutant=None):
    """-> (dgates [N, 4 Hd], dc_out): the five expressions of lstm_cell_bwd_kernel"""
    gi, gf, gg, go = act.chunk(4, dim=-1)
    tc = torch.tanh(c_cur)
    dc = dh * go * (1 - tc * tc)
    if mutant != "dc_io input dropped":
        dc = dc_in + dc
    cp = torch.zeros_like(gi) if c_prev is None or mutant == "c_prev ignored" else c_prev
    dgg = dc * gi * (gg * (1 - gg) if mutant == "g (1 - g) for the g gate" else 1 - gg * gg)
    dgo = (dc if mutant == "dg[o] from dc" else dh) * tc * go * (1 - go)
    dco = dc if mutant == "dc_io written before the f multiply" else dc * gf
    return torch.cat([dc * gg * gi * (1 - gi), dc * cp * gf * (1 - gf), dgg, dgo], -1), dco


LSTM_MUTANTS = ["f and o swapped", "b_hh omitted", "c_prev ignored", "g (1 - g) for the g gate", "dc_io input dropped",
                "dc_io written before the f multiply", "dg[o] from dc"]


def _lstm_ratios(case, mutant=None):
    """worst err/bound of every output of the fp32 cell statement (forward, then backward from the CORRECT forward's outputs)"""
    hd = case["gates"].shape[1] // 4
    act, c, h = lstm_fwd_f32(case["gates"], case["b_ih"], case["b_hh"], case["c_prev"], mutant)
    ref = B.lstm_cell_fwd_ref(case["gates"], case["b_ih"], case["b_hh"], case["c_prev"])
    out = {}
    for k, name in enumerate("ifgo"):
        out["fwd " + name] = B.check(act[:, k * hd:(k + 1) * hd], *ref[name], name)[1]
    out["fwd c"], out["fwd h"] = B.check(c, *ref["c"], "c")[1], B.check(h, *ref["h"], "h")[1]
    act, c, _ = lstm_fwd_f32(case["gates"], case["b_ih"], case["b_hh"], case["c_prev"])
    dg, dco = lstm_bwd_f32(act, case["c_prev"], c, case["dh"], case["dc_in"], mutant)
    ref = B.lstm_cell_bwd_ref(act, case["c_prev"], c, case["dh"], case["dc_in"])
    for k, name in enumerate(("di", "df", "dg", "do")):
        out["bwd " + name] = B.check(dg[:, k * hd:(k + 1) * hd], *ref[name], name)[1]
    out["bwd dc"] = B.check(dco, *ref["dc"], "dc")[1]
    return out


def _lstm_cases(n, hd):
    return [C.lstm_case(n, hd, kind, wp) for kind in C.LSTM_KINDS for wp in (False, True)]


def test_lstm_reference_is_the_oracle_cell():
    """the fp64 references equal one step of oracle.lstm_forward in fp64 and its autograd gradients"""
    case = C.lstm_case(33, 64, "unit", True)
    d = {k: v.double() for k, v in case.items()}
    gates = d["gates"].clone().requires_grad_(True)
    cp = d["c_prev"].clone().requires_grad_(True)
    i, f, gg, o = (gates + d["b_ih"] + d["b_hh"]).chunk(4, dim=-1)
    c = torch.sigmoid(f) * cp + torch.sigmoid(i) * torch.tanh(gg)        # oracle/pose_oracle.py: lstm_forward
    h = torch.sigmoid(o) * torch.tanh(c)
    dgates, dcp = torch.autograd.grad([h, c], (gates, cp), [d["dh"], d["dc_in"]])
    ref = B.lstm_cell_fwd_ref(case["gates"], case["b_ih"], case["b_hh"], case["c_prev"])
    assert _close(ref["c"][0], c.detach()) and _close(ref["h"][0], h.detach())
    act = torch.cat([ref[k][0] for k in "ifgo"], -1)
    rb = B.lstm_cell_bwd_ref(act, d["c_prev"], c.detach(), d["dh"], d["dc_in"])
    assert _close(torch.cat([rb[k][0] for k in ("di", "df", "dg", "do")], -1), dgates) and _close(rb["dc"][0], dcp)


# -- pose loss
def pose_loss_f32(pred, truth, metric, mode, scale, alpha, eps, mutant=None):
    """-> (out3 fp32 [loss, val position error, val orientation error], grad [n, 7]); the sums in double, as the kernel takes them"""
    f = torch.float32
    p, t = pred.reshape(-1, 7), truth.reshape(-1, 7)
    n = p.shape[0]
    scale, alpha, eps = (torch.tensor(x, dtype=f) for x in (scale, alpha, eps))
    d = p[:, :3] - t[:, :3]
    ad = d.abs()
    sgn = torch.where(d == 0, torch.ones_like(d), torch.sign(d)) if mutant == "sign(0) = 1" else torch.sign(d)
    l2 = torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] + eps)
    g, pos = torch.zeros(n, 3), torch.zeros(n)
    if metric in (0, 3):
        pos, g = pos + l2, g + d / l2[:, None]
    if metric in (1, 3):
        pos, g = pos + ((ad[:, 0] + ad[:, 1]) + ad[:, 2]), g + sgn
    if metric in (2, 3):
        am = torch.zeros(n, dtype=torch.long)
        for k in (1, 2):
            cur = ad.gather(1, am[:, None])[:, 0]
            am = torch.where(ad[:, k] >= cur if mutant == "linf to the last index" else ad[:, k] > cur, torch.full_like(am, k), am)
        hot = F.one_hot(am, 3).float()
        pos, g = pos + (ad * hot).sum(1), g + hot * sgn
    q, tq = p[:, 3:], t[:, 3:]
    mag = torch.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    h = q / mag[:, None]
    ht = h * tq
    ip = ((ht[:, 0] + ht[:, 1]) + ht[:, 2]) + ht[:, 3]
    ori, gq = torch.zeros(n), torch.zeros(n, 4)
    if mode == 1:
        ori = (1 - ip * ip) + (-h[:, 3]).clamp_min(0)
        gh = (-2 * ip)[:, None] * tq
        gh[:, 3] -= (-h[:, 3] >= 0).float()
        if mutant == "no projection":
            gq = gh
        else:
            x = gh * h
            hd = ((x[:, 0] + x[:, 1]) + x[:, 2]) + x[:, 3]
            gq = (gh - h * hd[:, None]) / mag[:, None]
    grad = torch.cat([(scale * alpha if mutant == "alpha on the position part" else scale) * g, scale * alpha * gq], 1)
    tt = ((tq[:, 0] * tq[:, 0] + tq[:, 1] * tq[:, 1]) + tq[:, 2] * tq[:, 2]) + tq[:, 3] * tq[:, 3]
    w = (ip / tt).clamp(-1, 1).double()
    ang = torch.where(torch.sqrt(1 - w * w) != 0, 2 * torch.acos(w), torch.zeros_like(w))
    ang = torch.where(ang > np.pi, ang - 2 * np.pi, ang).abs()
    tot = (pos.double() + alpha.double() * ori.double()).sum()
    out3 = torch.stack([scale * tot.float(), l2.double().sum().float(), ang.sum().float()])
    return out3, grad


def pose_loss_autograd_f32(pred, truth, metric, mode, scale, alpha, eps):
    """the oracle's own statement in fp32, differentiated by autograd -> (loss, grad)"""
    p = pred.clone().requires_grad_(True)
    loss = po.pose_loss(p, truth, ("l2", "l1", "linf", "combined")[metric], scale, alpha, eps, ("position", "pose")[mode])
    (grad,) = torch.autograd.grad(loss, p)
    return loss.detach(), grad


POSE_MUTANTS = ["no projection", "alpha on the position part", "linf to the last index", "sign(0) = 1"]


def _pose_cases(n):
    for rot in C.POSE_ROTS:
        pred, truth = C.pose_rows(n, rot)
        for metric in C.POSE_METRICS:
            for mode in C.POSE_MODES:
                for scale, alpha in C.POSE_SCALES:
                    yield pred, truth, (metric, mode, scale, alpha, C.POSE_EPS)


def test_pose_reference_is_the_oracle_loss():
    """the fp64 reference equals oracle.pose_loss in fp64 and its autograd gradient, exact rows (ties, zeros, the clamp's edge) included"""
    for pred, truth, (metric, mode, scale, alpha, eps) in _pose_cases(257):
        p = pred.double().requires_grad_(True)
        loss = po.pose_loss(p, truth.double(), ("l2", "l1", "linf", "combined")[metric], scale, alpha, B._f32(eps), ("position", "pose")[mode])
        (grad,) = torch.autograd.grad(loss, p)
        ref = B.pose_loss_ref(pred, truth, metric, mode, scale, alpha, eps)
        assert _close(ref["out"][0][0], loss.detach()), (metric, mode)
        assert float((ref["grad"][0] - grad).abs().max()) <= 1e-9 * max(1.0, float(grad.abs().max())), (metric, mode)
    pe, oe = po.pose_loss(pred, truth, mode="val")                  # the validation sums (the oracle's are fp32 / numpy)
    ref = B.pose_loss_ref(pred, truth, 0, 1, 1.0, 1.0, 1e-4)["out"][0]
    assert abs(float(ref[1]) - float(pe)) <= 1e-5 * float(pe) and abs(float(ref[2]) - oe) <= 1e-4 * oe


# -- Adam
def adam_f32(p, g, m, v, step, lr, b1, b2, eps, mutant=None):
    """adam_kernel's statement in torch fp32, scalars formed in double -> (p, m, v)"""
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    s = step - 1 if mutant == "bias correction of step s - 1" else step
    bc1, bc2 = 1.0 - b1 ** s, 1.0 - b2 ** s
    omb1, omb2 = f(1.0 - b1), f(1.0 - b2)
    if mutant == "1 - beta in fp32":
        omb1, omb2 = f(1.0) - f(b1), f(1.0) - f(b2)
    m = m + ((g * g if mutant == "m updated with g g" else g) - m) * omb1
    v = v * f(b2) + g * g * omb2
    if mutant == "eps inside the square root":
        denom = torch.sqrt(v + f(eps)) / f(math.sqrt(bc2)) if bc2 > 0 else torch.full_like(v, float("inf"))
    else:
        with np.errstate(all="ignore"):
            denom = torch.sqrt(v) / f(bc2 if mutant == "bc2 without the square root" else math.sqrt(bc2)) + f(eps)
    return p - (f(lr) / f(bc1)) * (m / denom), m, v


def adam_torch_f32(p, g, m, v, step, lr, b1, b2, eps):
    """the oracle's statement (torch.optim.Adam's own operations) on fp32 tensors"""
    p, m, v = p.clone(), m.clone(), v.clone()
    po.adam_update(p, g, m, v, step, lr, b1, b2, eps)
    return p, m, v


ADAM_MUTANTS = ["bc2 without the square root", "eps inside the square root", "1 - beta in fp32", "bias correction of step s - 1",
                "m updated with g g"]


def _adam_ratios(fn, case, step, **kw):
    p, g, m, v = case
    got = fn(p, g, m, v, step, **C.ADAM_HP, **kw)
    ref = B.adam_ref(p, g, m, v, step, **C.ADAM_HP)
    return {k: B.check(t, *ref[k], k)[1] for k, t in zip("pmv", got)}


def _adam_cases(n):
    return [(C.adam_case(n, step, kind), step) for step in C.ADAM_STEPS for kind in C.ADAM_KINDS]


def scalar_kernel_ratios():
    """{group: worst err/bound} of the correct fp32 statements over every listed input"""
    worst = {}

    def put(group, r):
        worst[group] = max(worst.get(group, 0.0), r)

    for n, hd in C.LSTM_SHAPES:
        for case in _lstm_cases(n, hd):
            for k, r in _lstm_ratios(case).items():
                put("lstm " + ("fwd gates" if k[4:] in "ifgo" and k.startswith("fwd") else k), r)
    for n in C.POSE_NS:
        for pred, truth, args in _pose_cases(n):
            ref = B.pose_loss_ref(pred, truth, *args)
            out3, grad = pose_loss_f32(pred, truth, *args)
            put("pose grad", B.check(grad, *ref["grad"], "grad")[1])
            put("pose sums", B.check(out3, *ref["out"], "out3")[1])
            loss, grad = pose_loss_autograd_f32(pred, truth, *args)
            put("pose grad (autograd)", B.check(grad, *ref["grad"], "grad")[1])
    for n in C.ADAM_NS:
        for case, step in _adam_cases(n):
            for k, r in _adam_ratios(adam_f32, case, step).items():
                put("adam kernel form " + k, r)
            for k, r in _adam_ratios(adam_torch_f32, case, step).items():
                put("adam torch form " + k, r)
    return worst


def test_scalar_kernels_stay_within_half_the_bound():
    """fixes _bounds.TR and _bounds.EW: correct fp32 statements of the LSTM cell, the pose loss and Adam at <= 0.5 of every bound on
    every input of the GPU tests"""
    worst = scalar_kernel_ratios()
    for k, r in sorted(worst.items()):
        print("soundness %-28s worst err/bound %.3f" % (k, r))
    bad = {k: r for k, r in worst.items() if not r <= 0.5}
    assert not bad, bad
    assert max(worst.values()) > 0.1, "the bounds are needlessly loose"


@pytest.mark.parametrize("n,hd", C.LSTM_SHAPES)
def test_lstm_mutants_are_rejected(n, hd):
    for mutant in LSTM_MUTANTS:
        worst = max(max(_lstm_ratios(case, mutant).values()) for case in _lstm_cases(n, hd))
        print("mutant lstm (%d, %d) %-38s worst err/bound %.3g" % (n, hd, mutant, worst))
        assert not worst <= 1.0, mutant


@pytest.mark.parametrize("n", C.POSE_NS)
def test_pose_loss_mutants_are_rejected(n):
    for mutant in POSE_MUTANTS:
        worst = 0.0
        for pred, truth, args in _pose_cases(n):
            _, grad = pose_loss_f32(pred, truth, *args, mutant=mutant)
            worst = max(worst, B.check(grad, *B.pose_loss_ref(pred, truth, *args)["grad"], "grad")[1])
        print("mutant pose n=%d %-30s worst err/bound %.3g" % (n, mutant, worst))
        assert not worst <= 1.0, mutant


@pytest.mark.parametrize("n", C.ADAM_NS)
def test_adam_mutants_are_rejected(n):
    for mutant in ADAM_MUTANTS:
        worst = max(max(_adam_ratios(adam_f32, case, step, mutant=mutant).values()) for case, step in _adam_cases(n))
        print("mutant adam n=%d %-32s worst err/bound %.3g" % (n, mutant, worst))
        assert not worst <= 1.0, mutant


def test_amp_model_follows_the_protocol():
    """the Python model of the loss scaler (the GPU test's reference): back-off floored at 1, growth after `interval` finite steps
    capped at 2^24, skip / streak / steps as amp.py documents them"""
    st = [4.0, 0.25, 0.0, 0.0, 0.0, 0.0]
    st = C.amp_model(st, False, 2.0, 0.5, 2)
    assert st == [4.0, 0.25, 0.0, 0.0, 1.0, 1.0]
    st = C.amp_model(st, False, 2.0, 0.5, 2)
    assert st == [8.0, 0.125, 0.0, 0.0, 0.0, 2.0]
    st = C.amp_model(st, True, 2.0, 0.5, 2)
    assert st == [4.0, 0.25, 0.0, 1.0, 0.0, 2.0]
    assert C.amp_model([1.0, 1.0, 0.0, 0.0, 5.0, 7.0], True, 2.0, 0.5, 2) == [1.0, 1.0, 0.0, 1.0, 0.0, 7.0]
    assert C.amp_model([2.0 ** 24, 2.0 ** -24, 0.0, 0.0, 1.0, 7.0], False, 2.0, 0.5, 2) == [2.0 ** 24, 2.0 ** -24, 0.0, 0.0, 0.0, 8.0]
    assert C.amp_model([4.0, 0.25, 1.0, 0.0, 1.0, 3.0], False, 2.0, 0.5, 2)[:4] == [2.0, 0.5, 0.0, 1.0]    # found-inf already set
