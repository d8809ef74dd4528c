"""Self-tests of the element-wise bound helper (tests/_bounds.py), on the CPU.

- reference: the fp64 im2col builders equal F.conv2d, its autograd gradients and F.linear for every conv shape of the op tests;
- soundness: emulated correct kernels (fp32 sums in three orders, one round-to-nearest-even into the output type) stay at
  <= 0.5 of the bound -- this is what fixes _bounds.LAM;
- power: emulated precision faults (an extra rounding, a lost term, a wrong pad pixel, truncation) are rejected, where the old
  single-number metric max|got - ref| / max|ref| passes them."""
import math

import pytest
import torch
import torch.nn.functional as F

import _bounds as B
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
