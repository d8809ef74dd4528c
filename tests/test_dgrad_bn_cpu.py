"""Self-tests of the references and bounds of the fused BN-backward epilogue of the conv data gradient (tests/_dgrad_bn_bounds.py), on
the CPU: no library, no GPU.

- soundness: a torch-fp32 restatement of the epilogue -- the conv-transpose in fp32, the addend, the gate of each mode, xhat by
  torch.addcmul(-(mean inv), y, inv), the sums per 128-row tile in fp32 -- stays at <= 0.5 of every bound on the very cases of
  tests/_dgrad_bn_cases.py (the rule test_bounds_cpu.py::test_correct_kernels_stay_within_half_the_bound fixes for LAM), and at <= 1
  over the rows of a benchmark-sized launch (256 x 56 x 56 rows, 64 columns; the maximum over many sums lies further out in the tail);
- power: each fault of FAULTS, injected into the restatement, exceeds a bound on at least one small case; the case and the ratio are
  printed beside it;
- the share of elements whose mode-2 gate the reference leaves undecided is under the cap on every case."""
import pytest
import torch
import torch.nn.functional as F

import _bounds as B
import _dgrad_bn_bounds as DB
import _dgrad_bn_cases as C

F32 = torch.float32
ROWS = C.STATS_ROWS

# fault -> (modes it applies to, 16-bit types only)
FAULTS = {
    "sums over the 16-bit-rounded dz": ((1, 2, 3, 4), True),
    "tile partials stored in 16 bits": ((1, 2, 3, 4, 5), True),
    "one 128-row half dropped": ((1, 2, 3, 4, 5), False),
    "two halves written to one row": ((1, 2, 3, 4, 5), False),
    "mean of column j used for column j+1 in the tail chunk": ((1, 2, 3, 4), False),
    "xhat without the mean term": ((1, 2, 3, 4), False),
    "gate from y > 0": ((2,), False),
    "gate bit order reversed within a byte": ((4, 5), True),
    "addend skipped where n + j >= 8 floor(N / 8)": ((1, 2, 3), False),
    "mode 5 summing the unrounded dz": ((5,), True),
}


def restate(c, mode, fwd, fault=None):
    """The epilogue in torch fp32 -> (dz [rows, in_c] in the compute type, partial sums [T, 2, in_c] fp32, plain 128-row tiles)"""
    b, h, w, ci, co, k, s, p = c["shape"]
    ho, wo = C.out_hw(c["shape"])
    oph, opw = h - ((ho - 1) * s - 2 * p + k), w - ((wo - 1) * s - 2 * p + k)
    v = F.conv_transpose2d(c["dy"].float(), c["w"].float(), None, s, p, (oph, opw)).permute(0, 2, 3, 1).reshape(-1, ci)
    if c["addend"] is not None:
        a = c["addend"].float()
        if fault == "addend skipped where n + j >= 8 floor(N / 8)":
            a = a.clone()
            a[:, ci // 8 * 8:] = 0.0
        v = v + a
    y = c["y"].float()
    if mode == 1:
        gate = fwd["a_out"].float() > 0
    elif mode == 2:
        gate = (y > 0) if fault == "gate from y > 0" else (y.double() * c["scale"].double() + c["shift"].double()).float() > 0
    elif mode == 3:
        gate = torch.ones_like(y, dtype=torch.bool)
    else:
        gate = fwd["bits"]
        if fault == "gate bit order reversed within a byte":
            gate = gate.view(-1, ci // 8, 8).flip(2).reshape(-1, ci)
    dz32 = torch.where(gate, v, torch.zeros_like(v))
    dz = dz32.to(c["dtype"])
    inv, mean = c["invstd"], c["mean"]
    if fault == "mean of column j used for column j+1 in the tail chunk":
        mean = mean.clone()
        mean[-8:] = mean[-8:].roll(1)
    cmean = torch.zeros_like(inv) if fault == "xhat without the mean term" else -(mean * inv)
    xhat = torch.addcmul(cmean.expand_as(y), y, inv.expand_as(y))
    if mode == 5:
        src = dz32 if fault == "mode 5 summing the unrounded dz" else dz.float()
        prod = torch.zeros_like(src)
    else:
        src = dz.float() if fault == "sums over the 16-bit-rounded dz" else dz32
        prod = src * xhat
    rows = src.shape[0]
    t = -(-rows // ROWS)
    pad = lambda x: torch.cat([x, torch.zeros(t * ROWS - rows, ci)]).view(t, ROWS, ci)
    part = torch.stack([pad(src).sum(1), pad(prod).sum(1)], 1)
    if fault == "tile partials stored in 16 bits":
        part = part.to(c["dtype"]).float()
    if fault == "one 128-row half dropped":
        part[0] = 0.0
    if fault == "two halves written to one row" and t > 1:
        part[0] = part[0] + part[1]
        part[1] = 0.0
    return dz, part


def ratios(c, mode, fwd, dz, part, r):
    """-> ({quantity: worst err / bound}, undecided share)"""
    checks, und = DB.judge(c, mode, fwd, dz, part, r=r)
    return {q: B.check(got, ref, bnd, q)[1] for q, got, ref, bnd, _ in checks}, und


_CASES = {}


def prepared(shape, dtype):
    """case, its fp64 data gradient and its two forwards: computed once, shared by the tests below, never modified"""
    key = (shape, dtype)
    if key not in _CASES:
        c = C.case(shape, dtype)
        _CASES[key] = (c, DB.conv_ref(c, "cpu"), {False: C.forward(c, False), True: C.forward(c, True)})
    return _CASES[key]


def every_variant():
    for path, shape in C.SHAPES + [C.TAIL_SHAPE]:
        for dtype in C.DTYPES:
            for mode, res in C.variants(shape, dtype):
                yield path, shape, dtype, mode, res


@pytest.mark.parametrize("path,shape", C.SHAPES + [C.TAIL_SHAPE])
def test_restatement_stays_within_half_the_bound(path, shape):
    for dtype in C.DTYPES:
        c, r, fwds = prepared(shape, dtype)
        for mode, res in C.variants(shape, dtype):
            dz, part = restate(c, mode, fwds[res])
            got, und = ratios(c, mode, fwds[res], dz, part, r)
            print("HALF  %-14s %s %-8s mode %d%s  %s" % (path, shape, C.name(dtype), mode, "r" if res else " ",
                                                      "  ".join("%s %.3f" % kv for kv in got.items())))
            for q, x in got.items():
                assert x <= 0.5, "%s %s %s mode %d res %s: %s at %.3f of its bound" % (path, shape, dtype, mode, res, q, x)
            if mode == 5:
                assert DB.exact_zero(part)


def test_restatement_at_benchmark_row_counts():
    """256 x 56 x 56 rows x 64 columns of synthetic dz (exact in fp32, half of it gated off; no conv needed): the fp32 tile sums of dz
    and dz xhat, totals in double, stay within 1.0 of sum_bound, the constructed 8-sigma column included"""
    rows, ci, cols = 256 * 56 * 56, 64, 8
    g = C._seed(rows, ci)
    worst = {"sum dz": 0.0, "sum dz xhat": 0.0}
    for c0 in range(0, ci, cols):
        mu = torch.full((cols,), 0.3)
        if c0 == 0:
            mu[5] = C.BIG_SIGMAS * 1.5
        y = torch.randn(rows, cols, generator=g) * 1.5 + mu
        dz = torch.randn(rows, cols, generator=g) * (torch.rand(rows, cols, generator=g) < 0.5)
        mean = y.double().mean(0).float()
        inv = (y.double().var(0, unbiased=False) + C.EPS).rsqrt().float()
        xhat = torch.addcmul((-(mean * inv)).expand_as(y), y, inv.expand_as(y))
        tsum = lambda x: x.view(rows // ROWS, ROWS, cols).sum(1).double().sum(0)
        d = dict(ref=dz.double(), eb=torch.zeros(rows, cols, dtype=torch.float64))
        s = DB.sums_ref(dict(y=y, mean=mean, invstd=inv), d, "cpu")
        worst["sum dz"] = max(worst["sum dz"], B.check(tsum(dz), *s["s1"], "")[1])
        worst["sum dz xhat"] = max(worst["sum dz xhat"], B.check(tsum(dz * xhat), *s["s2"], "")[1])
    print("BENCH rows %d: %s" % (rows, "  ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("fault", list(FAULTS))
def test_fault_is_rejected(fault):
    modes, only16 = FAULTS[fault]
    best = (0.0, None)
    big = 0.0
    for path, shape, dtype, mode, res in every_variant():
        if mode not in modes or (only16 and dtype == F32):
            continue
        c, r, fwds = prepared(shape, dtype)
        if fault.startswith("addend") and c["addend"] is None:
            continue
        dz, part = restate(c, mode, fwds[res], fault)
        checks, _ = DB.judge(c, mode, fwds[res], dz, part, r=r)
        for q, got, ref, bnd, _l in checks:
            x = B.check(got, ref, bnd, q)[1]
            if x > best[0]:
                best = (x, "%s %s %s mode %d%s: %s" % (path, shape, C.name(dtype), mode, " +res" if res else "", q))
            if fault.startswith("mode 5") and q == "sum dz":
                col = c["big"]
                big = max(big, B.check(got[col:col + 1], ref[col:col + 1], bnd[col:col + 1], q)[1])
    print("FAULT %-55s exceeds its bound %.3g times on %s" % (fault, best[0], best[1]))
    assert best[0] > 1.0, "%s is not rejected on any case (worst err / bound %.3f)" % (fault, best[0])
    if fault.startswith("mode 5"):
        print("FAULT %-55s in the constructed 8-sigma column: %.3g" % (fault, big))
        assert big > 1.0, "the constructed column does not show %s (%.3f)" % (fault, big)


def test_undecided_gates_are_under_the_cap():
    worst = 0.0
    for path, shape in C.SHAPES + [C.TAIL_SHAPE]:
        for dtype in C.DTYPES:
            c = prepared(shape, dtype)[0]
            _, und = DB.gate_ref(c, 2, None, None, "cpu")
            worst = max(worst, und)
            assert und <= C.UNDECIDED_CAP, "%s %s: %.3g of the mode-2 gates undecided" % (shape, dtype, und)
    print("UNDECIDED worst share %.3g" % worst)
