"""Self-tests of the BatchNorm references and bounds (tests/_norm_bounds.py), on the CPU: no library, no GPU.

- soundness: torch-fp32 restatements of the kernels of csrc/norm.hip in the kernels' own association -- the slices and row lanes of
  reduce_finalize_kernel in double and its functors in fp32, the fma order of bn_apply_kernel, per-thread strided rows then the RPI
  partials then double across blocks for pass 1, the generic pass 3 and the k0 / k1 / k2 form of the streaming one -- stay at <= 0.5 of
  every bound on the very cases of tests/_norm_cases.py (fp16 results under the smallest normal: <= 1, the floor IS their rounding);
- power: each fault of MUTANTS, injected into a restatement, is rejected by a bound or an exact check on at least one case; printed
  beside it on how many of those cases max|err| / max|ref| at the bars of test_bn_train_fwd_bwd (2e-5 / 2e-2 / 3e-3 forward, 5e-5 /
  3e-2 backward, 1e-5 for the statistics) passes it, i.e. would not have noticed."""
import torch

import _bounds as B
import _norm_bounds as NB
import _norm_cases as C

F32 = torch.float32
OLD_FWD = {F32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}
OLD_BWD = {F32: 5e-5, torch.bfloat16: 3e-2, torch.float16: 3e-2}
OLD_STATS = 1e-5

MUTANTS = ["neighbouring chunk's coefficients in the last partial span", "one row per block left out of pass 1",
           "last slice's tiles left out of finalize", "finalize summing in fp32", "variance without the clamp", "biased running variance",
           "momentum on the wrong operand", "mask from the rounded output", "output rounded twice", "output truncated",
           "res_bn shift dropped", "c2 scaled by invstd once too few", "dz mask a_out >= 0", "trailing slab dropped"]


def old_metric(got, ref):
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    if not bool(torch.isfinite(got).all()):
        return float("inf")          # rel_err asserts finiteness
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12))


def _fma(a, b, c):
    """fmaf through double: the product of two fp32 is exact in 53 bits"""
    return (a.double() * b.double() + c.double()).float()


def _rtz(t, dtype):
    r = t.to(dtype)
    away = r.float().abs() > t.abs()
    bits = r.view(torch.int16)
    return torch.where(away, bits - 1, bits).view(dtype)


def _ratio(got, ref, bnd, mask=None):
    if mask is not None:
        got, ref, bnd = got[mask], ref[mask], bnd[mask]
    return B.check(got, ref, bnd, "")[1] if ref.numel() else 0.0


def _normal(ref, dtype):
    return ref.abs() >= (2.0 ** -14 if dtype == torch.float16 else 2.0 ** -126)


# ------------------------------------------------------------------ restatements
def slice_sums(col, ns, mutant=None):
    """col [tiles, C] fp32 -> the sums of reduce_finalize_kernel: slice s takes tiles s, s + NS, ..., its 8 row lanes every 8th of
    those, in double; the lanes then the slices are added in order"""
    tiles, c = col.shape
    acc = torch.float32 if mutant == "finalize summing in fp32" else torch.float64
    pad = -(-tiles // (8 * ns)) * 8 * ns
    v = torch.zeros(pad, c, dtype=acc)
    v[:tiles] = col.to(acc)
    v = v.view(-1, 8, ns, c)                       # tile t = (k * 8 + lane) * NS + slice
    lanes = torch.zeros(8, ns, c, dtype=acc)
    for k in range(v.shape[0]):
        lanes = lanes + v[k]
    sl = lanes[0]
    for i in range(1, 8):
        sl = sl + lanes[i]                         # [NS, C]
    if mutant == "last slice's tiles left out of finalize" and ns > 1:
        sl = sl[:-1]
    tot = sl[0]
    for i in range(1, sl.shape[0]):
        tot = tot + sl[i]
    return tot.double()


def finalize_f32(case, momentum, running=True, mutant=None):
    part, n = case["part"], float(case["count"])
    ns = C.reduce_slices(part.shape[0], part.shape[2])
    s, q = slice_sums(part[:, 0], ns, mutant), slice_sums(part[:, 1], ns, mutant)
    mean = s / n
    var = q / n - mean * mean
    if mutant != "variance without the clamp":
        var = var.clamp_min(0.0)
    invstd = (1.0 / (var + float(torch.tensor(C.EPS, dtype=F32))).sqrt()).float()
    sc = case["gamma"] * invstd
    meanf = mean.float()
    out = dict(scale=sc, shift=_fma(-meanf, sc, case["beta"]), mean=meanf, invstd=invstd)
    if running:
        unb = var if (n <= 1.0 or mutant == "biased running variance") else var * n / (n - 1.0)
        m = torch.tensor(momentum, dtype=F32)
        a, b = ((1.0 - m), m) if mutant != "momentum on the wrong operand" else (m, (1.0 - m))
        out["rm"] = a * case["rm"] + b * meanf
        out["rv"] = a * case["rv"] + b * unb.float()
    return out


def eval_affine_f32(case):
    sc = case["gamma"] / (case["rv"] + torch.tensor(C.EPS, dtype=F32)).sqrt()
    return dict(scale=sc, shift=case["beta"] - case["rm"] * sc)


def apply_f32(case, dtype, mode, relu, mutant=None):
    """bn_apply_kernel -> (out [rows, C] in dtype, mask bits [rows, C] bool)"""
    y, res = case["y"].float(), case["res"].float()
    rows, c = y.shape
    sc, sh = case["scale"].expand(rows, c), case["shift"]
    if mode == "res_bn" and mutant != "res_bn shift dropped":
        sh = sh + case["res_shift"]
    sh = sh.expand(rows, c)
    if mutant == "neighbouring chunk's coefficients in the last partial span":
        geo = C.stream_geometry(rows, c, dtype)
        ce = C.CE[dtype]
        first = (geo["n"] // geo["span"]) * geo["span"] * ce          # first element of the last, partial span
        if first < rows * c:
            roll = lambda t: torch.cat([t.reshape(-1)[:first], t.roll(-ce, 1).reshape(-1)[first:]]).view(rows, c)
            sc, sh = roll(sc), roll(sh)
    t = _fma(y, sc, sh)
    if mode == "res_bn":
        t = _fma(res, case["res_scale"].expand(rows, c), t)
    elif mode == "res":
        t = t + res
    v = t.clamp_min(0) if relu else t
    if mutant == "output rounded twice":
        out = v.to(torch.bfloat16).to(dtype)
    elif mutant == "output truncated":
        out = _rtz(v, dtype)
    else:
        out = v.to(dtype)
    bits = (out.float() > 0) if mutant == "mask from the rounded output" else (t > 0)
    return out, bits


def reduce_f32(case, dtype, use_a, mutant=None):
    """bn_bwd_reduce_kernel + reduce_finalize<BnBwdFin> -> dict(dbeta, dgamma, c1, c2 [C] fp32, dz)"""
    a_ok = (case["a_out"] >= 0) if mutant == "dz mask a_out >= 0" else (case["a_out"] > 0)
    dz = torch.where(a_ok, case["dA"], torch.zeros_like(case["dA"])) if use_a else case["dA"]
    m, c = dz.shape
    geo = C.bwd_geometry(m, c, dtype)
    rpi, nb, rpb = geo["rpi"], geo["nb"], geo["rpb"]
    d = dz.float()
    term = d * (case["y"].float() - case["mean"]) * case["invstd"]
    iters = -(-rpb // rpi)
    sums = []
    for v in (d, term):
        pad = torch.zeros(nb, iters * rpi, c)
        idx = torch.arange(m)
        pad[idx // rpb, idx % rpb] = v
        if mutant == "one row per block left out of pass 1":
            pad[:, min(rpb, m) - 1] = 0.0
        pad = pad.view(nb, iters, rpi, c)
        lane = torch.zeros(nb, rpi, c)
        for k in range(iters):                     # a thread's rows r0 + rr, r0 + rr + RPI, ...
            lane = lane + pad[:, k]
        blk = torch.zeros(nb, c)
        for k in range(rpi):                       # the RPI partials of a column, in order
            blk = blk + lane[:, k]
        s = slice_sums(blk, C.reduce_slices(nb, c))
        if mutant == "trailing slab dropped" and geo["slabs"] > 1:
            s[-geo["sw"]:] = float("nan")          # never reduced: the partial sums behind them are whatever the workspace held
        sums.append(s)
    n = float(m)
    return dict(dbeta=sums[0].float(), dgamma=sums[1].float(), c1=(sums[0] / n).float(), c2=(sums[1] / n).float(), dz=dz)


def dy_generic_f32(dz, case, c1, c2, dtype):
    """bn_bwd_apply_kernel"""
    xh = (case["y"].float() - case["mean"]) * case["invstd"]
    return (case["gamma"] * case["invstd"] * (dz.float() - c1 - xh * c2)).to(dtype)


def dy_stream_f32(dz, case, c1, c2, dtype, mutant=None):
    """bn_bwd_apply_dz_kernel: dy = fma(k0, dz, fma(k2, y, k1))"""
    gi = case["gamma"] * case["invstd"]
    k2 = -gi * c2 if mutant == "c2 scaled by invstd once too few" else -gi * case["invstd"] * c2
    k1 = -gi * c1 - k2 * case["mean"]
    e = lambda t: t.expand(dz.shape)
    return _fma(e(gi), dz.float(), _fma(e(k2), case["y"].float(), e(k1))).to(dtype)


def coeffs_f32(part, count):
    ns = C.reduce_slices(part.shape[0], part.shape[2])
    s, q = slice_sums(part[:, 0], ns), slice_sums(part[:, 1], ns)
    return dict(dbeta=s.float(), dgamma=q.float(), c1=(s / count).float(), c2=(q / count).float())


def coeffs_t_f32(case):
    part, ci = case["part"], case["t"].shape[1]
    s = slice_sums(part[:, 0], C.reduce_slices(part.shape[0], part.shape[2]))
    prod = case["t"].double() * case["w"].double()
    pad = torch.zeros(prod.shape[0], -(-ci // 128) * 128, dtype=torch.float64)
    pad[:, :ci] = prod
    pad = pad.view(prod.shape[0], -1, 16, 8)       # k = part + 8 (u + 16 j): lane `part` walks j then u
    lane = torch.zeros(prod.shape[0], 8, dtype=torch.float64)
    for j in range(pad.shape[1]):
        for u in range(16):
            lane = lane + pad[:, j, u]
    for sft in (1, 2, 4):
        lane = lane + lane[:, torch.arange(8) ^ sft]
    q = case["invstd"].double() * (lane[:, 0] - case["mean"].double() * s)
    n = float(case["rows"])
    return dict(dbeta=s.float(), dgamma=q.float(), c1=(s / n).float(), c2=(q / n).float())


# ------------------------------------------------------------------ judging a restatement
def fin_ratios(case, momentum, mutant=None):
    got = finalize_f32(case, momentum, True, mutant)
    ref = NB.finalize_ref(case["part"], case["count"], case["gamma"], case["beta"], case["rm"], case["rv"], momentum, C.EPS)
    ratios = {k: _ratio(got[k], *ref[k]) for k in got}
    old_ok = all(old_metric(got[k], ref[k][0]) < (OLD_STATS if k in ("rm", "rv") else 1e-5) for k in got)
    return ratios, old_ok


def apply_ratios(case, dtype, mode, relu, mutant=None):
    out, bits = apply_f32(case, dtype, mode, relu, mutant)
    r = NB.apply_ref(case["y"], case["scale"], case["shift"], case["res"] if mode != "none" else None,
                     case["res_scale"] if mode == "res_bn" else None, case["res_shift"] if mode == "res_bn" else None, relu, dtype)
    nm = _normal(r["ref"], dtype)
    ratios = {"out": _ratio(out, r["ref"], r["bnd"], nm), "out subnormal": _ratio(out, r["ref"], r["bnd"], ~nm)}
    bad = {}
    if dtype != F32:
        ratios["out once"] = float(B.rounding_excess(out, r["ref"], dtype, r["bnd"]).max())
        if relu:
            wrong, ghost, und = NB.mask_errors(bits, out, r, dtype, case["zeros"])
            bad = {"mask": wrong, "ghost bit": ghost, "undecided": int(und > 1e-3 * out.numel())}
            for (row, ch) in case["zeros"]:
                bad["zero"] = bad.get("zero", 0) + int(bool(bits[row, ch]) or int(out[row, ch].view(torch.int16)) != 0)
    return ratios, bad, old_metric(out, r["ref"]) < OLD_FWD[dtype]


def bwd_ratios(case, dtype, use_a, mutant=None):
    """the whole of rpe_bn_backward: pass 1 + 2, then pass 3 in both forms from the restatement's own coefficients"""
    m, c = case["y"].shape
    geo = C.bwd_geometry(m, c, dtype)
    got = reduce_f32(case, dtype, use_a, mutant)
    dz = C.dz_of(case, use_a)
    ref = NB.reduce_ref(dz, case["y"], case["mean"], case["invstd"], m, geo["rpb"])
    ratios = {k: _ratio(got[k], *ref[k].out()) for k in ("dbeta", "dgamma", "c1", "c2")}
    bad = {"dz bits": int((got["dz"].view(torch.int32 if dtype == F32 else torch.int16) != dz.view(torch.int32 if dtype == F32 else torch.int16)).sum())}
    dref, dbnd = NB.dy_ref(dz, case["y"], case["mean"], case["invstd"], case["gamma"], ref["c1"], ref["c2"], dtype)
    nm = _normal(dref, dtype)
    old_ok = all(old_metric(got[k], ref[k].v) < OLD_BWD[dtype] for k in ("dbeta", "dgamma")) and old_metric(got["dz"], dz) < OLD_BWD[dtype]
    for name, dy in (("dy generic", dy_generic_f32(got["dz"], case, got["c1"], got["c2"], dtype)),
                     ("dy stream", dy_stream_f32(got["dz"], case, got["c1"], got["c2"], dtype, mutant))):
        ratios[name] = _ratio(dy, dref, dbnd, nm)
        ratios[name + " subnormal"] = _ratio(dy, dref, dbnd, ~nm)
        if dtype != F32:
            ratios[name + " once"] = float(B.rounding_excess(dy, dref, dtype, dbnd).max())
        old_ok &= old_metric(dy, dref) < OLD_BWD[dtype]
    return ratios, bad, old_ok


def apply_dz_ratios(case, dtype, mutant=None):
    """rpe_bn_backward_apply_dz: coefficients passed in (exact)"""
    dz = C.dz_of(case, True)
    c1, c2 = case["c1c2"][0], case["c1c2"][1]
    dref, dbnd = NB.dy_ref(dz, case["y"], case["mean"], case["invstd"], case["gamma"], B.Fx(c1.double()), B.Fx(c2.double()), dtype)
    dy = dy_stream_f32(dz, case, c1, c2, dtype, mutant)
    nm = _normal(dref, dtype)
    ratios = {"dy passed": _ratio(dy, dref, dbnd, nm), "dy passed subnormal": _ratio(dy, dref, dbnd, ~nm)}
    if dtype != F32:
        ratios["dy passed once"] = float(B.rounding_excess(dy, dref, dtype, dbnd).max())
    return ratios, old_metric(dy, dref) < OLD_BWD[dtype]


HALF = 0.5


def _limit(k):
    return 1.0 if k.endswith("once") or k.endswith("subnormal") else HALF


def _rejected(ratios, bad=None):
    return any(not v <= 1.0 for v in ratios.values()) or any((bad or {}).values())


def _cases(name):
    """the cases a family is judged on, built once"""
    if name not in _MEMO:
        if name == "fin":
            _MEMO[name] = [("fin %s %s" % (sh, k), C.fin_case(sh[0], sh[1], k)) for sh in C.FIN_SHAPES for k in C.fin_kinds(sh[0])]
        elif name == "apply":
            _MEMO[name] = [("apply %s %s" % (str(t)[6:], sh), t, C.apply_case(t, *sh)) for t in C.DTYPES for sh in C.apply_shapes(t)]
        else:
            _MEMO[name] = [("bwd %s %s mean %g" % (str(t)[6:], sh, mk), t, C.bwd_case(t, sh[0], sh[1], mk))
                           for t in C.DTYPES for sh in C.BWD_SHAPES + C.BWD_DZ_EXTRA for mk in C.MEAN_KINDS]
    return _MEMO[name]


_MEMO = {}


# ------------------------------------------------------------------ soundness
def _assert_half(worst):
    for k, r in sorted(worst.items()):
        print("soundness %-28s worst err/bound %.3f" % (k, r))
    bad = {k: r for k, r in worst.items() if not r <= _limit(k)}
    assert not bad, bad


def _put(worst, prefix, ratios):
    for k, r in ratios.items():
        worst[prefix + k] = max(worst.get(prefix + k, 0.0), r)


def test_launcher_arithmetic_reaches_the_paths_named():
    """the shapes do what the tables say: slice counts, ragged unroll tails, partial spans, slabs, refusals"""
    assert [C.reduce_slices(*s) for s in C.FIN_SHAPES] == [1, 1, 2, 4, 64, 8, 1]
    t, ns = 2053, 64
    assert any(r + 3 * 8 * ns < t for r in range(8 * ns)) and (t % (4 * 8 * ns)) != 0          # unrolled loop and its tail
    for dtype in C.DTYPES:
        g = [C.stream_geometry(r, c, dtype) for (r, c) in C.apply_shapes(dtype)]
        assert g[1]["unr"] == 4 and g[1]["n"] % g[1]["span"] and g[1]["n"] > g[1]["span"]           # ends mid-unroll, > 1 block
        assert g[2]["unr"] == 1 and g[3]["unr"] == 1 and g[3]["cpr"] > 256
        assert g[4]["cpr"] == 512 and g[4]["sub"] == 2 and g[4]["n"] > g[4]["span"] and g[5]["cpr"] == 1
        geo = [C.bwd_geometry(m, c, dtype) for (m, c) in C.BWD_SHAPES]
        assert all(x is not None for x in geo)
        assert geo[0]["nb"] == 1 and geo[2]["nb"] > 1 and 601 % geo[2]["rpb"] and geo[5]["rpi"] == 1
        assert (geo[5]["slabs"], geo[6]["slabs"]) == ((2, 4) if dtype == F32 else (1, 2))
        assert C.bwd_geometry(5, 64, dtype)["rpi"] > 5
    assert all(C.bwd_geometry(C.BWD_ODD_M, c, t) is None for (t, c) in C.BWD_ODD_C)             # refused, all of them
    for sh in C.FIN_SHAPES:
        case = C.fin_case(sh[0], sh[1], "constant channels")
        p = case["part"].double()
        var = p[:, 1].sum(0) / case["count"] - (p[:, 0].sum(0) / case["count"]) ** 2
        if sh[0] > 1:
            assert float(var[:C.N_CONST].min()) < -C.EPS, "no constant channel of %s reaches the clamp" % (sh,)


def test_finalize_and_eval_affine_stay_within_half_the_bound():
    worst = {}
    for label, case in _cases("fin"):
        for m in C.MOMENTA:
            _put(worst, "fin ", fin_ratios(case, m)[0])
    for c in C.EVAL_C:
        case = C.eval_case(c)
        got, ref = eval_affine_f32(case), NB.eval_affine_ref(case["gamma"], case["beta"], case["rm"], case["rv"], C.EPS)
        _put(worst, "eval ", {k: _ratio(got[k], *ref[k]) for k in got})
    _assert_half(worst)


def test_apply_stays_within_half_the_bound():
    worst = {}
    for label, dtype, case in _cases("apply"):
        for mode in C.APPLY_MODES:
            for relu in (0, 1):
                ratios, bad, _ = apply_ratios(case, dtype, mode, relu)
                assert not any(bad.values()), (label, mode, relu, bad)
                _put(worst, "apply %s " % str(dtype)[6:], ratios)
    _assert_half(worst)


def test_backward_stays_within_half_the_bound():
    worst = {}
    for label, dtype, case in _cases("bwd"):
        name = str(dtype)[6:] + " "
        if C.bwd_geometry(*case["y"].shape, dtype) is not None:
            for use_a in (False, True):
                ratios, bad, _ = bwd_ratios(case, dtype, use_a)
                assert not any(bad.values()), (label, bad)
                _put(worst, "bwd " + name, ratios)
        _put(worst, "bwd " + name, apply_dz_ratios(case, dtype)[0])
        dz = C.dz_of(case, True)
        part = C.stats_part(dz, case)
        got, ref = coeffs_f32(part, dz.shape[0]), NB.coeffs_ref(part, dz.shape[0])
        _put(worst, "coeffs ", {k: _ratio(got[k], *ref[k].out()) for k in got})
        dref, dbnd = NB.dy_ref(dz, case["y"], case["mean"], case["invstd"], case["gamma"], ref["c1"], ref["c2"], dtype)
        dy = dy_stream_f32(dz, case, got["c1"], got["c2"], dtype)
        _put(worst, "from_dz " + name, {"dy": _ratio(dy, dref, dbnd, _normal(dref, dtype)), "dy subnormal": _ratio(dy, dref, dbnd, ~_normal(dref, dtype))})
    for dtype in C.DTYPES:
        for (tiles, c, ci) in C.COEFFS_T:
            for mk in C.MEAN_KINDS:
                case = C.coeffs_t_case(dtype, tiles, c, ci, mk)
                got = coeffs_t_f32(case)
                ref = NB.coeffs_t_ref(case["part"], case["t"], case["w"], case["mean"], case["invstd"], case["rows"])
                assert all(bool(torch.isfinite(v).all()) for v in got.values())
                _put(worst, "coeffs_t ", {k: _ratio(got[k], *ref[k].out()) for k in got})
    _assert_half(worst)


# ------------------------------------------------------------------ power
def _judge(mutant):
    """-> (cases rejecting, cases run, cases rejected here that the old metric at its bars passes)"""
    hits, n, old = 0, 0, 0
    if mutant in MUTANTS[2:7]:
        for label, case in _cases("fin"):
            for m in C.MOMENTA:
                ratios, ok = fin_ratios(case, m, mutant)
                hits, n, old = hits + _rejected(ratios), n + 1, old + (ok and _rejected(ratios))
    elif mutant in (MUTANTS[0], MUTANTS[7], MUTANTS[8], MUTANTS[9], MUTANTS[10]):
        for label, dtype, case in _cases("apply"):
            if dtype == F32 and mutant in (MUTANTS[7], MUTANTS[8], MUTANTS[9]):
                continue
            for mode in (("res_bn",) if mutant == MUTANTS[10] else C.APPLY_MODES):
                ratios, bad, ok = apply_ratios(case, dtype, mode, 1, mutant)
                hits, n, old = hits + _rejected(ratios, bad), n + 1, old + (ok and _rejected(ratios, bad))
    else:
        for label, dtype, case in _cases("bwd"):
            geo = C.bwd_geometry(*case["y"].shape, dtype)
            if geo is None or (mutant == MUTANTS[13] and geo["slabs"] == 1):
                continue
            ratios, bad, ok = bwd_ratios(case, dtype, True, mutant)
            hits, n, old = hits + _rejected(ratios, bad), n + 1, old + (ok and _rejected(ratios, bad))
    return hits, n, old


def test_mutants_are_rejected():
    missed, unseen = [], []
    for mutant in MUTANTS:
        hits, n, old = _judge(mutant)
        print("mutant %-60s rejected on %3d of %3d cases; the old rel_err bars pass %3d of those" % (mutant, hits, n, old))
        if not hits:
            missed.append(mutant)
        if old:
            unseen.append(mutant)
    print("faults that pass the old metric on a case where a bound rejects them: %d of %d: %s" % (len(unseen), len(MUTANTS), unseen))
    assert not missed, "mutants not rejected: %s" % missed
