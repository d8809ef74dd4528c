"""Self-tests of the pooling / stem-backward references and bounds (tests/_pool_bounds.py), on the CPU: no library, no GPU.

- the reference forward is torch's max_pool2d in value and index, on the random cases and on the constructed windows (ties, NaN, -inf);
- every case of tests/_pool_cases.py reaches the code path named beside it (the launchers' arithmetic restated there);
- soundness: torch-fp32 restatements of the kernels of csrc/norm.hip in the kernels' own association -- the backward's tap order behind
  the addend; the stem's per-lane sums over the passes of a pooled row and the rows of a block, the PPB-lane sum, the blocks in double,
  the k0 / k1 / k2 form of dy; the 8-lane butterfly of the few-image average pool -- stay at <= 0.5 of every bound on the very cases
  of the GPU test (judged on normal numbers: fp16 results under the smallest normal are reported, the floor IS their rounding);
- power: each fault of the *_MUTANTS lists, injected into a restatement, is rejected by a bound or an exact comparison on at least one
  case; printed beside it on how many of those cases the old metric max|err| / max|ref| at the old bars (test_maxpool_avgpool: equal
  values, tol(dtype) under the mask x > 0, 1e-5; test_stem_backward_fused: 2e-4 / 3e-2) passes it, i.e. would not have noticed."""
import pytest
import torch
import torch.nn.functional as F

import _bounds as B
import _pool_bounds as PB
import _pool_cases as C

F32 = torch.float32
OLD_TOL = {F32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}        # test_gpu_ops.tol
OLD_STEM = {F32: 2e-4, torch.bfloat16: 3e-2, torch.float16: 3e-2}
OLD_AVG = 1e-5

FWD_MUTANTS = ["padding counted as 0", "ties to the last tap", "NaN ignored", "an all -inf window names tap 0"]
BWD_MUTANTS = ["tap index transposed", "the window below dropped at odd rows", "addend added after rounding to T"]
STEM_MUTANTS = ["W01's tap 3 dropped", "W11's tap 0 dropped", "neighbour window not zeroed past the right edge", "aux winner transposed",
                "aux gradient without the depth feature", "mask from y > 0", "second ow pass skipped", "ragged last block left out",
                "count = B Ho Wo", "dy rounded twice"]
AVG_MUTANTS = ["pixels past 8 floor(HW / 8) dropped", "division by 8 ceil(HW / 8)", "sum taken in T"]


def old_metric(got, ref):
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    m = torch.isfinite(ref) & torch.isfinite(got)
    if not bool(m.any()):
        return 0.0
    return float((got[m] - ref[m]).abs().max() / ref[m].abs().max().clamp_min(1e-12))


def _name(dtype):
    return str(dtype)[6:]


def _fma(a, b, c):
    """fmaf through double: the product of two fp32 is exact in 53 bits"""
    return (a.double() * b.double() + c.double()).float()


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _ratio(got, ref, bnd, mask=None):
    if mask is not None:
        got, ref, bnd = got[mask], ref[mask], bnd[mask]
    return B.check(got, ref, bnd, "")[1] if ref.numel() else 0.0


def _normal(ref, dtype):
    return ref.abs() >= (2.0 ** -14 if dtype == torch.float16 else 2.0 ** -126)


def _once(got, ref, bnd, dtype, mask):
    """worst rounding excess (<= 1 for one rounding) over mask; 0 for fp32"""
    if dtype == F32 or not bool(mask.any()):
        return 0.0
    return float(B.rounding_excess(got, ref, dtype, bnd)[mask].max())


def _report(title, mutants, rejected, passed_old):
    for m in mutants:
        print("MUTANT %-16s %-50s rejected on %2d cases, the old metric passes it on %2d of them" % (title, m, rejected[m], passed_old[m]))
    missed = [m for m in mutants if rejected[m] == 0]
    assert not missed, "%s: no case rejects %s" % (title, missed)


# ------------------------------------------------------------------ max pool forward
def maxpool_fwd_k(x, mutant=None):
    """maxpool_fwd_kernel: best = -inf, the winner starts at the first in-image tap and is replaced on v > best || v != v"""
    b, h, w, c = x.shape
    ho, wo = C.pooled(h), C.pooled(w)
    v = PB._taps(x.float(), 0.0)
    inside = PB._taps(torch.ones(b, h, w, 1), 0.0) > 0
    if mutant == "padding counted as 0":
        inside = torch.ones_like(inside)
    first = (torch.arange(ho).view(ho, 1) == 0) * 3 + (torch.arange(wo).view(1, wo) == 0) * 1
    if mutant == "an all -inf window names tap 0":
        first = torch.zeros_like(first)
    best = torch.full((b, ho, wo, c), float("-inf"))
    bi = first.view(1, ho, wo, 1).expand(b, ho, wo, c).contiguous()
    for k in range(9):
        cond = (v[k] >= best) if mutant == "ties to the last tap" else (v[k] > best)
        if mutant != "NaN ignored":
            cond = cond | torch.isnan(v[k])
        cond = cond & inside[k]
        best, bi = torch.where(cond, v[k], best), torch.where(cond, torch.full_like(bi, k), bi)
    return best.to(x.dtype), bi.to(torch.uint8)


def _fwd_differs(got, ref):
    """value (bit for bit; a NaN for a NaN) or winner tap differs somewhere"""
    (go, gi), (ro, ri) = got, ref
    nan = torch.isnan(ro)
    return bool((torch.isnan(go) != nan).any()) or bool((_bits(go) != _bits(ro))[~nan].any()) or not torch.equal(gi, ri)


def _maxpool_cases():
    for dtype in C.DTYPES:
        for shape in C.maxpool_shapes(dtype):
            for kind in C.MAXPOOL_KINDS:
                yield dtype, shape, kind, C.maxpool_case(dtype, shape, kind)


def test_reference_forward_is_torch_max_pool2d():
    """value and index on every case, the constructed windows included; torch names the flat input pixel, the kernels the tap"""
    n_expect = 0
    for dtype, shape, kind, d in _maxpool_cases():
        b, h, w, c = shape
        x = d["x"]
        out, idx = PB.maxpool_ref(x)
        to, ti = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
        to, ti = to.permute(0, 2, 3, 1), ti.permute(0, 2, 3, 1)
        ho, wo = C.pooled(h), C.pooled(w)
        oh, ow = torch.arange(ho).view(1, ho, 1, 1), torch.arange(wo).view(1, 1, wo, 1)
        k = idx.long()
        flat = (2 * oh - 1 + k // 3) * w + (2 * ow - 1 + k % 3)
        label = "%s %s %s" % (_name(dtype), shape, kind)
        assert torch.equal(flat, ti), "%s: the reference's winner is not torch's in %d elements" % (label, int((flat != ti).sum()))
        nan = torch.isnan(to)
        assert torch.equal(torch.isnan(out), nan) and torch.equal(out.float()[~nan], to[~nan]), label + ": the reference's value is not torch's"
        for (bb, a, e, ch), tap in d["expect"].items():
            assert int(idx[bb, a, e, ch]) == tap, "%s: constructed window %s names tap %d, expected %d" % (label, (bb, a, e, ch), int(idx[bb, a, e, ch]), tap)
            n_expect += 1
        assert not _fwd_differs(maxpool_fwd_k(x), (out, idx)), label + ": the kernel's statement differs from the reference"
    assert n_expect > 0
    # the issue's example: a 4 x 4 map of nothing but -inf gives torch's indices 0, 1, 4, 5
    x = torch.full((1, 4, 4, 1), C.NINF)
    assert PB.maxpool_ref(x)[1].flatten().tolist() == [4, 3, 1, 0]
    assert F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)[1].flatten().tolist() == [0, 1, 4, 5]


def test_maxpool_forward_mutants_are_rejected():
    rejected, passed_old = {m: 0 for m in FWD_MUTANTS}, {m: 0 for m in FWD_MUTANTS}
    for dtype, shape, kind, d in _maxpool_cases():
        ref = PB.maxpool_ref(d["x"])
        for m in FWD_MUTANTS:
            got = maxpool_fwd_k(d["x"], m)
            if _fwd_differs(got, ref):
                rejected[m] += 1
                passed_old[m] += old_metric(got[0], ref[0]) == 0.0          # the old test never looked at the taps
    _report("pool forward", FWD_MUTANTS, rejected, passed_old)


# ------------------------------------------------------------------ max pool backward
def maxpool_bwd_k(dout, idx, addend, hw, dtype, mutant=None):
    """maxpool_bwd_kernel: acc = addend (or 0), then per pixel the windows in ascending (kh, kw) whose idx names that tap, in fp32;
    rounded once"""
    h, w = hw
    d, i = dout.float(), idx.long()
    b, _, _, c = d.shape
    late = mutant == "addend added after rounding to T" and addend is not None
    acc = addend.float().clone() if (addend is not None and not late) else torch.zeros(b, h, w, c)
    for k in range(9):
        if mutant == "the window below dropped at odd rows" and k // 3 == 0:      # (tap row 0 is the window below, and only odd rows have it)
            continue
        named = (k % 3) * 3 + k // 3 if mutant == "tap index transposed" else k
        acc = acc + PB._untap(torch.where(i == named, d, torch.zeros_like(d)), k, h, w)
    if late:
        return (acc.to(dtype).float() + addend.float()).to(dtype)
    return acc.to(dtype)


def _bwd_ratios(got, ref, bnd, named, addend, dtype):
    r = dict(dx=_ratio(got, ref, bnd, _normal(ref, dtype)), once=_once(got, ref, bnd, dtype, _normal(ref, dtype)))
    base = torch.zeros_like(got) if addend is None else addend
    r["unnamed not exact"] = float((_bits(got) != _bits(base))[~named].sum())
    r["dx subnormal"] = _ratio(got, ref, bnd, ~_normal(ref, dtype))
    return r


def _bad(r):
    """the checks of a ratio dict that fail: a bound or the one-rounding rule exceeded, an exact comparison broken"""
    return {k: v for k, v in r.items() if not k.endswith("subnormal") and (v > 1.0 or (k.endswith("exact") and v > 0))}


def test_maxpool_backward_stays_within_half_the_bound_and_rejects_its_mutants():
    worst = {}
    rejected, passed_old = {m: 0 for m in BWD_MUTANTS}, {m: 0 for m in BWD_MUTANTS}
    for dtype, shape, kind, d in _maxpool_cases():
        hw = shape[1:3]
        idx = PB.maxpool_ref(d["x"])[1]
        for addend in (None, d["addend"]):
            ref, bnd, named = PB.maxpool_bwd_ref(d["dout"], idx, addend, hw, dtype)
            r = _bwd_ratios(maxpool_bwd_k(d["dout"], idx, addend, hw, dtype), ref, bnd, named, addend, dtype)
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
            mask = (d["x"] > 0).double()                                    # the old test's mask
            for m in BWD_MUTANTS:
                got = maxpool_bwd_k(d["dout"], idx, addend, hw, dtype, m)
                if _bad(_bwd_ratios(got, ref, bnd, named, addend, dtype)):
                    rejected[m] += 1
                    passed_old[m] += old_metric(got.double() * mask, ref * mask) < OLD_TOL[dtype]
    print("RATIOS pool backward: %s" % {k: round(v, 3) for k, v in worst.items()})
    assert worst["dx"] <= 0.5 and worst["once"] <= 1.0 and worst["unnamed not exact"] == 0, worst
    _report("pool backward", BWD_MUTANTS, rejected, passed_old)


# ------------------------------------------------------------------ stem backward
def stem_k(d, geo, dtype, mutant=None):
    """stem_bwd_reduce_kernel + reduce_finalize (BnBwdFin) + stem_bwd_apply_kernel -> dict(dbeta, dgamma, c1, c2 [64] fp32, dy in dtype,
    dz fp32 [B, H, W, 64])"""
    y = d["y"]
    b, h, w, _ = y.shape
    ho, wo = h // 2, w // 2
    dp, pi = d["dpool"].float(), d["pool_idx"].long()
    zero = torch.zeros_like(dp)

    def win(dh, dw):            # the window (oh + dh, ow + dw): zero gradient and no tap past the edge
        z, t = torch.zeros_like(dp), torch.full_like(pi, 255)
        z[:, :ho - dh, :wo - dw], t[:, :ho - dh, :wo - dw] = dp[:, dh:, dw:], pi[:, dh:, dw:]
        return z, t
    (d0, t0), (d1, t1), (d2, t2), (d3, t3) = (dp, pi), win(0, 1), win(1, 0), win(1, 1)
    if mutant == "neighbour window not zeroed past the right edge":      # (the kernel reads the own window in its place)
        d1, t1 = d1.clone(), t1.clone()
        d1[:, :, wo - 1], t1[:, :, wo - 1] = dp[:, :, wo - 1], pi[:, :, wo - 1]
    pick = lambda t, k, dd: torch.where(t == k, dd, zero)
    dz = [pick(t0, 4, d0),
          pick(t0, 5, d0) + (zero if mutant == "W01's tap 3 dropped" else pick(t1, 3, d1)),
          pick(t0, 7, d0) + pick(t2, 1, d2),
          ((pick(t0, 8, d0) + pick(t1, 6, d1)) + pick(t2, 2, d2)) + (zero if mutant == "W11's tap 0 dropped" else pick(t3, 0, d3))]
    if d["aux_dout"] is not None:
        g = d["aux_dout"][:, :ho * wo].reshape(b, ho, wo, 1)
        if d["depth_feat"] is not None and mutant != "aux gradient without the depth feature":
            g = g * d["depth_feat"].reshape(b, ho, wo, 1)
        gw = g * d["aux_w"]
        win_ = d["aux_idx"].long().reshape(b, ho, wo, 1)
        if mutant == "aux winner transposed":
            win_ = (win_ % 2) * 2 + win_ // 2
        dz = [dz[k] + torch.where(win_ == k, gw, zero) for k in range(4)]
    yf = y.float()
    yy = [yf[:, 0::2, 0::2], yf[:, 0::2, 1::2], yf[:, 1::2, 0::2], yf[:, 1::2, 1::2]]
    sc, sh, mu, iv = d["scale"], d["shift"], d["mean"], d["invstd"]
    for k in range(4):
        on = (yy[k] > 0) if mutant == "mask from y > 0" else (_fma(yy[k], sc, sh) > 0)
        dz[k] = torch.where(on, dz[k], zero)
    # pass 1: a thread's sums over the passes of a pooled row and the rows of its block, the PPB lanes in order, the blocks in double
    rows, rpb, nb, ppb = geo["rows"], geo["rpb"], geo["nb"], geo["ppb"]
    dzr = [t.reshape(rows, wo, 64) for t in dz]
    tr = [(dzr[k] * (yy[k].reshape(rows, wo, 64) - mu)) * iv for k in range(4)]
    lane1, lane2 = torch.zeros(nb, ppb, 64), torch.zeros(nb, ppb, 64)
    for r in range(rpb):
        row = torch.arange(nb) * rpb + r
        vb = torch.nonzero(row < rows).flatten()
        for ow0 in range(0, wo, ppb):
            if ow0 and mutant == "second ow pass skipped":
                break
            n = min(ppb, wo - ow0)
            for k in range(4):
                lane1[vb, :n] += dzr[k][row[vb], ow0:ow0 + n]
                lane2[vb, :n] += tr[k][row[vb], ow0:ow0 + n]
    t1, t2 = torch.zeros(nb, 64), torch.zeros(nb, 64)
    for k in range(ppb):
        t1, t2 = t1 + lane1[:, k], t2 + lane2[:, k]
    if mutant == "ragged last block left out" and rows % rpb:
        t1, t2 = t1[:-1], t2[:-1]
    s1, s2 = t1.double().sum(0), t2.double().sum(0)
    cnt = float(b * ho * wo if mutant == "count = B Ho Wo" else b * h * w)
    o = dict(dbeta=s1.float(), dgamma=s2.float(), c1=(s1 / cnt).float(), c2=(s2 / cnt).float())
    # pass 2
    gi = d["gamma"] * iv
    k2 = -gi * iv * o["c2"]
    k1 = -gi * o["c1"] - k2 * mu
    dy, dzf = torch.zeros(b, h, w, 64), torch.zeros(b, h, w, 64)
    for k in range(4):
        rest = _fma(k2, yy[k], k1)
        if mutant == "dy rounded twice":
            rest = rest.to(dtype).float()
        dy[:, k // 2::2, k % 2::2] = _fma(gi, dz[k], rest)
        dzf[:, k // 2::2, k % 2::2] = dz[k]
    o.update(dy=dy.to(dtype), dz=dzf)
    return o


def stem_ratios(o, r, dtype):
    """got (stem_k's or the library's outputs; dz only from the restatement) against stem_ref"""
    dec = ~r["undecided"]
    ref, bnd = r["dy"]
    nrm = _normal(ref, dtype) & dec
    out = {k: _ratio(o[k], *r[k].out()) for k in ("dbeta", "dgamma", "c1", "c2")}
    out.update(dy=_ratio(o["dy"], ref, bnd, nrm), once=_once(o["dy"], ref, bnd, dtype, nrm))
    out["dy subnormal"] = _ratio(o["dy"], ref, bnd, dec & ~_normal(ref, dtype))
    out["dy off"] = _ratio(o["dy"], *r["plain"], r["off"] & _normal(r["plain"][0], dtype))
    if "dz" in o:
        out["dz"] = _ratio(o["dz"], *r["dz"].out(), dec)
        out["dz off not exact"] = float((_bits(o["dz"]) != 0)[r["off"]].sum())
    return out


_STEM = {}


def _stem(dtype, shape, aux):
    """case, geometry and reference, computed once"""
    key = (dtype, shape, aux)
    if key not in _STEM:
        d = C.stem_case(dtype, shape, aux)
        geo = C.stem_geometry(*shape, dtype)
        _STEM[key] = (d, geo, PB.stem_ref(d, geo["rpb"], dtype))
    return _STEM[key]


def test_stem_backward_stays_within_half_the_bound():
    worst, und_total = {}, 0
    for dtype in C.DTYPES:
        for shape in C.STEM_SHAPES:
            for aux in C.STEM_AUX:
                d, geo, r = _stem(dtype, shape, aux)
                und = int(r["undecided"].sum())
                und_total += und
                assert und <= 1e-3 * r["undecided"].numel(), "%s %s %s: %d undecided elements" % (_name(dtype), shape, aux, und)
                zb, zh, zw, zc = d["zero"]
                assert bool(r["off"][zb, zh, zw, zc]), "the constructed +0 is not off"
                for k, v in stem_ratios(stem_k(d, geo, dtype), r, dtype).items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print("RATIOS stem backward: %s; undecided elements in all cases: %d" % ({k: round(v, 3) for k, v in worst.items()}, und_total))
    bad = {k: v for k, v in worst.items() if not v <= (1.0 if k in ("once", "dy subnormal") else 0.0 if k.endswith("exact") else 0.5)}
    assert not bad, "restatement beyond half a bound: %s" % bad
    assert und_total == 0


def test_stem_backward_mutants_are_rejected():
    """on the cases with the aux head and the depth feature (every mutant has something to break there), without the 2050-row one"""
    rejected, passed_old = {m: 0 for m in STEM_MUTANTS}, {m: 0 for m in STEM_MUTANTS}
    for dtype in C.DTYPES:
        for shape in C.STEM_SHAPES:
            if shape[1] > 100:
                continue
            d, geo, r = _stem(dtype, shape, "aux x depth")
            for m in STEM_MUTANTS:
                o = stem_k(d, geo, dtype, m)
                if _bad(stem_ratios(o, r, dtype)):
                    rejected[m] += 1
                    passed_old[m] += all(old_metric(o[k], ref) < OLD_STEM[dtype] for k, ref in
                                         (("dy", r["dy"][0]), ("dgamma", r["dgamma"].v), ("dbeta", r["dbeta"].v)))
    _report("stem backward", STEM_MUTANTS, rejected, passed_old)


# ------------------------------------------------------------------ average pool
def avgpool_fwd_k(x, mutant=None):
    """avgpool_fwd_kernel (pixels in order) or, where the launcher switches, avgpool_fwd_few_kernel: 8 lanes walk the pixels 8 apart,
    their sums meet in the butterfly xor 1, 2, 4; times 1.f / HW"""
    b, hw, c = x.shape
    acc_t = x.dtype if mutant == "sum taken in T" else F32
    xf = x.to(acc_t)
    if C.avgpool_few(b, hw, c):
        end = hw // 8 * 8 if mutant == "pixels past 8 floor(HW / 8) dropped" else hw
        lanes = []
        for s in range(8):
            acc = torch.zeros(b, c, dtype=acc_t)
            for p in range(s, end, 8):
                acc = acc + xf[:, p]
            lanes.append(acc)
        for o in (1, 2, 4):
            lanes = [lanes[k] + lanes[k ^ o] for k in range(8)]
        acc = lanes[0]
    else:
        acc = torch.zeros(b, c, dtype=acc_t)
        for p in range(hw):
            acc = acc + xf[:, p]
    n = (hw + 7) // 8 * 8 if mutant == "division by 8 ceil(HW / 8)" else hw
    return acc.float() * (torch.tensor(1.0) / torch.tensor(float(n)))


def avgpool_bwd_k(dout, hw, dtype):
    b, c = dout.shape
    return (dout * (torch.tensor(1.0) / torch.tensor(float(hw)))).view(b, 1, c).expand(b, hw, c).to(dtype)


def test_average_pool_stays_within_half_the_bound_and_rejects_its_mutants():
    worst = {}
    rejected, passed_old = {m: 0 for m in AVG_MUTANTS}, {m: 0 for m in AVG_MUTANTS}
    for dtype in C.DTYPES:
        for shape in C.avgpool_bwd_shapes(dtype):
            d = C.avgpool_case(dtype, shape)
            ref, bnd = PB.avgpool_bwd_ref(d["dout"], shape[1], dtype)
            got = avgpool_bwd_k(d["dout"], shape[1], dtype)
            nrm = _normal(ref, dtype)
            for k, v in (("backward", _ratio(got, ref, bnd, nrm)), ("backward once", _once(got, ref, bnd, dtype, nrm)),
                         ("backward subnormal", _ratio(got, ref, bnd, ~nrm))):
                worst[k] = max(worst.get(k, 0.0), v)
            if shape not in C.avgpool_shapes(dtype):
                continue
            ref, bnd = PB.avgpool_ref(d["x"])
            worst["forward"] = max(worst.get("forward", 0.0), _ratio(avgpool_fwd_k(d["x"]), ref, bnd))
            for m in AVG_MUTANTS:
                got = avgpool_fwd_k(d["x"], m)
                if _ratio(got, ref, bnd) > 1.0:
                    rejected[m] += 1
                    passed_old[m] += old_metric(got, ref) < OLD_AVG
    print("RATIOS average pool: %s" % {k: round(v, 3) for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v <= (1.0 if k in ("backward once", "backward subnormal") else 0.5)}
    assert not bad, "restatement beyond half a bound: %s" % bad
    _report("average pool", AVG_MUTANTS, rejected, passed_old)


# ------------------------------------------------------------------ the cases reach their paths
@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
def test_cases_reach_their_paths(dtype):
    ce = C.CE[dtype]
    one_tap, one_window, odd, general, odd_cpr, blocks = C.maxpool_shapes(dtype)
    assert one_tap[1:3] == (1, 1) and one_window[1:3] == (2, 2) and C.pooled(2) == 1
    assert odd[1] % 2 == 1 and odd[2] % 2 == 1 and odd[3] // ce > 1                  # window (Ho - 1, Wo - 1) reaches row H and column W
    assert general == C.CONSTRUCTED and general[0] > 1
    cpr = odd_cpr[3] // ce
    assert cpr & (cpr - 1)
    b, h, w, c = blocks
    assert b * C.pooled(h) * C.pooled(w) * (c // ce) > 256 and b * h * w * (c // ce) > 256      # forward and backward: more than one block
    assert all(s[3] % ce == 0 for s in C.maxpool_shapes(dtype))
    assert len(C.fused_shapes(dtype)) == (2 if dtype == F32 else 4)       # (fp32: the general case and the one with several blocks)

    geo = [C.stem_geometry(*s, dtype) for s in C.STEM_SHAPES]
    ppb = 16 if dtype == F32 else 32
    assert all(g["ppb"] == ppb for g in geo)
    g = geo[0]                                                                       # one window
    assert (g["rows"], g["wo"], g["nbl"], g["rpb"], g["nb"], g["apply_blocks"]) == (1, 1, 1, 1, 1, 1)
    g = geo[1]                                                                       # Wo = 34: 16 + 16 + 2 / 32 + 2, one pooled row per block
    assert g["wo"] == 34 and -(-g["wo"] // ppb) == (3 if dtype == F32 else 2) and g["wo"] % ppb == 2 and g["rpb"] == 1 and g["nb"] == 6
    g = geo[2]                                                                       # two blocks of 5 and 4 of the nine pooled rows; Ho = 3
    assert (g["nbl"], g["rpb"], g["nb"], g["rows"]) == (2, 5, 2, 9) and g["rows"] % g["rpb"] == 4
    assert C.STEM_SHAPES[2][1] // 2 == 3 and g["rpb"] > 3                            # block 0 crosses from image 0 into image 1
    assert g["apply_blocks"] == 5 and g["rows"] % 2 == 1                             # a one-row last block; block 1 = pooled rows 2, 3: images 0, 1
    g = geo[3]                                                                       # the cap of 1024 blocks
    assert g["rows"] == 1025 and (g["nbl"], g["rpb"], g["nb"]) == (1024, 2, 513) and g["rows"] % g["rpb"] == 1
    from _norm_cases import reduce_slices
    assert reduce_slices(g["nb"], 64) == 64 and all(reduce_slices(q["nb"], 64) == 1 for q in geo[:3] + geo[4:])
    g = geo[4]
    assert (g["nbl"], g["rpb"], g["nb"], g["rows"]) == (3, 5, 3, 14)
    assert C.stem_geometry(1, 2, 2, 127, dtype) is None                              # refused: RPE_ERR_WORKSPACE

    plain = [(2, 1, 2 * ce), (2, 9, ce), (2, 15, 64), (33, 16, 2048)]
    few = [(1, 16, ce), (2, 17, 64), (3, 49, 2048), (32, 16, 2048)]
    assert C.avgpool_shapes(dtype) == plain + few
    assert not any(C.avgpool_few(*s) for s in plain) and all(C.avgpool_few(*s) for s in few)
    assert all(s[1] < 16 for s in plain[:3]) and all(s[0] * s[2] // ce < 256 for s in plain[:3])       # idle threads in the one block
    assert 33 * 2048 > 65536 and 32 * 2048 == 65536
    assert 1 * ce // ce * 8 == 8 and 17 % 8 and 49 % 8
    extra = [s for s in C.avgpool_bwd_shapes(dtype) if s not in C.avgpool_shapes(dtype)]
    assert len(extra) == 1 and (extra[0][2] // ce) & (extra[0][2] // ce - 1)
    assert C.refused_channels(dtype) % ce and C.refused_channels(dtype) > ce
