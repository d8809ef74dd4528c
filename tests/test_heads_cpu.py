"""Self-tests of the head-kernel references and bounds (tests/_head_bounds.py), on the CPU.

- reference: the fp64 references equal oracle.pose_oracle.aux_head / depth_head (any `pools`, odd sizes) and torch autograd;
- soundness: plain torch-fp32 statements of the kernels of csrc/heads.hip, in the kernels' own association (per-lane partial dot
  products then the xor tree, per-thread partial sums then waves then blocks, window sums then * 1 / win^2, statistics in double),
  stay at <= 0.5 of every bound on every case of tests/_head_cases.py that is small enough for the CPU;
- decided windows: at most 0.1 % of the random windows of any case are too close to call;
- power: the faults listed in AUX_MUTANTS / DEPTH_MUTANTS and a det_y that skips its rounding are each rejected on at least one
  case, several of them where the one-number metric max|got - ref| / max|ref| of test_aux_and_depth_heads passes them."""
import pytest
import torch

import _bounds as B
import _head_bounds as HB
import _head_cases as C
from oracle import pose_oracle as po

F32 = torch.float32
OLD_BAR = {F32: 1e-5, torch.bfloat16: 1e-2, torch.float16: 1e-2}      # test_aux_and_depth_heads: its forward bars
OLD_BAR_BWD = {F32: 1e-4, torch.bfloat16: 2e-2, torch.float16: 2e-2}  # and its backward bars


def old_metric(got, ref):
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    m = torch.isfinite(ref)
    if not bool(m.any()):
        return 0.0
    return float((got[m] - ref[m]).abs().max() / ref[m].abs().max().clamp_min(1e-12))


# ------------------------------------------------------------------ fp32 statements of the kernels
def _xor_tree(v, n):
    """v [..., n]: the butterfly `v += shfl_xor(v, s)` for s = 1, 2, .. < n; every lane ends with the same sum"""
    lanes, s = torch.arange(n), 1
    while s < n:
        v = v + v[..., lanes ^ s]
        s <<= 1
    return v[..., 0]


def _rtz(t, dtype):
    """fp32 -> dtype rounded toward zero (the faulty conversion)"""
    if dtype == F32:
        return t
    r = t.to(dtype)
    away = r.float().abs() > t.abs()
    bits = r.view(torch.int16)
    return torch.where(away, bits - 1, bits).view(dtype)        # one step toward zero (sign-magnitude: the magnitude's bits shrink)


def aux_fwd_f32(case, dtype, mutant=None):
    """auxc_fwd_kernel (and aux_fwd_kernel, which is its C = 64 case: LPP = 64 / CE lanes per pixel) -> out, raw, idx [B, Ho Wo]"""
    x, w = case["x"], case["w"]
    b, h, wd, c = x.shape
    ce = C.CE[dtype]
    cpp = c // ce
    lpp = min(cpp, 64)
    walk = cpp // lpp
    xf, wf = x.float().reshape(-1, walk, lpp, ce), w.reshape(walk, lpp, ce)
    d = torch.zeros(xf.shape[0], lpp)
    for j in range(walk - 1 if mutant == "last chunk dropped" and walk > 1 else walk):
        for e in range(ce):
            d = d + xf[:, j, :, e] * wf[j, :, e]
    d = _xor_tree(d, lpp) + case["bias"]
    ho, wo = h // 2, wd // 2
    raw, idx = HB.scan_winner(HB.taps(d.reshape(b, h, wd), ho, wo).reshape(b, ho * wo, 4), ge=(mutant == ">= winner"))
    out = raw if case["depth_feat"] is None else raw * case["depth_feat"]
    return out, (out if mutant == "raw after depth product" else raw), idx


def _block_sums(p, grid, groups, gpw, det, start):
    """p [windows, cols]: the per-window terms of aux_bwd_kernel's dw / dbias sums, in its association: a lane group takes the windows
    blockIdx groups + its number, striding by grid x groups, and adds them in turn; the gpw groups of a wave fold by shuffles, the four
    waves add in order; then the blocks: one atomic add each onto `start` (block order here), or (det) aux_bwd_reduce_kernel: 256
    lanes take strided shares of the block column, folded by a tree in shared memory -- overwriting."""
    total, cols = p.shape
    per_trip = grid * groups
    trips = (total + per_trip - 1) // per_trip
    pad = torch.zeros(trips * per_trip, cols)
    pad[:total] = p
    pad = pad.reshape(trips, grid, groups // gpw, gpw, cols)
    acc = torch.zeros_like(pad[0])
    for t in range(trips):
        acc = acc + pad[t]
    acc = _xor_tree(acc.permute(0, 1, 3, 2), gpw)                         # [grid, waves, cols]
    blk = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]               # [grid, cols]
    if det:
        lanes = torch.zeros(256, cols)
        for r0 in range(0, grid, 256):
            part = blk[r0:r0 + 256]
            lanes[:part.shape[0]] = lanes[:part.shape[0]] + part
        o = 128
        while o:
            lanes = lanes[:o] + lanes[o:2 * o]
            o >>= 1
        return lanes[0]
    s = start.clone()
    for g in range(grid):
        s = s + blk[g]
    return s


def aux_bwd_f32(case, dtype, raw, idx, out=None, form="atomic", start=(0.0, 0.0), mutant=None, act=None):
    """aux_bwd_kernel (form atomic / det) and auxc_bwd_kernel (form c) -> d_depth_feat [B, n], d_x [B, H, W, C] in dtype, dw [C], db [1].
    act: the activated tensor the dw sum reads instead of case["x"] (the det_y form recomputes it at the winner pixel)."""
    x, w, df, dout = case["x"] if act is None else act, case["w"], case["depth_feat"], case["dout"]
    b, h, wd, c = x.shape
    d = dout if df is None else dout * df
    ddf = dout * (out if mutant == "d_depth_feat from out" else raw)
    img, ih, iw = HB.winner_pixels(idx, b, h, wd)
    g = d[..., None] * w
    g = _rtz(g, dtype) if mutant == "gradient truncated" else g.to(dtype)
    dx = torch.zeros(b, h, wd, c, dtype=dtype)
    if mutant == "gradient to tap 0":
        dx[img, ih - (idx.long() >> 1), iw - (idx.long() & 1)] = g
    else:
        dx[img, ih, iw] = g
    terms = torch.cat([d.reshape(-1, 1) * x[img, ih, iw].float().reshape(-1, c), d.reshape(-1, 1)], 1)      # the last column: dbias
    total = terms.shape[0]
    ce = C.CE[dtype]
    lpp = min(c // ce, 64)
    st = torch.cat([torch.full((c,), float(start[0])), torch.tensor([float(start[1])])])
    if form == "c":        # shared-memory atomics in window order within a block of 256 / LPP groups, then one global atomic per block
        groups, grid = 256 // lpp, C.ew_grid(total, 32)
        per_trip = grid * groups
        trips = (total + per_trip - 1) // per_trip
        pad = torch.zeros(trips * per_trip, c + 1)
        pad[:total] = terms
        pad = pad.reshape(trips, grid, groups, c + 1)
        blk = torch.zeros(grid, c + 1)
        for t in range(trips):
            for q in range(groups):
                blk = blk + pad[t, :, q]
        s = st.clone()
        for k in range(grid):
            s = s + blk[k]
    else:
        grid = C.ew_grid(total, (16 if dtype == F32 else 32) * 4)
        s = _block_sums(terms, grid, 256 // lpp, 64 // lpp, form == "det", st)
    return ddf, dx, s[:c], s[c:]


def bn_act_f32(y, scale, shift, dtype, rounded=True):
    """a1 = round_T(relu(fma(y, scale, shift))): bn_apply_kernel's expression (the fma through double: 53 >= 2 x 24 + 2 bits, so the
    second rounding is innocuous); rounded=False: the faulty det_y that skips the rounding to T"""
    a = (y.double() * scale.double() + shift.double()).float().clamp_min(0)
    return a.to(dtype) if rounded else a


def depth_fwd_f32(case, pools, form, mutant=None):
    """depth_fwd_kernel (form quad: four 2 x 2 averages averaged) / depth_pools_fwd_kernel (form wave: 64 lanes stride over the window,
    xor tree, * 1 / win^2) -> xhat, feat [B, Ho Wo]"""
    depth, w, bias = case["depth"], case["w"], case["b"]
    b, h, wd = depth.shape
    win = 1 << pools
    anchor = (lambda o, size, osize: (o * size) // osize) if mutant == "windows at oh H / Ho" else None
    wnd = HB.depth_windows(depth, pools, anchor)
    n = wnd.shape[1] * wnd.shape[2]
    if form == "quad":
        v = wnd.reshape(b, n, 2, 2, 2, 2)                                  # [.., a, row, c, column] of the 4 x 4 window
        acc = torch.zeros(b, n)
        for a in range(2):
            for c in range(2):
                acc = acc + (v[:, :, a, 0, c, 0] + v[:, :, a, 0, c, 1] + v[:, :, a, 1, c, 0] + v[:, :, a, 1, c, 1]) * 0.25
        pooled = acc * 0.25
    else:
        k = win * win
        t = (k + 63) // 64
        pad = torch.zeros(b, n, t * 64)
        pad[..., :k] = wnd.reshape(b, n, k)
        pad = pad.reshape(b, n, t, 64)
        acc = torch.zeros(b, n, 64)
        for i in range(t):
            acc = acc + pad[:, :, i]
        pooled = _xor_tree(acc, 64) * (1.0 / k)
    pd = pooled.double()
    mean = pd.mean(1, keepdim=True)
    var = ((pd * pd).mean(1, keepdim=True) - mean * mean).clamp_min(0.0)
    if mutant == "unbiased variance":
        var = var * n / max(n - 1, 1)
    invstd = (1.0 / (var.sqrt() + 1e-5) if mutant == "eps outside the root" else 1.0 / (var + 1e-5).sqrt()).float()
    xhat = (pooled - mean.float()) * invstd
    return xhat, xhat * w + bias


def depth_bwd_f32(case, start):
    """depth_bwd_kernel: thread-strided partial sums, wave tree, four waves in order, one atomic add per block"""
    n = case["d_feat"].numel()
    grid = C.depth_bwd_blocks(n)
    terms = torch.stack([case["d_feat"] * case["xhat"], case["d_feat"]], 1)
    span = grid * 256
    trips = (n + span - 1) // span
    pad = torch.zeros(trips * span, 2)
    pad[:n] = terms
    pad = pad.reshape(trips, grid, 4, 64, 2)
    acc = torch.zeros_like(pad[0])
    for t in range(trips):
        acc = acc + pad[t]
    acc = _xor_tree(acc.permute(0, 1, 3, 2), 64)                          # [grid, 4, 2]
    blk = acc[:, 0] + acc[:, 1] + acc[:, 2] + acc[:, 3]
    s = torch.tensor([float(start[0]), float(start[1])])
    for g in range(grid):
        s = s + blk[g]
    return s[:1], s[1:]


# ------------------------------------------------------------------ the cases small enough for the CPU
def aux_cases(dtype):
    """(label, case, form): every C = 64 shape and every any-C shape of _head_cases.py but the forward-only grid-stride ones; built once,
    each case keeps its references (computed on first use, never changed)"""
    if dtype not in _AUX_CASES:
        _AUX_CASES[dtype] = list(_aux_cases(dtype))
    return _AUX_CASES[dtype]


_AUX_CASES = {}


def _cached(case, key, make):
    memo = case.setdefault("_memo", {})
    if key not in memo:
        memo[key] = make()
    return memo[key]


def _aux_cases(dtype):
    for (b, h, w) in C.AUX_SHAPES:
        for kind in C.KINDS:
            for use_depth in (False, True):
                for con in C.CONSTRUCTS:
                    yield "aux64 %s %s depth=%d %s" % ((b, h, w), kind, use_depth, con), C.aux_case(dtype, b, h, w, 64, kind, use_depth, con), "64"
    for c in C.AUXC_C[dtype]:
        for (h, w) in C.AUXC_HW:
            for b in C.AUXC_B:
                for k, con in enumerate(C.CONSTRUCTS):
                    kind, use_depth = C.KINDS[(k + b) % 2], bool((k + h) % 2)
                    yield "auxc C=%d %s %s depth=%d %s" % (c, (b, h, w), kind, use_depth, con), C.aux_case(dtype, b, h, w, c, kind, use_depth, con), "c"


def _slot_mask(case, b, n, wo):
    m = torch.zeros(b, n, dtype=torch.bool)
    for (i, oh, ow) in case["slots"]:
        m[i, oh * wo + ow] = True
    return m


def _ratio(got, ref, bnd, mask=None):
    if mask is not None:
        got, ref, bnd = got[mask], ref[mask], bnd[mask]
    return B.check(got, ref, bnd, "")[1] if ref.numel() else 0.0


def aux_ratios(dtype, case, form, mutant=None):
    """-> ({output: worst err/bound}, {check: mismatches}, [old metric forward, backward]) of the fp32 statement (with `mutant`) against
    the references; the backward runs from the CORRECT forward's raw / idx (a case with a NaN window has no backward)"""
    x = case["x"]
    b, h, wd, c = x.shape
    n, wo = C.windows(h, wd), wd // 2
    ref = _cached(case, "fwd ref", lambda: HB.aux_fwd_ref(x, case["w"], case["bias"], case["depth_feat"]))
    out, raw, idx = aux_fwd_f32(case, dtype, mutant)
    fin = ref["finite"]
    ratios = dict(raw=_ratio(raw, ref["raw"], ref["braw"], fin), out=_ratio(out, ref["out"], ref["bout"], fin))
    slots = _slot_mask(case, b, n, wo)
    strict = int((idx[slots] != ref["idx"][slots]).sum())                 # constructed windows: the scan-order rule, exactly
    nanbad = int((~(raw[~fin].isnan() & out[~fin].isnan()) | (idx[~fin] != 2)).sum())
    bad = dict(idx=HB.idx_errors(idx, ref), strict=strict, nan=nanbad)
    old = [old_metric(out, ref["out"]), 0.0]                              # forward, backward
    if bool(fin.all()):
        out0, raw0, idx0 = _cached(case, "fwd", lambda: aux_fwd_f32(case, dtype))
        start = (0.5, -0.25) if form != "det" else (0.0, 0.0)
        bform = {"64": "atomic", "c": "c", "det": "det"}[form]
        total = b * n
        steps = 0 if form == "det" else (C.ew_grid(total, 32) if form == "c" else C.ew_grid(total, (16 if dtype == F32 else 32) * 4))
        ddf, dx, dw, db = aux_bwd_f32(case, dtype, raw0, idx0, out0, bform, start, mutant)
        rb = _cached(case, "bwd ref " + form, lambda: HB.aux_bwd_ref(case["dout"], x, case["w"], case["depth_feat"], raw0, idx0, dtype, start, steps))
        img, ih, iw = rb["winner"]
        gw = dx[img, ih, iw]
        # below T's smallest normal the rounding step is the subnormal spacing, whose half IS the bound's floor: a correct kernel reaches
        # 1.0 of the bound there by construction (fp16 gradients under 2^-14), so the 0.5 rule is judged on the normal range
        normal = rb["gx"][0].abs() >= (2.0 ** -14 if dtype == torch.float16 else 2.0 ** -126)
        ratios.update(ddf=_ratio(ddf, *rb["ddf"]) if case["depth_feat"] is not None else 0.0, gx=_ratio(gw, *rb["gx"], normal),
                      dw=_ratio(dw, *rb["dw"]), db=_ratio(db, *rb["db"]))
        ratios["gx subnormal"] = _ratio(gw, *rb["gx"], ~normal)
        if dtype != F32:
            ratios["gx once"] = float(B.rounding_excess(gw, rb["gx"][0], dtype, rb["gx"][1]).max())
        lose = torch.ones(b, h, wd, dtype=torch.bool)
        lose[img, ih, iw] = False
        bad["zero bits"] = int((dx.view(torch.int32 if dtype == F32 else torch.int16)[lose] != 0).sum())
        old[1] = max(old_metric(dx, _dense(rb, b, h, wd, c)), old_metric(dw, rb["dw"][0]), old_metric(db, rb["db"][0]))
    return ratios, bad, old


def _dense(rb, b, h, wd, c):
    t = torch.zeros(b, h, wd, c, dtype=torch.float64)
    t[rb["winner"]] = rb["gx"][0]
    return t


def _rejected(ratios, bad):
    return any(not v <= 1.0 for v in ratios.values()) or any(bad.values())


# ------------------------------------------------------------------ references
@pytest.mark.parametrize("c,h,w,b", [(64, 16, 16, 2), (8, 7, 5, 3), (1024, 2, 2, 1)])
def test_aux_reference_is_the_oracle_head(c, h, w, b):
    """aux_fwd_ref / aux_bwd_ref equal oracle.aux_head (x depth feature) in fp64 and its autograd gradients, odd sizes included"""
    case = C.aux_case(torch.bfloat16, b, h, w, c, "relu", True)
    x64 = case["x"].double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    w64 = case["w"].double().reshape(1, c, 1, 1).requires_grad_(True)
    b64 = case["bias"].double().requires_grad_(True)
    df = case["depth_feat"].double().requires_grad_(True)
    raw = po.aux_head(x64, w64, b64)
    out = raw * df
    gx, gw, gb, gdf = torch.autograd.grad(out, (x64, w64, b64, df), case["dout"].double())
    ref = HB.aux_fwd_ref(case["x"], case["w"], case["bias"], case["depth_feat"])
    close = lambda a, r: float((a - r).abs().max()) <= 1e-12 * max(1.0, float(r.abs().max()))
    assert close(ref["raw"], raw.detach()) and close(ref["out"], out.detach())
    rb = HB.aux_bwd_ref(case["dout"], case["x"], case["w"], case["depth_feat"], ref["raw"], ref["idx"], torch.bfloat16)
    assert close(_dense(rb, b, h, w, c), gx.permute(0, 2, 3, 1)) and close(rb["dw"][0], gw.reshape(c)) and close(rb["db"][0], gb)
    assert close(rb["ddf"][0], gdf)


@pytest.mark.parametrize("h,w,pools", [(8, 12, 2), (13, 22, 1), (13, 22, 2), (13, 22, 3), (64, 128, 6), (20, 20, 2)])
def test_depth_reference_is_the_oracle_head(h, w, pools):
    """depth_fwd_ref equals oracle.depth_head for every `pools` and odd sizes; depth_bwd_ref equals autograd's dw / db"""
    case = C.depth_case(3, h, w, "uniform")
    w64, b64 = case["w"].double().requires_grad_(True), case["b"].double().requires_grad_(True)
    feat = po.depth_head(case["depth"].double()[:, None], w64, b64, pools)
    r = HB.depth_fwd_ref(case["depth"], case["w"], case["b"], pools)
    assert float((r["feat"][0] - feat.detach()).abs().max()) <= 1e-11
    d = torch.randn(feat.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    gw, gb = torch.autograd.grad(feat, (w64, b64), d)
    rb = HB.depth_bwd_ref(d, r["xhat"][0], (0.0, 0.0), 0)
    assert abs(float(rb["dw"][0] - gw)) <= 1e-10 and abs(float(rb["db"][0] - gb)) <= 1e-10


# ------------------------------------------------------------------ soundness
def depth_cases():
    for (h, w) in C.DEPTH_HW:
        for b in C.DEPTH_B:
            for kind in C.DEPTH_KINDS:
                yield "depth %s b=%d %s" % ((h, w), b, kind), C.depth_case(b, h, w, kind), 2, "quad"
                yield "depth pools=2 %s b=%d %s" % ((h, w), b, kind), C.depth_case(b, h, w, kind), 2, "wave"
    for (h, w, pools) in C.DEPTH_POOLS:
        for kind in C.DEPTH_KINDS:
            yield "depth pools=%d %s %s" % (pools, (h, w), kind), C.depth_case(2, h, w, kind), pools, "wave"


def depth_ratios(case, pools, form, mutant=None):
    xhat, feat = depth_fwd_f32(case, pools, form, mutant)
    r = HB.depth_fwd_ref(case["depth"], case["w"], case["b"], pools)
    return dict(xhat=B.check(xhat, *r["xhat"], "")[1], feat=B.check(feat, *r["feat"], "")[1]), old_metric(feat, r["feat"][0])


def test_head_kernels_stay_within_half_the_bound():
    """correct fp32 statements at <= 0.5 of every bound on every CPU-sized case; no constant was needed beyond those of _bounds.py.
    Undecided windows: at most 0.1 % of a case's random windows (none found: the smallest gap / slack is printed)."""
    worst, min_gap = {}, float("inf")

    def put(k, r):
        worst[k] = max(worst.get(k, 0.0), r)

    for dtype in C.DTYPES:
        for label, case, form in aux_cases(dtype):
            for f in ((form, "det") if form == "64" else (form,)):
                ratios, bad, _ = aux_ratios(dtype, case, f)
                assert not any(bad.values()), (label, f, bad)
                for k, r in ratios.items():
                    put("aux " + k, r)
            ref = case["_memo"]["fwd ref"]
            b, n = ref["raw"].shape
            rnd = ~_slot_mask(case, b, n, case["x"].shape[2] // 2) & ref["finite"]
            if int(rnd.sum()):
                und = int((~ref["decided"] & rnd).sum())
                assert und <= 1e-3 * int(rnd.sum()), "%s: %d of %d random windows undecided" % (label, und, int(rnd.sum()))
                min_gap = min(min_gap, float(ref["gap_over_slack"][rnd].min()))
    for label, case, pools, form in depth_cases():
        ratios, _ = depth_ratios(case, pools, form)
        for k, r in ratios.items():
            put("depth " + k, r)
        if "const" in label or case["depth"].shape[1] >> pools == 1 == case["depth"].shape[2] >> pools:
            xhat, feat = depth_fwd_f32(case, pools, form)
            assert (xhat == 0).all() and (feat == case["b"]).all(), label      # zero variance: xhat exactly 0, feat exactly b
    for n in C.DEPTH_BWD_NS:
        case = C.depth_bwd_case(n)
        dw, db = depth_bwd_f32(case, C.DEPTH_BWD_START)
        r = HB.depth_bwd_ref(case["d_feat"], case["xhat"], C.DEPTH_BWD_START, C.depth_bwd_blocks(n))
        put("depth bwd dw", B.check(dw, *r["dw"], "")[1])
        put("depth bwd db", B.check(db, *r["db"], "")[1])
    for k, r in sorted(worst.items()):
        print("soundness %-22s worst err/bound %.3f" % (k, r))
    print("smallest gap / slack of a random window: %.1f" % min_gap)
    bad = {k: r for k, r in worst.items() if not r <= (1.0 if k in ("aux gx once", "aux gx subnormal") else 0.5)}
    assert not bad, bad
    assert max(worst.values()) > 0.1, "the bounds are needlessly loose"


def test_det_y_statement_equals_det_on_the_activated_tensor():
    """the recomputation of det_y (relu(fma(y, scale, shift)) rounded to T at the winner pixel) reproduces det on a1 bit for bit"""
    for dtype in C.DTYPES:
        case = C.stem_case(dtype, 3, 6, 10, "relu", True)
        a1 = bn_act_f32(case["x"], case["scale"], case["shift"], dtype)
        acase = dict(case, x=a1)
        out, raw, idx = aux_fwd_f32(acase, dtype)
        want = aux_bwd_f32(acase, dtype, raw, idx, out, "det")
        img, ih, iw = HB.winner_pixels(idx, *a1.shape[:3])
        act = torch.zeros_like(a1)
        act[img, ih, iw] = bn_act_f32(case["x"][img, ih, iw], case["scale"], case["shift"], dtype)      # only the winners are recomputed
        got = aux_bwd_f32(acase, dtype, raw, idx, out, "det", act=act)
        assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3]) and torch.equal(got[0], want[0])


# ------------------------------------------------------------------ mutants
AUX_MUTANTS = [">= winner", "raw after depth product", "d_depth_feat from out", "gradient to tap 0", "last chunk dropped", "gradient truncated"]
DEPTH_MUTANTS = ["windows at oh H / Ho", "unbiased variance", "eps outside the root"]


def test_head_mutants_are_rejected():
    """every fault is rejected on at least one case: worst err/bound > 1, an idx mismatch or a non-zero loser; printed beside it whether
    the one-number metric of test_aux_and_depth_heads (max error / max magnitude under 1e-5 fp32, 1e-2 16-bit) would have passed it on
    EVERY case, i.e. would not have noticed"""
    missed = []
    for mutant in AUX_MUTANTS:
        hits, cases, old_pass, worst = 0, 0, True, 0.0
        for dtype in C.DTYPES:
            for label, case, form in aux_cases(dtype):
                if mutant == "last chunk dropped" and case["x"].shape[3] != 1024:
                    continue
                ratios, bad, old = aux_ratios(dtype, case, form, mutant)
                cases += 1
                hits += _rejected(ratios, bad)
                worst = max(worst, max(ratios.values()))
                old_pass &= old[0] < OLD_BAR[dtype] and old[1] < OLD_BAR_BWD[dtype]
        print("mutant %-28s rejected on %3d of %3d cases, worst err/bound %9.3g; old rel_err bar passes it everywhere: %s" % (
            mutant, hits, cases, worst, old_pass))
        if not hits:
            missed.append(mutant)
    for mutant in DEPTH_MUTANTS:
        hits, cases, old_pass, worst = 0, 0, True, 0.0
        for label, case, pools, form in depth_cases():
            if mutant == "windows at oh H / Ho" and (form != "wave" or case["depth"].shape[1:] != (13, 22)):
                continue
            ratios, old = depth_ratios(case, pools, form, mutant)
            cases += 1
            hits += not max(ratios.values()) <= 1.0
            worst = max(worst, max(ratios.values()))
            old_pass &= old < 1e-4
        print("mutant %-28s rejected on %3d of %3d cases, worst err/bound %9.3g; old rel_err bar passes it everywhere: %s" % (
            mutant, hits, cases, worst, old_pass))
        if not hits:
            missed.append(mutant)
    # det_y without the rounding of the recomputed activation to T: not bitwise det any more, and outside dw's bound
    hits = 0
    for dtype in (torch.bfloat16, torch.float16):
        case = C.stem_case(dtype, 3, 6, 10, "relu", True)
        a1 = bn_act_f32(case["x"], case["scale"], case["shift"], dtype)
        acase = dict(case, x=a1)
        out, raw, idx = aux_fwd_f32(acase, dtype)
        want = aux_bwd_f32(acase, dtype, raw, idx, out, "det")
        got = aux_bwd_f32(acase, dtype, raw, idx, out, "det", act=bn_act_f32(case["x"], case["scale"], case["shift"], dtype, rounded=False))
        rb = HB.aux_bwd_ref(case["dout"], a1, case["w"], case["depth_feat"], raw, idx, dtype)
        r = B.check(got[2], *rb["dw"], "")[1]
        old = old_metric(got[2], rb["dw"][0])
        print("mutant %-28s %-8s bitwise equal to det: %s, dw worst err/bound %9.3g; old rel_err %.2e (bar 2e-2 passes it: %s)" % (
            "det_y without rounding to T", str(dtype)[6:], torch.equal(got[2], want[2]), r, old, old < 2e-2))
        hits += (not torch.equal(got[2], want[2])) and r > 1.0
    if hits < 2:
        missed.append("det_y without rounding to T")
    assert not missed, "mutants not rejected: %s" % missed


def test_tensor_add_in_t_is_the_same_function():
    """`tensor_add accumulating in T` cannot be told from the kernel: fp32 carries p = 24 >= 2 x 11 + 2 bits, so rounding the fp32 sum
    of two 16-bit values to T is the correctly rounded sum -- what an add in T gives (Figueroa: double rounding is innocuous from
    2 p + 2 bits on).  The statement the GPU test compares with, and the add in T, agree bit for bit on every case, specials included;
    an add that ROUNDS DIFFERENTLY (toward zero) does not."""
    for dtype in (torch.bfloat16, torch.float16):
        for n in C.tensor_add_ns(dtype)[:2] + [65536]:
            dst, src = C.tensor_add_case(dtype, n, 0)
            dst[:4] = torch.tensor([float("inf"), 60000.0, 1.0, 2.0 ** -20]).to(dtype)
            src[:4] = torch.tensor([float("-inf"), 60000.0, 2.0 ** -12, -2.0 ** -20]).to(dtype)
            want = (dst.float() + src.float()).to(dtype)
            eq = lambda a, b: torch.equal(a.view(torch.int16)[~a.isnan()], b.view(torch.int16)[~a.isnan()]) and torch.equal(a.isnan(), b.isnan())
            assert eq(dst + src, want)
            if n > 1000:
                assert not eq(_rtz(dst.float() + src.float(), dtype), want)
    print("mutant tensor_add accumulating in T: the same function bit for bit (24 >= 2 x 11 + 2): no test can reject it")
