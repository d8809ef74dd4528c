"""fp64 references with element-wise bounds for the head kernels of csrc/heads.hip: the aux head (C = 64 and any C), its backward
forms, the depth heads and their backward.  Built on tests/_bounds.py: LAM, EPI, EW, TR, U_OUT and FLOOR are used unchanged, no constant
is added here.  Every reference is computed from the already rounded operands the kernel reads, on their device.

aux forward.  Per pixel d = x . w + bias is a GEMM row of K = C terms accumulated in fp32: B.bound(r, float32, epi=|acc| + |bias|).
raw = max of the window's four d: max is 1-Lipschitz, so raw errs by at most the largest of the four taps' bounds.  out = raw
depth_feat: EPI u32 |out| for the product plus |depth_feat| times raw's bound.  The winner tap is an integer: a window is DECIDED when
the fp64 gap between its best tap and every other tap exceeds the sum of their two bounds (a tap whose pixel equals the winner's pixel
bit for bit does not count: it has the winner's value in any arithmetic) -- there idx must be the fp64 argmax; elsewhere
idx must name a tap that a correct kernel could have seen as largest: its fp64 value within (its own bound + the maximum's bound) of
the maximum.  First tap in scan order wins a tie (`>`), a NaN tap wins over everything before it and keeps the window.

aux backward, from the forward's own raw / idx: d = dout depth_feat; d_depth_feat = dout raw (one product: EW u32 |ref|); the feature
gradient at the winner pixel is round_T(d w_c): 2 u_out |ref| + EPI u32 |ref| + floor and rounds once; every other element is +0 bit
for bit; dw[c] = sum over the windows of d x[winner, c] and dbias = sum d are fp32 sums of K = B Ho Wo terms: B.bound(r, float32).  A
form that accumulates onto a start value s in G steps (one atomic add per block) adds the rounding of those G adds, by the same
statistics as any fp32 sum: LAM u32 sqrt(G) (|s| + |sum|).

depth heads.  pooled = mean of the win x win window, an fp32 sum of K = win^2 terms times the exact 1 / win^2: B.bound(r, float32) = bp.
The statistics are formed in double from the fp32 pooled values p_i + e_i, |e_i| <= bp_i, so they only inherit that error:
    d mean <= mean(bp)
    d var  <= (2 / n) sum |p_i - mean| bp_i + mean(bp^2)              (d var / d p_i = 2 (p_i - mean) / n, plus the second order)
              + 8 u64 mean(p^2)                                       (q / n - mean^2 cancels in double)
(float)mean costs u32 |mean| more.  invstd = (float)(1 / sqrt(var + eps)) is taken at its worst end, (var + eps - d var)^-1/2, plus
u32 invstd for the cast.  Then xhat = (p - mean) invstd and feat = xhat w + b propagate through Fx: the subtraction adds
EW u32 (|p| + |mean|), which invstd magnifies -- the ill-conditioned direction of an image whose offset is far above its spread.

CPU self-test (tests/test_heads_cpu.py: fp32 statements of the kernels in their own association, on every case of _head_cases.py that
is small enough for the CPU); worst err/bound of a correct statement, no constant tuned:
    aux forward   raw 0.11   out 0.12        aux backward  d_depth_feat 0.33   dw 0.20   dbias 0.12
    feature gradient 0.50 where |ref| is a normal number of T, rounds-once 1.00 (ties: half an ulp exactly); 0.95 among fp16 subnormals,
    where the rounding step is the subnormal spacing and half of it IS the floor -- there a correct kernel reaches 1.0 by construction
    depth forward xhat 0.06   feat 0.06      depth backward dw 0.01   db 0.002
    smallest gap / slack of a random window: 5.9 (at C = 256; 13 at C = 64); undecided random windows: none
The kernels on an MI355X (tests/test_gpu_heads.py prints the BOUND / ONCE lines): raw 0.11, out 0.12, d_depth_feat 0.33, feature
gradient 0.50 / 0.95 / 1.00 as above, dw 0.20, dbias 0.12, depth xhat 0.05, feat 0.06, depth backward 0.02."""
import torch

import _bounds as B
from _bounds import EPI, EW, F32_FLOOR, FLOOR, LAM, U32, U_OUT, Fx

U64 = 2.0 ** -53
F32 = torch.float32


def taps(t, ho, wo):
    """[B, H, W, ...] -> [B, Ho, Wo, 4, ...]: tap k = 2 (row in the window) + (column in the window); an odd last row / column is
    dropped"""
    b, rest = t.shape[0], tuple(t.shape[3:])
    dims = tuple(range(5, 5 + len(rest)))
    return t[:, :2 * ho, :2 * wo].reshape((b, ho, 2, wo, 2) + rest).permute((0, 1, 3, 2, 4) + dims).reshape((b, ho, wo, 4) + rest)


def scan_winner(dt, ge=False):
    """the kernels' winner rule over the last axis (4 taps): `d > best || d != d`, from best = -inf (ge: the faulty `>=`)"""
    best, bi = dt[..., 0].clone(), torch.zeros(dt.shape[:-1], dtype=torch.long, device=dt.device)
    for k in range(1, dt.shape[-1]):
        v = dt[..., k]
        m = ((v >= best) if ge else (v > best)) | v.isnan()
        best, bi = torch.where(m, v, best), torch.where(m, torch.full_like(bi, k), bi)
    return best, bi


def aux_fwd_ref(x, w, bias, depth_feat):
    """x [B, H, W, C] (compute type), w [C], bias [1], depth_feat [B, Ho Wo] or None -> dict of fp64 [B, Ho Wo] tensors: raw, braw,
    out, bout, idx (long), decided (bool), finite (bool: no NaN tap), and d, bd [B, Ho Wo, 4] (the taps and their bounds)"""
    b, h, wd, c = x.shape
    ho, wo = h // 2, wd // 2
    r = B.gemm_ref(x.reshape(-1, c), w.reshape(1, c))
    acc, bias64 = r.acc.reshape(b, h, wd), bias.double()
    d = acc + bias64
    bd = B.bound(B.Ref(acc, r.Q.reshape(b, h, wd), c), F32, out=d, epi=acc.abs() + bias64.abs())
    dt, bt = taps(d, ho, wo).reshape(b, ho * wo, 4), taps(bd, ho, wo).reshape(b, ho * wo, 4)
    raw, idx = scan_winner(dt)
    finite = torch.isfinite(dt).all(-1)
    braw = bt.max(-1).values
    # contenders: taps a correct kernel may see at or above the winner; a contender whose pixel is the winner's pixel bit for bit has the
    # winner's d bit for bit in any arithmetic, so the scan order decides between them (all-zero pixels of post-ReLU features)
    xt = taps(x, ho, wo).reshape(b, ho * wo, 4, c)
    twin = (xt == xt.gather(2, idx[..., None, None].expand(-1, -1, 1, c))).all(-1)
    slack = bt + braw[..., None]
    rival = (raw[..., None] - dt <= slack) & ~twin
    ratio = torch.where(twin | ~finite[..., None], torch.full_like(dt, float("inf")), (raw[..., None] - dt) / slack)
    df = torch.ones_like(raw) if depth_feat is None else depth_feat.double()
    out = raw * df
    bout = EPI * U32 * out.abs() + df.abs() * braw + F32_FLOOR
    return dict(d=dt, bd=bt, raw=raw, braw=braw, out=out, bout=bout, idx=idx, decided=~rival.any(-1) & finite, finite=finite,
                gap_over_slack=ratio.min(-1).values)


def idx_errors(idx_got, ref):
    """-> number of windows (without a NaN tap) whose winner tap a correct kernel cannot have chosen"""
    got = idx_got.to(ref["idx"].device).long()
    if int((got > 3).sum()):
        return int((got > 3).sum())
    dsel = ref["d"].gather(-1, got[..., None])[..., 0]
    bsel = ref["bd"].gather(-1, got[..., None])[..., 0]
    ok = torch.where(ref["decided"], got == ref["idx"], ref["raw"] - dsel <= bsel + ref["braw"])
    return int((~ok & ref["finite"]).sum())


def winner_pixels(idx, b, h, wd):
    """idx [B, Ho Wo] -> (image, row, column) index tensors of the winner pixels, each [B, Ho Wo]"""
    ho, wo = h // 2, wd // 2
    idx = idx.long()
    pos = torch.arange(ho * wo, device=idx.device)[None].expand(b, -1)
    img = torch.arange(b, device=idx.device)[:, None].expand(-1, ho * wo)
    return img, 2 * (pos // wo) + (idx >> 1), 2 * (pos % wo) + (idx & 1)


def accum_bound(r, start, steps):
    """(reference, bound) of start + r.acc where the kernel adds its sum onto `start` in `steps` fp32 adds (steps = 0: it overwrites)"""
    ref = r.acc + start
    bnd = B.bound(r, F32)
    if steps:
        bnd = bnd + LAM * U32 * steps ** 0.5 * (abs(start) + r.acc.abs())
    return ref, bnd


def aux_bwd_ref(dout, x, w, depth_feat, raw, idx, dtype, start=(0.0, 0.0), steps=0):
    """The aux backward from the forward's OWN raw / idx (as the engine feeds it).  dout, raw [B, Ho Wo] fp32, x [B, H, W, C] -> dict:
    ddf (ref, bound) [B, Ho Wo]; gx (ref, bound) [B, Ho Wo, C] at the winner pixels; winner (img, row, col); dw (ref, bound) [C];
    db (ref, bound) [1].  start / steps: see accum_bound (dw, dbias start values)."""
    b, h, wd, c = x.shape
    d = dout.double() * (1.0 if depth_feat is None else depth_feat.double())
    ddf = dout.double() * raw.double()
    img, ih, iw = winner_pixels(idx, b, h, wd)
    xw = x[img, ih, iw].double()                                           # [B, n, C]
    gx = d[..., None] * w.double()
    bgx = 2.0 * U_OUT[dtype] * gx.abs() + EPI * U32 * gx.abs() + FLOOR[dtype]
    dcol = d.reshape(-1, 1)
    rw = B.gemm_ref_tn(dcol, xw.reshape(-1, c))
    rb = B.gemm_ref_tn(dcol, torch.ones_like(dcol))
    dw, bdw = accum_bound(rw, start[0], steps)
    db, bdb = accum_bound(rb, start[1], steps)
    return dict(ddf=(ddf, EW * U32 * ddf.abs() + F32_FLOOR), gx=(gx, bgx), winner=(img, ih, iw), dw=(dw.reshape(c), bdw.reshape(c)),
                db=(db.reshape(1), bdb.reshape(1)))


def depth_windows(depth, pools, anchor=None):
    """depth [B, H, W] -> [B, Ho, Wo, win^2] with Ho = H >> pools: the window of output (oh, ow) starts at (oh, ow) 2^pools, which is
    what `pools` flooring AvgPool2d(2) steps read (anchor: a faulty start row / column rule, for the self-test)"""
    b, h, w = depth.shape
    win, ho, wo = 1 << pools, h >> pools, w >> pools
    if anchor is None:
        return depth[:, :ho * win, :wo * win].reshape(b, ho, win, wo, win).permute(0, 1, 3, 2, 4).reshape(b, ho, wo, win * win)
    r0 = torch.tensor([anchor(o, h, ho) for o in range(ho)])
    c0 = torch.tensor([anchor(o, w, wo) for o in range(wo)])
    rr = (r0[:, None] + torch.arange(win)[None]).to(depth.device)          # [Ho, win]
    cc = (c0[:, None] + torch.arange(win)[None]).to(depth.device)          # [Wo, win]
    return depth[:, rr[:, None, :, None], cc[None, :, None, :]].reshape(b, ho, wo, win * win)


def depth_fwd_ref(depth, w, bias, pools=2, eps=1e-5):
    """rpe_depth_head_fwd (pools = 2) / rpe_depth_head_fwd_pools in fp64 from the fp32 image [B, H, W] -> {xhat, feat: (reference,
    bound)} [B, Ho Wo] and pooled (reference, bound).  The derivation is in the module comment."""
    b = depth.shape[0]
    win2 = (1 << pools) ** 2
    wnd = depth_windows(depth, pools)
    n = wnd.shape[1] * wnd.shape[2]
    r = B.gemm_ref(wnd.reshape(-1, win2), torch.full((1, win2), 1.0 / win2, dtype=torch.float64, device=depth.device))
    p, bp = r.acc.reshape(b, n), B.bound(r, F32).reshape(b, n)
    mean = p.mean(1, keepdim=True)
    var = ((p - mean) ** 2).mean(1, keepdim=True)
    dmean = bp.mean(1, keepdim=True)
    dvar = (2.0 * (p - mean).abs() * bp).mean(1, keepdim=True) + (bp * bp).mean(1, keepdim=True) + 8.0 * U64 * (p * p).mean(1, keepdim=True)
    v = var + eps
    invstd = v.rsqrt()
    dinv = (v - dvar).clamp_min(eps * 1e-3).rsqrt() - invstd + U32 * invstd
    xhat = (Fx(p, bp) - Fx(mean, dmean + U32 * mean.abs())) * Fx(invstd, dinv)
    feat = xhat * Fx(w.double()) + Fx(bias.double())
    return dict(xhat=xhat.out(), feat=feat.out(), pooled=(p, bp))


def depth_bwd_ref(d_feat, xhat, start, steps):
    """rpe_depth_head_bwd: dw = start[0] + sum d xhat, db = start[1] + sum d, fp32 sums of n terms added in `steps` atomic adds"""
    d = d_feat.double().reshape(-1, 1)
    dw = accum_bound(B.gemm_ref_tn(d, xhat.double().reshape(-1, 1)), start[0], steps)
    db = accum_bound(B.gemm_ref_tn(d, torch.ones_like(d)), start[1], steps)
    return dict(dw=(dw[0].reshape(1), dw[1].reshape(1)), db=(db[0].reshape(1), db[1].reshape(1)))
