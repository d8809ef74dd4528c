"""fp64 references, with element-wise bounds, of the front end: image staging, weight packing, the stem conv and its weight gradient, and
the small fp32 utilities of csrc/heads.hip.

Every reference is computed from the operands the kernel reads (the staged x4 and the packed weight read back, never the fp32 masters
behind them), on the device of those operands, so that each kernel answers for its own error only.  No constant is introduced:

- the stem forward and both weight gradients are GEMMs: B.conv_fwd_ref (K = 147) / B.conv_wgrad_ref (K = M) with B.bound; the affine
  form adds the fp32 epilogue's share (epi = |acc| + |bias|); the BN partial sums go through B.assert_stats;
- the packing kernels round once: bit for bit torch's fp32 product w * scale[co] rounded to T (a NaN for a NaN); the unpacking and
  rpe_stage_image_nhwc4 do no arithmetic at all;
- the frame staging is ((float) p * (1 / 255.f) - m) * (1.f / std): Fx propagation with the two constants as Fx.const, then one rounding
  into the compute type (NB.out_bound).  A byte step is 1 / (255 std) ~ 0.017 (0.002 at the gross std of 2), orders of magnitude above
  the bound (~1e-6 in fp32, an ulp in 16 bits), so a wrong source pixel cannot pass.  The integer resize in front of it is exact:
  oracle.pil_resize.resize_bilinear_u8, pinned to Pillow by test_oracle_golden;
- rpe_colsum is one fp32 sum over the rows: B.bound(Ref(sum, sqrt(sum of squares), rows), fp32), plus EPI u32 (|old| + |sum|) when it
  accumulates.

tests/test_stem_cpu.py holds torch-fp32 restatements of the kernels, in the kernels' own association, to <= 0.5 of each of these on the
cases of tests/_stem_cases.py.  Worst err/bound there, per kernel (the 16-bit types set every figure near 0.5: one rounding is half
of the two the bound allows, and assert_rounds_once holds them to that one, at 0.999 of half an ulp plus the accumulation's share):

    stem forward y 0.497, BN partial sums 0.068, affine form 0.498
    weight gradient in slab order 0.185, the splits reversed (the atomic form has no order) 0.185, accumulating into a prefill 0.175
    frame staging with the multiply-subtract separate 0.489, contracted to an FMA 0.489; behind the resize 0.480 both ways
    colsum 0.102, accumulating 0.181

and the faults it rejects, with the number of those cases on which the checks the suite had before pass them: rel_err < tol(dtype) on
the 64 x 64 shape for the conv and the packing; for the staging allclose(rtol = 1e-4) on a model output, fp32 only (16-bit cases
count as passed), stood in for on the CPU by conv1 -> ReLU -> global average of the staged image; faults no old check looks at count
as passed throughout -- rejected on / passed by the old checks on:

    a crop one row low                        12 /  8     mean / std channels swapped                24 / 16
    channel 3 not zeroed                      12 / 12     a border element written                   12 / 12
    truncation instead of nearest-even        24 / 24     scale applied after the 16-bit rounding     2 /  2
    scale applied to wd as well                6 /  6     tap row 7 included in the forward          21 / 21
    rows past M entering the BN sums          15 / 15     second image of a tile at the first's      12 / 12
    ties -> floor in crop_origin               3 /  3     vertical pass skipped                       9 /  6
    horizontal intermediate not rounded        6 /  4

(the 64 x 64 shape has neither a ragged tile nor a tile of two images, and its packed weight's tap row 7 is zero: three of the forward
faults do not change its result at all)."""
import numpy as np
import torch

import _bounds as B
import _norm_bounds as NB
from _bounds import Fx

PAD = 3


# ------------------------------------------------------------------ the staged image and the packed weight, as the kernels read them
def x4_image(x4, h, w):
    """x4 [B, H + 6, W + 6, 4] -> the image [B, 3, H, W] the stem reads (x4's own type)"""
    return x4[:, PAD:PAD + h, PAD:PAD + w, :3].permute(0, 3, 1, 2)


def x4_border(b, h, w, device="cpu"):
    """bool [B, H + 6, W + 6, 4]: the elements no staging kernel may write"""
    m = torch.ones(b, h + 2 * PAD, w + 2 * PAD, 4, dtype=torch.bool, device=device)
    m[:, PAD:PAD + h, PAD:PAD + w] = False
    return m


def packed_weight(wp):
    """w_packed [64, 8, 8, 4] -> OIHW [64, 3, 7, 7]"""
    return wp[:, :7, :7, :3].permute(0, 3, 1, 2)


def pack_stem_ref(w, scale, dtype):
    """rpe_pack_stem_weight: [64][8][8][4], tap row / column 7 and channel 3 zero, (w * scale[co]) formed in fp32 and rounded once"""
    p = torch.zeros(64, 8, 8, 4, dtype=torch.float32, device=w.device)
    p[:, :7, :7, :3] = w.permute(0, 2, 3, 1)
    if scale is not None:
        p = p * scale.view(64, 1, 1, 1)
    return p.to(dtype)


def unpack_stem_ref(dp):
    """rpe_unpack_stem_grad: [64][8][8][4] -> OIHW [64, 3, 7, 7], a pure permutation"""
    return dp.view(64, 8, 8, 4)[:, :7, :7, :3].permute(0, 3, 1, 2).contiguous()


def pack_ref(src, scale, dtype):
    """rpe_pack_conv_weight(s_multi) of one layer, src [Co, RS, Ci] fp32 -> (wf [Co, RS, Ci]: fp32 w * scale[co] rounded once, wd
    [Ci, RS, Co]: unscaled)"""
    wf = src if scale is None else src * scale.view(-1, 1, 1)
    return wf.to(dtype), src.permute(2, 1, 0).contiguous().to(dtype)


# ------------------------------------------------------------------ stem conv
def stem_fwd_ref(x4, wp, h, w):
    """B.Ref of conv1 from the staged image and the packed weight: acc / Q [B, Ho, Wo, 64], K = 147"""
    return B.conv_fwd_ref(x4_image(x4, h, w), packed_weight(wp), 2, 3)


def affine_ref(r, bias, relu, dtype):
    """rpe_stem_conv_fwd_affine: out = [relu](acc + bias) -> (reference, bound)"""
    bb = bias.double()
    v = r.acc + bb
    ref = v.clamp_min(0.0) if relu else v
    return ref, B.bound(r, dtype, out=ref, epi=r.acc.abs() + bb.abs())


def stem_wgrad_ref(x4, dy, h, w):
    """B.Ref of conv1's weight gradient from the staged image and dy [B, Ho, Wo, 64]: acc / Q [64, 7, 7, 3], K = M"""
    return B.conv_wgrad_ref(x4_image(x4, h, w), dy.permute(0, 3, 1, 2), 7, 2, 3)


def packed_grad(dwp):
    """the gradient entries of dw_packed [64][8][8][4] as [64, 7, 7, 3] (tap row / column 7 are not gradients)"""
    return dwp.view(64, 8, 8, 4)[:, :7, :7, :3]


# ------------------------------------------------------------------ frame staging
def normalise_ref(p, mean, std, dtype):
    """p [..., 3] (byte values, any integer type), mean / std [3] fp32 as the kernel receives them -> (reference, bound) of
    ((float) p * (1 / 255.f) - m) * (1.f / std) stored in dtype"""
    m, s = mean.double().to(p.device), std.double().to(p.device)
    v = (Fx(p.double()) * Fx.const(1.0 / 255.0) - Fx(m)) * Fx(1.0 / s, B.U32 * (1.0 / s))
    return v.v, NB.out_bound(v.v, v.e, dtype)


def window(frames, top, left, h, w):
    return frames[:, top:top + h, left:left + w]


def resize_u8(frames, hr, wr):
    """Pillow's 8-bit bilinear resample of every frame (uint8 [B, Hs, Ws, 3], on any device) -> uint8 [B, Hr, Wr, 3]"""
    from oracle.pil_resize import resize_bilinear_u8
    a = frames.cpu().numpy()
    return torch.from_numpy(np.stack([resize_bilinear_u8(f, hr, wr) for f in a])).to(frames.device)


# ------------------------------------------------------------------ small utilities
def colsum_ref(x, cols, old=None):
    """rpe_colsum of x [rows, ld] over its first `cols` columns (old: what `out` held, with accumulate = 1) -> (reference, bound)"""
    v = x[:, :cols].double()
    s = v.sum(0)
    bnd = B.bound(B.Ref(s, (v * v).sum(0).sqrt(), v.shape[0]), torch.float32)
    if old is None:
        return s, bnd
    o = old.double()
    return o + s, bnd + B.EPI * B.U32 * (o.abs() + s.abs())
