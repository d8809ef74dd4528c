"""Inputs of the element-wise tests of the pooling and stem-backward kernels of csrc/norm.hip (rpe_maxpool3x3s2_fwd / _bwd,
rpe_bn_apply_maxpool3x3s2, rpe_stem_bwd, rpe_avgpool_fwd / _bwd), shared by the CPU self-test (tests/test_pool_cpu.py) and the GPU test
(tests/test_gpu_pool.py), so that the bounds of tests/_pool_bounds.py are judged on the very inputs the kernels are held to.  CPU
tensors, NHWC, in the compute type.

The launchers' own arithmetic is restated here (stem_bwd_launch, the switch of rpe_avgpool_fwd): the bounds take the rows per block
from it, the restatements of the self-test their association, and each shape below is the smallest that reaches the code path named
beside it (asserted by test_pool_cpu.py::test_cases_reach_their_paths)."""
import torch

from _norm_cases import BF16, CE, DTYPES, EPS, F16, F32, GUARD, _seed      # noqa: F401  (re-exported)

NAN, NINF = float("nan"), float("-inf")


def pooled(n):
    """extent of the 3x3 / stride 2 / pad 1 pool's output"""
    return (n - 1) // 2 + 1


# ------------------------------------------------------------------ launcher arithmetic
def stem_geometry(b, h, w, part_floats, dtype):
    """stem_bwd_launch -> dict(ppb, nbl, rpb, nb, apply_blocks, rows, wo), or None where it refuses the workspace: the reduce pass runs
    nb blocks of rpb consecutive pooled rows (two image rows each), a block walks a pooled row in passes of ppb pixels; the apply pass
    takes two pooled rows per block"""
    ho, wo = pooled(h), pooled(w)
    rows = b * ho
    nbl = min(part_floats // 128, 1024, rows)
    if nbl < 1:
        return None
    rpb = (rows + nbl - 1) // nbl
    return dict(ppb=256 // (64 // CE[dtype]), nbl=nbl, rpb=rpb, nb=(rows + rpb - 1) // rpb, apply_blocks=(rows + 1) // 2, rows=rows, wo=wo)


def avgpool_few(b, hw, c):
    """rpe_avgpool_fwd takes the 8-lanes-per-chunk kernel"""
    return b * c <= 65536 and hw >= 16


# ------------------------------------------------------------------ max pool
def maxpool_shapes(dtype):
    """(B, H, W, C): one tap; one window; odd sizes (the bottom row and right column of taps are out of the image); the general case;
    chunks per pixel not a power of two; more than one block"""
    ce = CE[dtype]
    return [(1, 1, 1, ce), (1, 2, 2, ce), (2, 5, 7, 2 * ce), (3, 6, 10, 64), (1, 8, 4, 3 * ce), (1, 34, 18, 64)]


MAXPOOL_KINDS = ("signed", "relu-like")
CONSTRUCTED = (3, 6, 10, 64)                # the shape whose last chunk (image 0) carries the constructed windows
PEAK = (3, 3)                               # odd (h, w): the pixel wins windows (1, 1) tap 8, (1, 2) tap 6, (2, 1) tap 2, (2, 2) tap 0


def maxpool_case(dtype, shape, kind):
    """-> dict(x [B, H, W, C], dout [B, Ho, Wo, C], addend [B, H, W, C] in dtype, expect: {(b, oh, ow, c): tap} for the constructed
    windows).  signed: randn - 0.5 (many window maxima are negative: padding counted as 0 shows); relu-like: clamp_min(0), about half
    zeros (ties everywhere).  Channel k of the last chunk of image 0 of CONSTRUCTED holds
      0: one value everywhere -- every tap ties, the first in-image one wins;
      1: -inf everywhere -- windows of nothing but -inf at a corner, at an edge and in the interior name their first in-image tap;
      2: a NaN at tap 0 of window (1, 1) with a larger finite value behind it (the NaN stays), and two NaNs in window (1, 3), at taps
         0 and 8 (the later one is named);
      3: a peak at PEAK that wins four windows (the backward's five-term sum with the addend)."""
    b, h, w, c = shape
    g = _seed(b, h, w, c, DTYPES.index(dtype), MAXPOOL_KINDS.index(kind))
    x = torch.randn(b, h, w, c, generator=g)
    x = (x - 0.5 if kind == "signed" else x.clamp_min(0)).to(dtype)
    expect = {}
    if shape == CONSTRUCTED:
        c0 = c - CE[dtype]
        x[0, :, :, c0] = 0.75
        x[0, :, :, c0 + 1] = NINF
        for (oh, ow) in ((0, 0), (0, 2), (1, 0), (1, 2)):       # corner, top edge, left edge, interior
            first = (3 if oh == 0 else 0) + (1 if ow == 0 else 0)
            expect[(0, oh, ow, c0)] = first
            expect[(0, oh, ow, c0 + 1)] = first
        x[0, 1, 1, c0 + 2], x[0, 2, 2, c0 + 2] = NAN, 100.0
        expect[(0, 1, 1, c0 + 2)] = 0
        x[0, 1, 5, c0 + 2], x[0, 3, 7, c0 + 2] = NAN, NAN
        expect[(0, 1, 3, c0 + 2)] = 8
        x[0, PEAK[0], PEAK[1], c0 + 3] = 50.0
        expect.update({(0, 1, 1, c0 + 3): 8, (0, 1, 2, c0 + 3): 6, (0, 2, 1, c0 + 3): 2, (0, 2, 2, c0 + 3): 0})
    return dict(x=x, dout=torch.randn(b, pooled(h), pooled(w), c, generator=g).to(dtype), addend=torch.randn(b, h, w, c, generator=g).to(dtype),
                expect=expect)


def fused_shapes(dtype):
    """rpe_bn_apply_maxpool3x3s2: the even-sized max-pool shapes with C % 8 == 0"""
    return [s for s in maxpool_shapes(dtype) if s[1] % 2 == 0 and s[2] % 2 == 0 and s[3] % 8 == 0]


def fused_case(dtype, shape):
    """-> dict(y [B, H, W, C] in dtype, scale, shift [C]); every fifth scale negative, about 60 % of the activations zero"""
    b, h, w, c = shape
    g = _seed(b, h, w, c, DTYPES.index(dtype), 9)
    scale = 0.5 + torch.rand(c, generator=g)
    scale[::5] *= -1
    return dict(y=torch.randn(b, h, w, c, generator=g).to(dtype), scale=scale, shift=torch.rand(c, generator=g) - 0.7)


# ------------------------------------------------------------------ stem backward
# (B, H, W, part_floats), 64 channels: one window (no right or below neighbour, one block, one slice); Wo = 34 (a second and third pass
# over a pooled row in fp32: 16 + 16 + 2, a second in the 16-bit types: 32 + 2), one pooled row per block; two reduce blocks of five pooled
# rows, the first crossing from image 0 into image 1, the last ragged (4 rows), nine pooled rows: the apply pass ends in a one-row
# block; B Ho = 1025 > the cap of 1024 blocks: rpb = 2, 513 blocks, ragged last, 64 slices in reduce_finalize; three blocks of 5, 5, 4
STEM_SHAPES = [(1, 2, 2, 128), (3, 4, 68, 128 * 1024), (3, 6, 70, 256), (1, 2050, 2, 128 * 4096), (2, 14, 10, 128 * 3)]
STEM_AUX = ("none", "aux", "aux x depth")
STEM_ZERO = (0, 1, 1, 63)                   # (b, h, w, channel) of the constructed pre-activation of exactly +0
DPART_DOUBLES = 256 * 2 * 64 + 64           # RPE_BN_DPART_DOUBLES(64)


def stem_case(dtype, shape, aux):
    """-> dict(y [B, H, W, 64], dpool [B, Ho, Wo, 64] in dtype, pool_idx uint8 [B, Ho, Wo, 64], gamma, mean, invstd, scale, shift [64],
    zero: STEM_ZERO, and with an aux head aux_idx uint8 [B, Ho Wo], aux_dout [B, aux_ld], aux_ld, aux_w [64], depth_feat [B, Ho Wo] or
    None).  y = 1.5 randn + 0.2, every seventh gamma negative, mean and invstd from y in double; pool_idx are the reference forward's
    winners on round_T(relu(y scale + shift)).  At STEM_ZERO y = 0 and the channel's shift is 0: the pre-activation is exactly +0, the
    pixel gets no gradient although the aux head (where there is one) names it."""
    from _pool_bounds import maxpool_ref
    b, h, w, _ = shape
    ho, wo = h // 2, w // 2
    g = _seed(b, h, w, DTYPES.index(dtype), STEM_AUX.index(aux), 5)
    y = (torch.randn(b, h, w, 64, generator=g) * 1.5 + 0.2).to(dtype)
    zb, zh, zw, zc = STEM_ZERO
    y[zb, zh, zw, zc] = 0.0
    gamma = 0.5 + torch.rand(64, generator=g)
    gamma[::7] *= -1
    beta = torch.randn(64, generator=g) * 0.3
    yd = y.double()
    mean = yd.mean((0, 1, 2))
    invstd = (yd.var((0, 1, 2), unbiased=False) + EPS).rsqrt().float()
    mean = mean.float()
    scale = gamma * invstd
    shift = beta - mean * scale
    shift[zc] = 0.0
    a = (yd * scale.double() + shift.double()).clamp_min(0.0).to(dtype)
    d = dict(y=y, dpool=torch.randn(b, ho, wo, 64, generator=g).to(dtype), pool_idx=maxpool_ref(a)[1], gamma=gamma, mean=mean, invstd=invstd,
             scale=scale, shift=shift, zero=STEM_ZERO, aux_idx=None, aux_dout=None, aux_ld=0, aux_w=None, depth_feat=None)
    if aux != "none":
        n = ho * wo
        idx = torch.randint(0, 4, (b, n), generator=g).to(torch.uint8)
        idx[zb, (zh // 2) * wo + zw // 2] = (zh % 2) * 2 + zw % 2
        d.update(aux_idx=idx, aux_dout=torch.randn(b, n + 4, generator=g), aux_ld=n + 4, aux_w=torch.randn(64, generator=g) * 0.2)
        if aux == "aux x depth":
            d["depth_feat"] = torch.rand(b, n, generator=g) + 0.5
    return d


# ------------------------------------------------------------------ average pool
def avgpool_shapes(dtype):
    """(B, HW, C).  Plain kernel: HW < 16 (a block with idle threads among them), B C > 65536.  8-lanes-per-chunk kernel: 8 live lanes
    in a block of 256; a ragged pixel tail; the engine's shape; B C = 65536 exactly"""
    ce = CE[dtype]
    return [(2, 1, 2 * ce), (2, 9, ce), (2, 15, 64), (33, 16, 2048), (1, 16, ce), (2, 17, 64), (3, 49, 2048), (32, 16, 2048)]


def avgpool_bwd_shapes(dtype):
    """the same, and a chunk count per row that is not a power of two"""
    return avgpool_shapes(dtype) + [(2, 9, 3 * CE[dtype])]


def avgpool_case(dtype, shape):
    """-> dict(x [B, HW, C] in dtype (randn + 0.5), dout [B, C] fp32)"""
    b, hw, c = shape
    g = _seed(b, hw, c, DTYPES.index(dtype), 13)
    return dict(x=(torch.randn(b, hw, c, generator=g) + 0.5).to(dtype), dout=torch.randn(b, c, generator=g))


# ------------------------------------------------------------------ refusals
def refused_channels(dtype):
    """a channel count that is no whole number of 16-byte chunks: C = 6 in fp32, C = CE + 4 in the 16-bit types"""
    return 6 if dtype == F32 else CE[dtype] + 4
