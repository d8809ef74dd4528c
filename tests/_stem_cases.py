"""Inputs of the direct tests of the front end -- image staging (rpe_stage_image_nhwc4, rpe_stage_frames_u8, rpe_stage_frames_u8_resized),
weight packing (rpe_pack_stem_weight, rpe_pack_conv_weights_multi), the stem conv (rpe_stem_conv_fwd / _fwd_affine, rpe_stem_conv_wgrad /
_wgrad_det, rpe_unpack_stem_grad) and the small fp32 utilities (rpe_transpose_f32, rpe_colsum, rpe_copy2d, rpe_relu_bwd) -- shared by
the CPU self-test (tests/test_stem_cpu.py) and the GPU test (tests/test_gpu_stem.py), so that the bounds of tests/_stem_bounds.py are
judged on the very inputs the kernels are held to.  CPU tensors.

The launchers' own arithmetic is restated here (launch_nt_cfg<T, 2, 64, 4, MODE_STEM>: 128-row tiles; launch_tn_cfg<T, 64, 256,
MODE_CONV> with plan_tn_cfg: the split of M; pack_conv_weights_multi_kernel: tiled or element-wise per 4096-element chunk), and each
case below is the smallest that reaches the code path named beside it (asserted by test_stem_cpu.py::test_cases_reach_their_paths)."""
import math

import torch

from _norm_cases import BF16, CE, DTYPES, F16, F32, GUARD, _seed      # noqa: F401  (re-exported)

PAD = 3                                     # RPE_STEM_PAD
NAN, INF = float("nan"), float("inf")
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
GROSS_MEAN, GROSS_STD = (0.1, 0.5, 0.9), (0.05, 0.3, 2.0)      # channels that differ grossly: a swapped channel is a large error
NORMS = (("imagenet", IMAGENET_MEAN, IMAGENET_STD), ("gross", GROSS_MEAN, GROSS_STD))


def f32(v):
    """Python doubles as the kernel receives them through float arguments"""
    return torch.tensor(v, dtype=torch.float32)


# ------------------------------------------------------------------ stem conv: launcher arithmetic
BM = 128                                    # launch_nt_cfg<T, 2, 64, 4, MODE_STEM>: BM = 64 * WAVES_M

# (B, H, W), H and W even: what each one reaches (test_cases_reach_their_paths)
STEM_SHAPES = [
    (1, 8, 8),          # M = 16: a single ragged tile
    (3, 10, 14),        # M = 105: one tile spanning three images, ragged
    (5, 12, 20),        # M = 300: tiles that start inside an image and span three, a 44-row tail
    (2, 30, 18),        # 135 rows per image: the tile edge falls inside an output row, H > W
    (2, 16, 32),        # 128 rows per image: the aligned case, W > H
    (130, 8, 8),        # 16 rows per image: eight images per tile, tile_b0 > 0 in most tiles; the only one whose weight gradient splits M
    (1, 64, 48),        # six full tiles of one image
]
OLD_SHAPE = (2, 64, 64)                     # test_stem_conv's only shape


def out_hw(h, w):
    """conv1's output dims (7 x 7 / 2, pad 3) of an even-sized image"""
    return (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1


def fwd_tiles(b, h, w):
    """-> (M, [dict(m0, rows, b0: tile_b0, b1: the last row's image, mid: the tile starts inside an image, cut: inside an output row)])"""
    ho, wo = out_hw(h, w)
    hw, m = ho * wo, b * ho * wo
    tiles = []
    for m0 in range(0, m, BM):
        m1 = min(m, m0 + BM)
        tiles.append(dict(m0=m0, rows=m1 - m0, b0=m0 // hw, b1=(m1 - 1) // hw, mid=m0 % hw != 0, cut=m0 % wo != 0))
    return m, tiles


def wgrad_plan(b, h, w, dtype):
    """launch_tn_cfg<T, 64, 256, MODE_CONV> + plan_tn_cfg for the stem (one 64 x 256 tile; tn_ring: two K sub-steps, and two slots
    because BJ = 256, so wg_div = 1) -> dict(M, bmk: rows per reduction step, splits, rows_per_split, slab_bytes)"""
    ho, wo = out_hw(h, w)
    m = b * ho * wo
    bmk = 4 * 2 * CE[dtype]
    wgs = 512 * (128 * 128) // (64 * 256)
    want = wgs                                                   # (one tile: wgs / tiles)
    want = max(1, min(want, max(1, m // (16 * bmk))))
    rps = (m + want - 1) // want
    rps = (rps + bmk - 1) // bmk * bmk
    splits = (m + rps - 1) // rps
    return dict(M=m, bmk=bmk, splits=splits, rows_per_split=rps, slab_bytes=splits * 64 * 256 * 4)


def stem_case(dtype, shape):
    """-> dict(img [B, 3, H, W] fp32, w [64, 3, 7, 7] fp32 (the master), scale, bias [64] fp32, dy [B, Ho, Wo, 64] in dtype).  Every
    fifth scale is negative; bias has mixed signs at the scale of the conv's output, so about half of the affine outputs sit at the
    ReLU's zero."""
    b, h, w = shape
    ho, wo = out_hw(h, w)
    g = _seed(b, h, w, DTYPES.index(dtype), 31)
    scale = 0.5 + torch.rand(64, generator=g)
    scale[::5] *= -1
    return dict(img=torch.randn(b, 3, h, w, generator=g), w=torch.randn(64, 3, 7, 7, generator=g) / 12.0, scale=scale,
                bias=torch.randn(64, generator=g) * 0.7, dy=torch.randn(b, ho, wo, 64, generator=g).to(dtype))


STEM_REFUSED = [(1, 9, 8), (1, 8, 9), (1, 6, 8), (1, 8, 6), (0, 8, 8), (-1, 8, 8)]      # odd H / W, H / W below 7, B <= 0


# ------------------------------------------------------------------ rpe_stage_image_nhwc4
IMAGE_SHAPES = [(1, 2, 2), (3, 6, 10), (2, 33, 17), (1, 64, 48)]     # odd dims are legal here

# +-0, NaN, +-inf, fp32 subnormals, round-to-nearest-even ties of bf16 (8 significant bits) and fp16 (11), both directions, values
# beyond fp16's range (and one at the edge of bf16's), fp16 subnormal ties
SPECIALS = [0.0, -0.0, NAN, INF, -INF, 2.0 ** -149, -(2.0 ** -140), 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -11,
            1.0 + 3 * 2.0 ** -11, -(1.0 + 3 * 2.0 ** -11), 70000.0, -65520.0, 65519.996, 3.0e38, -3.4e38, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24 + 2.0 ** -30]


def image_case(shape):
    """[B, 3, H, W] fp32: randn with the SPECIALS planted over the first elements of each channel plane in turn (all of them wherever
    the image has room; the 2 x 2 image carries the first twelve)"""
    b, h, w = shape
    x = torch.randn(b, 3, h, w, generator=_seed(b, h, w, 37))
    flat = x.view(-1)
    n = min(len(SPECIALS), flat.numel())
    step = max(1, flat.numel() // n) if flat.numel() > 2 * n else 1
    flat[torch.arange(n) * step] = torch.tensor(SPECIALS[:n], dtype=torch.float32)
    return x


# ------------------------------------------------------------------ rpe_stage_frames_u8
FRAME_GEOMS = [(1, 8, 8, 8, 8), (2, 12, 16, 8, 10), (3, 17, 21, 8, 10), (1, 16, 48, 16, 16)]    # (B, Hs, Ws, H, W); the third has odd differences
ALL_BYTES = (1, 16, 48, 16, 16)             # the cropped window (16 x 16 at column 16) holds all 256 byte values in each channel


def frames_case(geom):
    """uint8 [B, Hs, Ws, 3]"""
    b, hs, ws, h, w = geom
    fr = torch.randint(0, 256, (b, hs, ws, 3), generator=_seed(b, hs, ws, h, w, 41), dtype=torch.uint8)
    if geom == ALL_BYTES:
        v = torch.arange(256, dtype=torch.int64).view(16, 16)
        left = (ws - w) // 2
        for c in range(3):
            fr[0, :, left:left + w, c] = ((v * (2 * c + 1) + 85 * c) % 256).to(torch.uint8)     # a different permutation per channel
    return fr


# ------------------------------------------------------------------ rpe_stage_frames_u8_resized
# (name, B, Hs, Ws, Hr, Wr, H, W, [(top, left)]): both passes up (top / left 0, the largest legal, an odd middle value) and down (ksize 5),
# each pass alone, and the pure window -- odd offsets, and below it the geometries the engine sends for odd crop differences
RESIZE_CASES = [
    ("both up", 2, 12, 20, 16, 26, 8, 10, [(0, 0), (8, 16), (3, 5)]),
    ("both down", 2, 40, 24, 26, 16, 8, 10, [(9, 3)]),
    ("horizontal only", 2, 12, 20, 12, 14, 8, 10, [(1, 3)]),
    ("vertical only", 2, 20, 12, 14, 12, 8, 10, [(3, 1)]),
    ("window", 2, 13, 17, 13, 17, 8, 10, [(1, 3), (5, 7), (0, 0)]),
]
# (Hs, Ws, H, W) with an odd difference and no resize (the frame's shorter side is the resize target): what engine.py routes to the window
# form, at crop_origin's offsets.  (Hs - H) / 2 is 2.5 and 3.5 (ties to 2 and 4), 0.5 (to 0) and 1.5 (to 2)
ODD_CROPS = [(13, 20, 8, 10), (15, 17, 8, 10), (9, 13, 8, 10), (16, 13, 8, 10)]


def resize_frames(b, hs, ws):
    """uint8 [B, Hs, Ws, 3]: the two frames differ (a per-image stride error in the intermediate shows); smooth ramps plus noise, so that
    neighbouring resampled pixels differ and intermediate values land on .5 often enough for the 8-bit rounding to matter"""
    g = _seed(b, hs, ws, 43)
    yy, xx = torch.meshgrid(torch.arange(hs), torch.arange(ws), indexing="ij")
    fr = torch.empty(b, hs, ws, 3, dtype=torch.uint8)
    for i in range(b):
        for c in range(3):
            ramp = (yy * (7 + 3 * c + i) + xx * (5 + 2 * i + c)) % 256
            fr[i, :, :, c] = ((ramp + torch.randint(0, 64, (hs, ws), generator=g)) % 256).to(torch.uint8)
    return fr


# ------------------------------------------------------------------ rpe_pack_conv_weights_multi
CHUNK = 4096
# (Co, RS, Ci, scale, wf, wd)
PACK_TABLE = [(64, 1, 64, False, True, True), (128, 9, 64, False, True, True), (48, 9, 24, False, True, True), (64, 1, 128, True, True, True),
              (64, 9, 64, False, False, True), (256, 1, 64, True, True, False)]
PACK_TABLE_TILED = [t for t in PACK_TABLE if t[0] % 64 == 0 and t[2] % 64 == 0]


def pack_starts(table):
    s, out = 0, []
    for co, rs, ci, _, _, _ in table:
        out.append(s)
        s += co * rs * ci
    return out, s


def pack_paths(table):
    """pack_conv_weights_multi_kernel's decision per 4096-element chunk -> [dict(base, layer: of its first element, tiled, straddles:
    the chunk's elements belong to more than one layer)]"""
    starts, total = pack_starts(table)
    ends = starts[1:] + [total]
    out = []
    for base in range(0, total, CHUNK):
        l = max(i for i, s in enumerate(starts) if s <= base)
        co, _, ci = table[l][:3]
        tiled = co % 64 == 0 and ci % 64 == 0 and starts[l] % CHUNK == 0 and ends[l] >= base + CHUNK
        out.append(dict(base=base, layer=l, tiled=tiled, straddles=min(base + CHUNK, total) > ends[l]))
    return out


def pack_case(table):
    """-> [dict(src [Co, RS, Ci] fp32, scale [Co] fp32 or None)]"""
    out = []
    for i, (co, rs, ci, sc, _, _) in enumerate(table):
        g = _seed(co, rs, ci, i, 47)
        s = None
        if sc:
            s = 0.5 + torch.rand(co, generator=g)
            s[::3] *= -1.7
        out.append(dict(src=torch.randn(co, rs, ci, generator=g) / math.sqrt(rs * ci), scale=s))
    return out


# ------------------------------------------------------------------ small fp32 utilities
TRANSPOSE_CASES = [(1, 1, 1, 1), (37, 50, 50, 40), (33, 31, 40, 64), (64, 64, 64, 64)]          # (rows, cols, ldi, ldo)
COLSUM_CASES = [(r, c, ld) for r in (1, 5, 8, 300) for c, ld in ((1, 1), (32, 32), (70, 70), (1, 3), (32, 40), (70, 77))]
COPY2D_CASES = [(1, 1, 3, 2), (300, 70, 75, 80), (7, 33, 40, 33)]                               # (rows, cols, ld_src, ld_dst)
RELU_OUT = [0.0, -0.0, 2.0 ** -149, 1e-30, -1.0, -(2.0 ** -149), NAN, INF, -INF, 3.5]


def colsum_case(rows, cols, ld):
    """x [rows, ld] (the columns past cols are never read: NaN), old [cols]; the values have a mean, so the sums grow with the rows"""
    g = _seed(rows, cols, ld, 53)
    x = torch.randn(rows, ld, generator=g) + 0.5
    x[:, cols:] = NAN
    return x, torch.randn(cols, generator=g) * 3.0
