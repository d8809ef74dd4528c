"""Inputs of the element-wise tests of the head kernels of csrc/heads.hip (aux head, any-channel aux head, depth heads, tensor_add),
shared by the CPU self-test (tests/test_heads_cpu.py: a correct fp32 statement stays at <= 0.5 of every bound, mutants are rejected)
and the GPU tests (tests/test_gpu_heads.py), so that the bounds of tests/_head_bounds.py are judged on the very inputs the kernels are
held to.  CPU tensors; features are NHWC in the compute type."""
import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
CE = {F32: 4, BF16: 8, F16: 8}              # elements of a 16-byte chunk
KINDS = ("relu", "signed")                  # clamp_min(0) features (many exact zeros) / signed features
CONSTRUCTS = (None, "zero", "tie", "nan")   # a constructed window at the first and the last window of the tensor

# ------------------------------------------------------------------ aux head, C = 64 (rpe_aux_head_fwd / _bwd / _bwd_det, fused stem aux)
AUX_SHAPES = [(1, 2, 2), (3, 6, 10), (2, 16, 16)]     # one window, most lanes idle; a partial block; whole blocks
# forward only: more than 4096 blocks' worth of windows (16 per block in fp32, 32 in 16-bit), so the grid takes a second trip
AUX_BIG = {F32: (17, 128, 128), BF16: (33, 128, 128), F16: (33, 128, 128)}

# ------------------------------------------------------------------ aux head, any C (rpe_aux_head_fwd_c / _bwd_c)
AUXC_C = {F32: [4, 64, 256, 1024], BF16: [8, 64, 256, 512, 1024], F16: [8, 64, 256, 512, 1024]}
AUXC_HW = [(2, 2), (7, 5), (14, 14)]        # (7, 5): the last row and column belong to no window
AUXC_B = [1, 3]
AUXC_BIG = (F32, 256, (5, 116, 116))        # forward only: 16 820 windows at 64 lanes each, 4 per block: more than 4096 blocks


def ew_grid(n, per_block=256):
    """the launch grid of the element-wise kernels (csrc/heads.hip: ew_grid)"""
    return max(1, min(4096, (n + per_block - 1) // per_block))


def windows(h, w):
    return (h // 2) * (w // 2)


def aux_case(dtype, b, h, w, c, kind, use_depth, construct=None):
    """-> dict(x [b, h, w, c] in dtype, w [c], bias [1], depth_feat [b, Ho Wo] or None, dout [b, Ho Wo], slots [(image, oh, ow)]).
    construct places one window at the first and at the last window of the tensor:
      zero: all four pixels zero -- every tap equals the bias, tap 0 must win;
      tie : taps 1 and 3 hold the same pixel sign(w) u, u in [1, 3) (so sum |w| u + bias, products that round), taps 0 and 2 are zero:
            tap 1 must win -- also a kernel that forms the two taps' dot products differently (one fused, one not) is caught;
      nan : one NaN in tap 2 (channel 0) -- raw and out are NaN there and idx == 2, every other window unaffected."""
    g = torch.Generator().manual_seed(7919 * c + 131 * h + 17 * w + 5 * b + 2 * KINDS.index(kind) + int(use_depth) + 100003 * DTYPES.index(dtype))
    x = torch.randn(b, h, w, c, generator=g)
    if kind == "relu":
        x = x.clamp_min(0)
    x = x.to(dtype)
    wt = torch.randn(c, generator=g) * 0.2
    bias = torch.tensor([0.1])
    ho, wo = h // 2, w // 2
    df = torch.randn(b, ho * wo, generator=g) if use_depth else None
    dout = torch.randn(b, ho * wo, generator=g)
    slots = []
    if construct is not None:
        slots = sorted({(0, 0, 0), (b - 1, ho - 1, wo - 1)})
        for (i, oh, ow) in slots:
            px = x[i, 2 * oh:2 * oh + 2, 2 * ow:2 * ow + 2]          # a view: [2, 2, c]
            if construct == "zero":
                px.zero_()
            elif construct == "tie":
                px.zero_()
                px[0, 1] = px[1, 1] = (torch.sign(wt) * (1.0 + 2.0 * torch.rand(c, generator=g))).to(dtype)
            elif construct == "nan":
                px[1, 0, 0] = float("nan")
    return dict(x=x, w=wt, bias=bias, depth_feat=df, dout=dout, slots=slots)


def stem_case(dtype, b, h, w, kind, use_depth):
    """The fused stem pass and the det_y backward: the raw conv output y [b, h, w, 64] in dtype with bn1's scale / shift [64], and an aux
    head behind the activation.  `relu`: shifts around zero (half of the activations are exact zeros); `signed` has no meaning here (the
    activation is a ReLU), it draws large positive shifts instead: hardly any zero."""
    case = aux_case(dtype, b, h, w, 64, "signed", use_depth)
    g = torch.Generator().manual_seed(31 * h + w + b)
    case["scale"] = torch.rand(64, generator=g) + 0.5
    case["shift"] = torch.randn(64, generator=g) * 0.3 + (0.0 if kind == "relu" else 1.5)
    return case


# ------------------------------------------------------------------ depth heads
DEPTH_HW = [(4, 4), (8, 12), (64, 64), (224, 224)]                           # rpe_depth_head_fwd (two pooling steps, multiples of 4)
DEPTH_B = [1, 3]
# rpe_depth_head_fwd_pools: (H, W, pools).  (13, 22): H >> pools drops a remainder at 1, 2 and 3; (64, 64, 6): one output pixel, a
# 4096-term window, var = 0; (224, 224, 1): 12 544 outputs, the largest shared-memory use the models reach
DEPTH_POOLS = [(13, 22, 1), (13, 22, 2), (13, 22, 3), (64, 64, 6), (224, 224, 1), (8, 12, 2)]
DEPTH_KINDS = ("uniform", "offset", "const")    # U[0, 1]; 2.5 + 0.05 N(0, 1) (ill-conditioned for (float)mean); a constant image
DEPTH_W, DEPTH_BIAS = 1.1, -0.2
DEPTH_CONST = 0.75


def depth_case(b, h, w, kind):
    g = torch.Generator().manual_seed(1009 * h + 13 * w + b + 7 * DEPTH_KINDS.index(kind))
    if kind == "uniform":
        d = torch.rand(b, h, w, generator=g)
    elif kind == "offset":
        d = 2.5 + 0.05 * torch.randn(b, h, w, generator=g)
    else:
        d = torch.full((b, h, w), DEPTH_CONST)
    return dict(depth=d, w=torch.tensor([DEPTH_W]), b=torch.tensor([DEPTH_BIAS]))


DEPTH_BWD_NS = [1, 255, 4097, 70001]
DEPTH_BWD_START = (0.75, -1.25)                 # dw and db accumulate onto these


def depth_bwd_blocks(n):
    return ew_grid(n, 256 * 16)


def depth_bwd_case(n):
    g = torch.Generator().manual_seed(50 + n)
    return dict(d_feat=torch.randn(n, generator=g), xhat=torch.randn(n, generator=g))


# ------------------------------------------------------------------ tensor_add
def tensor_add_ns(dtype):
    ce = CE[dtype]
    return [ce, 255 * ce, (2 ** 20 + 257) * ce]      # one chunk; a partial block; past 4096 x 256 chunks: a second grid-stride trip


def tensor_add_case(dtype, n, guard):
    """dst, src [n + guard] in dtype; magnitudes spread over many binades so that the sum's rounding matters"""
    g = torch.Generator().manual_seed(n % 100003 + DTYPES.index(dtype))
    mk = lambda: (torch.randn(n + guard, generator=g) * torch.exp2(torch.randint(-6, 7, (n + guard,), generator=g).float())).to(dtype)
    return mk(), mk()
