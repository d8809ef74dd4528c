"""Inputs of the element-wise tests of the BatchNorm train-step kernels of csrc/norm.hip (rpe_bn_finalize, rpe_bn_eval_affine,
rpe_bn_apply / _mask / _res_bn, rpe_bn_backward / _reduce / _from_dz / _coeffs / _coeffs_t / _apply_dz), shared by the CPU self-test
(tests/test_norm_cpu.py) and the GPU test (tests/test_gpu_norm.py), so that the bounds of tests/_norm_bounds.py are judged on the very
inputs the kernels are held to.  CPU tensors, rows x channels with the channels contiguous, in the compute type.

The launchers' own arithmetic is restated here (reduce_slices, bn_bwd_launch, the spans of the streaming kernels): the bounds take the
rows per block from it, the restatements of the self-test their association, and each shape below is the smallest that reaches the
code path named beside it."""
import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
CE = {F32: 4, BF16: 8, F16: 8}              # elements of a 16-byte chunk
EPS = 1e-5
UNR = 4                                     # the streaming kernels' unroll (ew_cfg) where C / CE is a power of two, else 1


def _seed(*v):
    s = 0
    for x in v:
        s = (s * 1000003 + int(x)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _pow2(v):
    return v > 0 and v & (v - 1) == 0


# ------------------------------------------------------------------ launcher arithmetic
def reduce_slices(tiles, c):
    """NS of reduce_finalize: min(ceil(512 / ceil(C / 32)), 64, tiles / 8), at least 1"""
    cb = (c + 31) // 32
    return max(1, min((512 + cb - 1) // cb, 64, tiles // 8))


def bwd_geometry(m, c, dtype):
    """bn_bwd_launch -> dict(sw, slabs, rpi, nb, rpb), or None where the launcher refuses C: C / CE must divide 256 or be a multiple
    of 256 (whole column slabs)"""
    ce = CE[dtype]
    if c % ce:
        return None
    sw = min(c, 256 * ce)
    if 256 % (sw // ce) or c % sw:
        return None
    rpi = 256 // (sw // ce)
    nb = max(1, min(1024, (m + rpi * 8 - 1) // (rpi * 8)))
    rpb = (m + nb - 1) // nb
    nb = (m + rpb - 1) // rpb
    return dict(sw=sw, slabs=c // sw, rpi=rpi, nb=nb, rpb=rpb)


def stream_geometry(rows, c, dtype):
    """bn_apply_kernel / bn_bwd_apply_dz_kernel -> dict(cpr, unr, sub, span, n): a block owns `span` = 256 sub unr consecutive chunks"""
    cpr = c // CE[dtype]
    unr = UNR if _pow2(cpr) else 1
    sub = cpr // 256 if cpr > 256 else 1
    return dict(cpr=cpr, unr=unr, sub=sub, span=256 * sub * unr, n=rows * cpr)


# ------------------------------------------------------------------ reduce + finalize (rpe_bn_finalize), fp32 only
FIN_SHAPES = [(1, 64), (7, 40), (16, 64), (37, 96), (2053, 64), (70, 2048), (9, 4096)]      # (tiles, C): see the issue's table
FIN_KINDS = ("zero-mean", "mean 20 sigma", "constant channels", "count 1")
FIN_ROWS = 4                                # rows behind each tile's partial sums (the sums are the kernel's INPUT: any count will do)
FIN_REFUSED_C = 4128
MOMENTA = (0.1, 0.37)
N_CONST = 8                                 # `constant channels`: the first 8 channels hold one value each


def fin_kinds(tiles):
    return FIN_KINDS if tiles == 1 else FIN_KINDS[:3]


def fin_case(tiles, c, kind):
    """-> dict(part [tiles, 2, C] fp32 (sum, sum of squares per tile), count, gamma, beta, rm, rv [C]).
    constant channels: x = v_c in every row, |v_c| in 10 .. 50, so that sumsq / count - mean^2 is rounding noise of either sign
    around 0, of size u32 v^2 ~ 5e-5 > eps: without the clamp the variance plus eps goes negative in some channel."""
    g = _seed(tiles, c, FIN_KINDS.index(kind))
    rows = 1 if kind == "count 1" else FIN_ROWS
    sigma = 0.5 + torch.rand(c, generator=g) * 2
    x = torch.randn(tiles, rows, c, generator=g) * sigma
    if kind == "mean 20 sigma":
        x = x + 20.0 * sigma * torch.sign(torch.randn(c, generator=g))
    if kind == "constant channels":
        x[:, :, :N_CONST] = (10.0 + 40.0 * torch.rand(N_CONST, generator=g)) * torch.tensor([1.0, -1.0] * (N_CONST // 2))
    xd = x.double()
    part = torch.stack([xd.sum(1), (xd * xd).sum(1)], 1).float().contiguous()
    return dict(part=part, count=tiles * rows, gamma=0.5 + torch.rand(c, generator=g), beta=torch.rand(c, generator=g) - 0.5,
                rm=torch.randn(c, generator=g), rv=0.5 + torch.rand(c, generator=g))


# ------------------------------------------------------------------ eval affine
EVAL_C = [1, 40, 257, 2048]                 # one lane; C not a multiple of 32; one lane into the second block; many blocks


def eval_case(c):
    g = _seed(c, 77)
    rv = torch.rand(c, generator=g) * 2
    rv[0] = 0.0                             # a channel that never varied: scale = gamma / sqrt(eps)
    return dict(gamma=0.5 + torch.rand(c, generator=g), beta=torch.rand(c, generator=g) - 0.5, rm=torch.randn(c, generator=g) * 3, rv=rv)


# ------------------------------------------------------------------ apply
def apply_shapes(dtype):
    """(rows, C): see the issue's table"""
    return [(1, 64), (515, 64), (43, 192), (3, 2304), (5, 2048) if dtype == F32 else (5, 4096), (9, CE[dtype])]


APPLY_MODES = ("none", "res", "res_bn")
GUARD = 64                                  # sentinel elements behind `out` / bytes behind the mask


def apply_case(dtype, rows, c):
    """-> dict(y, res [rows, C] in dtype, scale, shift, res_scale, res_shift [C], zeros: [(row, channel)] of constructed exact zeros
    (y = 0, res = 0 there and shift = res_shift = 0 in that channel: the pre-activation is +0, the mask bit 0 and the output +0)"""
    g = _seed(rows, c, DTYPES.index(dtype), 3)
    y = (torch.randn(rows, c, generator=g) * 1.5 + 0.2).to(dtype)
    res = torch.randn(rows, c, generator=g).to(dtype)
    scale, shift = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    rsc, rsh = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    scale[::5] *= -1                        # negative gammas happen
    zc = c - 1                              # the last channel of the last chunk
    shift[zc], rsh[zc] = 0.0, 0.0
    zeros = sorted({(0, zc), (rows - 1, zc)})
    for (r, ch) in zeros:
        y[r, ch], res[r, ch] = 0.0, 0.0
    # one tiny positive pre-activation, 2^-26: the mask bit is 1 (taken from the fp32 value) while an fp16 output rounds to +0
    shift[zc - 1], rsh[zc - 1], scale[zc - 1] = 0.0, 0.0, 0.25
    y[0, zc - 1], res[0, zc - 1] = 2.0 ** -24, 0.0
    return dict(y=y, res=res, scale=scale, shift=shift, res_scale=rsc, res_shift=rsh, zeros=zeros)


# ------------------------------------------------------------------ backward
BWD_SHAPES = [(1, 64), (5, 64), (601, 64), (147, 256), (3001, 128), (27, 2048), (27, 4096)]      # (M, C): see the issue's table
BWD_DZ_EXTRA = [(43, 192)]                  # _from_dz / _apply_dz: chunks per row not a power of two
MEAN_KINDS = (0.2, 30.0)                    # |mean| in units of sigma
# refused or right: (dtype, C) that bn_bwd_launch must compute in every channel or refuse with the shape error
BWD_ODD_C = [(BF16, 192), (F16, 192), (F32, 1536), (F32, 2304), (BF16, 3072)]
BWD_ODD_M = 27
STATS_ROWS = 128                            # rows per tile of the fused epilogue's partial sums (rpe_conv_stats_tiles)


def bwd_case(dtype, m, c, mean_sigmas):
    """-> dict(dA, a_out, y [M, C] in dtype, mean, invstd, gamma [C], c1c2 [2, C]): y = sigma (mean_sigmas s + n), a_out about half
    zeros (and a few negative zeros and negatives: no gradient there either), c1c2 arbitrary coefficients for rpe_bn_backward_apply_dz"""
    g = _seed(m, c, DTYPES.index(dtype), int(mean_sigmas * 10))
    sigma = 0.5 + torch.rand(c, generator=g) * 1.5
    mu = mean_sigmas * sigma * torch.sign(torch.randn(c, generator=g))
    y = (torch.randn(m, c, generator=g) * sigma + mu).to(dtype)
    a = torch.randn(m, c, generator=g).clamp_min(0)
    a[torch.rand(m, c, generator=g) < 0.02] = -0.0
    a[torch.rand(m, c, generator=g) < 0.02] = -1.0
    gamma = 0.5 + torch.rand(c, generator=g)
    gamma[::7] *= -1
    return dict(dA=torch.randn(m, c, generator=g).to(dtype), a_out=a.to(dtype), y=y, mean=mu + 0.01 * sigma * torch.randn(c, generator=g),
                invstd=1.0 / sigma, gamma=gamma, c1c2=torch.randn(2, c, generator=g) * 0.1)


def dz_of(case, use_a):
    """dz = dA where a_out > 0, +0 elsewhere -- exact, in the compute type"""
    if not use_a:
        return case["dA"]
    return torch.where(case["a_out"] > 0, case["dA"], torch.zeros_like(case["dA"]))


def stats_part(dz, case, rows=STATS_ROWS):
    """the fused data-gradient epilogue's partial sums [tiles, 2, C] fp32 of dz and dz xhat per tile of `rows` rows (inputs of
    rpe_bn_backward_from_dz / _coeffs: formed in fp64 and rounded once, how they were summed is not under test here)"""
    m, c = dz.shape
    tiles = (m + rows - 1) // rows
    d = torch.zeros(tiles * rows, c, dtype=torch.float64)
    d[:m] = dz.double()
    x = torch.zeros_like(d)
    x[:m] = (case["y"].double() - case["mean"].double()) * case["invstd"].double()
    return torch.stack([d.view(tiles, rows, c).sum(1), (d * x).view(tiles, rows, c).sum(1)], 1).float().contiguous()


COEFFS_T = [(3, 40, 72), (16, 256, 64), (9, 64, 1), (20, 2048, 512)]      # (tiles, C, Ci)


def coeffs_t_case(dtype, tiles, c, ci, mean_sigmas):
    """-> dict(part [tiles, 2, C] fp32 with NaN in the second half of every row (never read), t [C, Ci] fp32, w [C, Ci] in dtype,
    mean, invstd [C], rows)"""
    g = _seed(tiles, c, ci, DTYPES.index(dtype), int(mean_sigmas * 10))
    part = torch.randn(tiles, 2, c, generator=g) * 8
    part[:, 1] = float("nan")
    sigma = 0.5 + torch.rand(c, generator=g) * 1.5
    return dict(part=part.contiguous(), t=torch.randn(c, ci, generator=g) * 4, w=(torch.randn(c, ci, generator=g) * 0.2).to(dtype),
                mean=mean_sigmas * sigma * torch.sign(torch.randn(c, generator=g)), invstd=1.0 / sigma, rows=tiles * STATS_ROWS)
