"""Inputs of the element-wise tests of the fused BN-backward epilogue of the conv data gradient (rpe_conv2d_dgrad_bn, bn_mode 1 .. 5 of
nt_kernel, csrc/igemm_impl.h), shared by the CPU self-test (tests/test_dgrad_bn_cpu.py) and the GPU test (tests/test_gpu_dgrad_bn.py), so
that the bounds of tests/_dgrad_bn_bounds.py are judged on the very inputs the kernel is held to.  CPU tensors in the compute type.

A case is a conv shape (b, h, w, in_c, out_c, k, stride, pad) and a dtype; the producing layer (y -> BatchNorm (+ residual) -> ReLU, whose
output is this conv's input and whose gate and statistics the epilogue uses) and the conv's operands are drawn once per case, and every
mode runs on them: that is what lets modes 1, 2 and 4 be compared bit for bit.

Each shape is the smallest that reaches the path named beside it (rows = b h w of the data gradient; a partial-sum row covers 128 of
them, a workgroup tile 128 rows by 64 or 128 columns)."""
import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
EPS = 1e-5
STATS_ROWS = 128
BIG_SIGMAS = 8.0                            # the constructed column's mean, in units of sigma
UNDECIDED_CAP = 1e-3                        # share of a case's elements whose mode-2 gate the fp64 reference may leave open

# (path, (b, h, w, in_c, out_c, k, stride, pad))
SHAPES = [
    ("dense", (1, 10, 10, 64, 64, 1, 1, 0)),        # 100 rows: one partial row; nothing may be written for the tile's second 128 rows
    ("dense", (3, 8, 8, 128, 256, 1, 1, 0)),        # 192 rows: one and a half partial rows
    ("dense", (2, 9, 9, 72, 64, 1, 1, 0)),          # in_c a multiple of 8, not of 64: a ragged column tile, mask bytes still whole
    ("dense", (5, 16, 16, 64, 256, 1, 1, 0)),       # 1280 rows: several workgroup tiles
    ("3x3s1", (3, 14, 14, 64, 64, 3, 1, 1)),        # 16-bit: halo form, tiles straddle images, the last one partial; fp32: gathered form
    ("3x3s1", (1, 20, 36, 64, 128, 3, 1, 1)),       # H != W halo
    ("3x3s2 parity", (3, 12, 12, 64, 64, 3, 2, 1)),     # 108 rows per class: 4 partial rows
    ("3x3s2 parity", (5, 12, 12, 64, 128, 3, 2, 1)),    # 180 rows per class: the second row of each class is partial
    ("3x3s2 odd", (2, 15, 15, 64, 64, 3, 2, 1)),        # odd dims: stride 2 without the parity classes
    ("1x1s2 parity", (2, 12, 12, 64, 128, 1, 2, 0)),    # a projection shortcut's shape with the epilogue: classes with no tap at all
]
# in_c not a multiple of 8: the epilogue's scalar tail (load8's element-wise branch).  No conv in the suite runs such a width, and the
# data-gradient entry points refuse it (igemm.hip: "conv outputs need N % 8 == 0"), so the kernel cannot be asked for it: the GPU test
# holds the refusal, the CPU test uses the case to show that the bounds would reject a tail fault.  Modes 1, 2, 3 (a mask byte holds 8).
TAIL_SHAPE = ("dense tail", (2, 9, 9, 68, 64, 1, 1, 0))


def _seed(*v):
    s = 0
    for x in v:
        s = (s * 1000003 + int(x)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def name(dtype):
    return str(dtype)[6:]


def out_hw(shape):
    b, h, w, ci, co, k, s, p = shape
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def is_dense(shape):
    return shape[5:] == (1, 1, 0)


def is_parity(shape):
    return shape[6] == 2 and shape[1] % 2 == 0 and shape[2] % 2 == 0


def is_halo(shape, dtype):
    return dtype != F32 and shape[5:] == (3, 1, 1) and shape[4] % 64 == 0


def parity_rows(shape):
    """partial-sum rows of the parity-class form: every class rounds its b h w / 4 rows up to whole partial rows"""
    b, h, w = shape[:3]
    return 4 * (-(-(b * h * w // 4) // STATS_ROWS))


def variants(shape, dtype):
    """(mode, residual) pairs of a case: modes 1, 2, 3 in every type, the packed mask (4) in the 16-bit types, the y-free form (5) on
    the dense shapes of those; the gates of modes 1 and 4 once from a forward without and once with a residual"""
    v = [(1, False), (1, True), (2, False), (3, False)]
    if dtype != F32 and shape[3] % 8 == 0:
        v += [(4, False), (4, True)]
        if is_dense(shape):
            v += [(5, False), (5, True)]
    return v


def case(shape, dtype):
    """-> dict: y, res, addend [rows, in_c] (addend None in half the cases), dy [b, out_c, ho, wo], w [out_c, in_c, k, k] in dtype;
    mean, invstd, gamma, beta, scale, shift [in_c] fp32; big = the constructed column (mean 8 sigma: y invstd and mean invstd cancel
    in xhat = fma(y, invstd, -mean invstd))"""
    b, h, w, ci, co, k, s, p = shape
    di = DTYPES.index(dtype)
    g = _seed(*shape, di)
    rows = b * h * w
    big = min(ci - 1, 5)
    mu = torch.full((ci,), 0.3)
    mu[big] = BIG_SIGMAS * 1.5
    y = (torch.randn(rows, ci, generator=g) * 1.5 + mu).to(dtype)
    yd = y.double()
    mean = yd.mean(0)
    invstd = (yd.var(0, unbiased=False) + EPS).rsqrt()
    mean, invstd = mean.float(), invstd.float()
    gamma, beta = 0.5 + torch.rand(ci, generator=g), torch.rand(ci, generator=g) - 0.5
    scale = gamma * invstd
    shift = beta - mean * scale
    ho, wo = out_hw(shape)
    res = torch.randn(rows, ci, generator=g).to(dtype)
    dy = torch.randn(b, co, ho, wo, generator=g).to(dtype)
    wt = (torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5).to(dtype)
    addend = torch.randn(rows, ci, generator=g).to(dtype)
    if (sum(shape) + di) % 2:
        addend = None
    return dict(shape=shape, dtype=dtype, rows=rows, y=y, res=res, addend=addend, dy=dy, w=wt, mean=mean, invstd=invstd, gamma=gamma,
                beta=beta, scale=scale, shift=shift, big=big)


def unpack_bits(mask, rows, c):
    """the packed mask [rows C / 8] bytes -> [rows, C] bool: bit j of a byte = channel 8 k + j"""
    sh = torch.arange(8, dtype=torch.uint8, device=mask.device)
    return ((mask.view(rows, c // 8, 1) >> sh) & 1).bool().reshape(rows, c)


def forward(c, residual, ops=None):
    """The producing layer's forward: relu(fma(y, scale, shift) (+ res)) -> dict(a_out [rows, in_c] in dtype, bits [rows, in_c] bool or
    None, mask: the packed bytes on the device, else None).  These are INPUTS of the epilogue (mode 1 reads a_out, modes 4 and 5 the mask): with `ops` (the
    tensors of c on the device) they come from the project's own rpe_bn_apply / rpe_bn_apply_mask, without it from a torch statement.
    Asserts that no positive fp64 pre-activation lies at or under the type's smallest value: a_out > 0 and the mask bit then name the
    same set, which the mode-agreement test relies on."""
    dtype, ci = c["dtype"], c["y"].shape[1]
    res = c["res"] if residual else None
    pre = c["y"].double() * c["scale"].double() + c["shift"].double() + (0.0 if res is None else res.double())
    tiny = 2.0 ** -24 if dtype == F16 else 2.0 ** -126
    assert not bool(((pre > 0) & (pre <= tiny)).any()), "a positive pre-activation under the type's floor: pick another seed"
    packed = dtype != F32 and ci % 8 == 0
    if ops is not None:
        if packed:
            a, mask = ops.bn_apply_mask(c["y"], c["scale"], c["shift"], res)
            return dict(a_out=a, mask=mask, bits=unpack_bits(mask, c["rows"], ci))
        return dict(a_out=ops.bn_apply(c["y"], c["scale"], c["shift"], res, relu=True), mask=None, bits=None)
    t = (c["y"].double() * c["scale"].double() + c["shift"].double()).float()       # fmaf: the product of two fp32 is exact in double
    if res is not None:
        t = t + res.float()
    bits = t > 0
    return dict(a_out=t.clamp_min(0.0).to(dtype), bits=bits if packed else None, mask=None)
