"""Inputs of the gradient-clipping / AdamW tests, shared by the CPU self-tests (tests/test_clip_cpu.py: the correct fp32 statement
stays at <= 0.5 of every bound of tests/_clip_bounds.py, mutants are rejected) and the GPU tests (tests/test_gpu_clip.py).  CPU fp32
tensors, drawn like tests/_scalar_cases.py: adam_case."""
import torch

CLIP_NS = [1, 2, 3, 4, 5, 1023, 1024, 1025, 10007]     # the 4-wide body and its 1-3 element tail; more than one block / partial row
GPU_NS = [1, 3, 4, 5, 1023, 1024, 1025]                # the sizes of the operator-level GPU tests (plus full_pass_n and SPLIT)
SPLIT = (7, 1021, 33)                                  # a 3-segment split with odd lengths (each start padded to 16 bytes)
STEPS = [1, 2, 10, 1000]
WDS = (0.0, 1e-2, 0.1)
MAX_NORMS = (1e-3, 1.0, 1e30)                          # clips everything of unit scale; clips n > 1; never clips
HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
# gradient scale per kind.  unit: N(0,1); tiny: sqrt(v) comparable with eps, the norm comparable with clip_grad_norm_'s 1e-6; small20 /
# huge: the squares leave fp32's range (1e-40, 1e40) on both sides; zero: norm 0, coefficient exactly 1
SCALE = {"unit": 1.0, "tiny": 1e-6, "small20": 1e-20, "huge": 1e20, "zero": 0.0}
KINDS = tuple(SCALE)
NONFINITE = {"inf": float("inf"), "nan": float("nan")}   # unit gradients with ONE such element (operator level only)


def max_norms(kind):
    """huge gradients only with max_norm <= 1: the clipped gradient is then of unit scale or below, like its moments"""
    return tuple(x for x in MAX_NORMS if x <= 1.0) if kind == "huge" else MAX_NORMS


def clip_case(n, step, kind):
    """-> p, g, m, v as _scalar_cases.adam_case draws them: every other p exactly 0, m and v random and non-zero at the gradient's
    scale (v at 1e-3 .. 1 of its square) -- except for `huge`, whose moments stay at unit scale: what reaches them is the CLIPPED
    gradient."""
    gen = torch.Generator().manual_seed(7919 * KINDS.index(kind) + 31 * n + step)
    s = SCALE[kind]
    ms = 1.0 if kind == "huge" else s
    p = torch.randn(n, generator=gen)
    p[::2] = 0.0
    g = torch.randn(n, generator=gen) * s
    m = torch.randn(n, generator=gen) * (0.5 * ms)
    v = torch.rand(n, generator=gen) * (ms * ms) * 10.0 ** -((3 - torch.arange(n)) % 4).float()
    return p, g, m, v


def grad_case(n, kind, seed=0):
    """one gradient segment of n elements; kinds of SCALE, or `inf` / `nan`: unit with one non-finite element in the middle"""
    gen = torch.Generator().manual_seed(104729 * (list(KINDS) + list(NONFINITE)).index(kind) + 17 * n + seed)
    g = torch.randn(n, generator=gen) * SCALE.get(kind, 1.0)
    if kind in NONFINITE:
        g[n // 2] = NONFINITE[kind]
    return g


def full_pass_n(rows_fn):
    """5 elements more than one full pass of the sum-of-squares grid at its cap, from the exported row-count function alone: the
    cap is its value for a huge n, the elements one block takes per trip the largest n that still gets one row.  The first blocks
    then take a second trip and the 1-element tail is live."""
    cap = rows_fn(1 << 40)
    lo, hi = 1, 1 << 30          # rows_fn(lo) == 1 < rows_fn(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if rows_fn(mid) == 1 else (lo, mid)
    assert rows_fn(cap * lo) == cap and rows_fn(cap * lo - lo) == cap - 1, "the row count is not ceil(n / per-block elements), capped"
    return cap * lo + 5
