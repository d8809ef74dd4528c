"""Inputs of the element-wise tests of the fp32 scalar kernels (LSTM cell, pose loss, Adam, loss scaler), shared by the CPU self-tests
(tests/test_bounds_cpu.py: a correct fp32 statement stays at <= 0.5 of the bound, mutants are rejected) and the GPU tests
(tests/test_gpu_ops.py), so that TR and EW of tests/_bounds.py are fixed on the very inputs the kernels are held to.  CPU fp32 tensors.

The element-wise kernels take a second grid-stride trip only from 2^28 elements on (ew_grid in csrc/heads.hip caps the grid at
4096 blocks of 256 threads); that trip stays untested here: nothing of that size is allocated."""
import numpy as np
import torch

from oracle import pose_oracle as po

# ------------------------------------------------------------------ LSTM cell
# an odd Hd, totals that are no multiple of 256, more than one block
LSTM_SHAPES = [(1, 1), (5, 16), (3, 7), (2, 50), (33, 64), (257, 3)]
LSTM_KINDS = ("unit", "wide", "saturated")      # N(0,1); N(0,1) * 8 (tails to |x| ~ 30); N(0,1) with row 0 at +-90
SAT = 90.0


def lstm_case(n, hd, kind, with_prev):
    """-> dict(gates [n, 4 hd] pre-activations, b_ih, b_hh [4 hd], c_prev [n, hd] or None, dh, dc_in [n, hd])"""
    g = torch.Generator().manual_seed(1000 * n + 10 * hd + 2 * LSTM_KINDS.index(kind) + int(with_prev))
    gates = torch.randn(n, 4 * hd, generator=g) * (8.0 if kind == "wide" else 1.0)
    if kind == "saturated":
        j = torch.arange(4 * hd)
        gates[0] = torch.where((j // hd + j % hd) % 2 == 0, SAT, -SAT)      # every gate block sees both signs (Hd = 1: i +, f -, g +, o -)
    b_ih, b_hh = torch.randn(4 * hd, generator=g) * 0.1, torch.randn(4 * hd, generator=g) * 0.1
    c_prev = torch.randn(n, hd, generator=g)
    return dict(gates=gates, b_ih=b_ih, b_hh=b_hh, c_prev=c_prev if with_prev else None, dh=torch.randn(n, hd, generator=g),
                dc_in=torch.randn(n, hd, generator=g))


# ------------------------------------------------------------------ pose loss
POSE_NS = [1, 2, 255, 256, 257, 1000]       # one 256-thread block that strides: 257 and 1000 take a second and a partial last trip
POSE_METRICS = (0, 1, 2, 3)                 # l2, l1, linf, combined
POSE_MODES = (0, 1)                         # position, pose
POSE_SCALES = ((1.0, 1.0), (2.5, 0.5))      # (scale, alpha)
POSE_EPS = 1e-4
_T = (0.25, -0.125, 1.0, 0.5, -0.5, 0.5, 0.5)     # truth of the exact rows: |q| = 1 exactly
# exact rows (all values fp32-exact; prediction = truth position + d, quaternion q):
POSE_EXACT = [
    ((0.0, 0.0, 0.0), (0.5, -0.5, 0.5, 0.5)),             # d = 0: sign 0, l2 gradient 0 / sqrt(eps); qhat . t = +1
    ((0.5, -0.5, 0.25), (-1.0, 1.0, -1.0, -1.0)),         # tie |d0| = |d1| > |d2|; qhat . t = -1, |q| = 2, the clamp active
    ((0.125, 0.5, -0.5), (0.5, 0.5, -0.5, 0.0)),          # tie |d1| = |d2| > |d0|; qhat_w = 0 exactly: the clamp passes the gradient
    ((-0.375, 0.0625, 0.75), (5e-4, 5e-4, -5e-4, 5e-4)),  # |q| = 1e-3
    ((0.0, 0.25, -0.25), (500.0, 500.0, 500.0, -500.0)),  # one zero component, a tie behind it; |q| = 1e3, qhat_w < 0
]
POSE_ROTS = range(len(POSE_EXACT))


def pose_slots(n):
    return sorted({i for i in (0, 255, 256, n - 1) if i < n})


def pose_rows(n, rot):
    """Seeded rows as tools/gen_pose_errors_golden.py draws them (truth a random pose, prediction another random pose + 0.3 noise),
    with exact row (k + rot) mod 5 at the k-th of the indices 0, 255, 256, n - 1: over rot = 0..4 every exact row visits every index."""
    g = torch.Generator().manual_seed(77 + n)
    truth = po._rand_pose((n,), g)
    pred = po._rand_pose((n,), g) + 0.3 * torch.randn(n, 7, generator=torch.Generator().manual_seed(1 + n))
    for k, i in enumerate(pose_slots(n)):
        d, q = POSE_EXACT[(k + rot) % len(POSE_EXACT)]
        truth[i] = torch.tensor(_T)
        pred[i] = torch.tensor([_T[0] + d[0], _T[1] + d[1], _T[2] + d[2]] + list(q))
    return pred.contiguous(), truth.contiguous()


# ------------------------------------------------------------------ Adam
ADAM_NS = [1, 2, 3, 4, 5, 1023, 1024, 1025, 10007]      # the 4-wide body and its 1-3 element tail; more than one block
ADAM_STEPS = [1, 2, 10, 1000, 100000]                   # bc1 / bc2 from 0.1 / 0.001 to 1
ADAM_KINDS = ("unit", "tiny", "zero")                   # g ~ N(0,1); 1e-6 N(0,1) (sqrt(v) comparable with eps); exact 0 with m = v = 0
ADAM_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def adam_case(n, step, kind):
    """-> p, g, m, v.  Every other p is exactly 0 (the stored value is then the update itself, not swamped by ulp(p)); m and v start
    random and non-zero, v >= 0 at 1e-3 .. 1 of the gradient's square, element by element in turn (where v is small the step's own
    g g (1 - b2) shows in v', as it does early in training)."""
    gen = torch.Generator().manual_seed(100003 * ADAM_KINDS.index(kind) + 31 * n + step)
    s = {"unit": 1.0, "tiny": 1e-6, "zero": 0.0}[kind]
    p = torch.randn(n, generator=gen)
    p[::2] = 0.0
    g = torch.randn(n, generator=gen) * s
    m = torch.randn(n, generator=gen) * (0.5 * s)
    v = torch.rand(n, generator=gen) * (s * s) * 10.0 ** -((3 - torch.arange(n)) % 4).float()
    return p, g, m, v


# ------------------------------------------------------------------ loss scaler
AMP_NS = [1, 3, 4, 5, 1024, 1027, 70001]
AMP_BAD = (float("inf"), float("-inf"), float("nan"))
FLT_MAX = float(np.finfo(np.float32).max)


def amp_positions(n):
    """{class: index} of where a single non-finite gradient is placed: element 0, inside the 4-wide body, the last full vector, each
    of the 1-3 tail elements, the first element of a block other than block 0 (256 threads x 4 elements = 1024 per block)"""
    n4 = n // 4
    pos = {"first": 0}
    if n4 > 2:
        pos["body"] = 4 * (n4 // 2) + 1
    if n4 > 0:
        pos["last vector"] = 4 * n4 - 1
    for k in range(n % 4):
        pos["tail %d" % k] = 4 * n4 + k
    if n4 > 256:
        pos["block 1"] = 1024
    return pos


def amp_model(st, found_inf, growth, backoff, interval):
    """The protocol of amp.py on the 6-float state [scale, 1/scale, found_inf, skip, streak, steps], in fp32 arithmetic:
    one rpe_amp_unscale (which can only SET found_inf) followed by one rpe_amp_update."""
    f = np.float32
    scale, inv, found, skip, streak, steps = (f(x) for x in st)
    if found_inf or found != 0:
        scale = max(f(scale * f(backoff)), f(1.0))
        inv, skip, streak = f(1.0) / scale, f(1.0), f(0.0)
    else:
        skip, steps, streak = f(0.0), f(steps + f(1.0)), f(streak + f(1.0))
        if streak >= f(interval):
            scale = min(f(scale * f(growth)), f(16777216.0))
            inv, streak = f(1.0) / scale, f(0.0)
    return [float(x) for x in (scale, inv, 0.0, skip, streak, steps)]
