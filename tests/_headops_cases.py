"""Cases of the head-op tests (tests/test_headops_cpu.py, tests/test_gpu_headops.py): LinearOp / LSTMOp of headops.py on their own, and
the head graphs of the five model classes with the trunk cut off.  Everything is fp32 on the CPU, drawn from a generator seeded by the
case, so the CPU self-test and the GPU test see the same values."""
import torch

SENT = -12345.5   # gradient views and caller-owned outputs are prefilled with it: whatever a launch must not touch keeps it

# (M, N, K, relu, bias)
LINEAR_CASES = [
    (5, 7, 64, False, True),       # few-row kernel, N % 4 != 0
    (9, 7, 64, False, True),       # one row past LINEAR_ROWS_MAX: the tile kernel
    (8, 12, 50, True, True),       # few-row kernel, weight read in place with K % 4 != 0
    (24, 12, 50, True, True),      # _w() padded copy, tmp weight-gradient path, copy2d
    (33, 130, 259, True, True),    # partial N tile, odd K
    (300, 7, 4100, False, True),   # split-K forward
    (16, 8, 8, False, None),       # no bias
]
SPLIT_K_CASE = (300, 7, 4100, False, True)

# (S, N, I, H, h0 / c0 given)
LSTM_CASES = [
    (1, 1, 7, 4, False),       # no recurrent GEMM, no w_hh gradient launch: that gradient is exactly zero
    (1, 3, 12, 8, True),       # S == 1 with the h0 term only
    (4, 1, 57, 16, False),     # a rollout lane, I % 4 != 0
    (3, 8, 64, 32, True),      # N equal to the few-row limit
    (5, 9, 57, 64, False),     # first tile-path N
    (6, 40, 128, 100, True),   # H % 4 == 0 but % 8 != 0, 4H = 400
    (2, 130, 64, 256, False),  # partial M tile, K = 256 recurrent GEMM
]
LSTM_ZERO = {(1, 1, 7, 4, False): ("w_hh",)}   # reference tensors that are exactly zero: the result must be, too

# the head graphs: leads of the two one-shot families and of the three sequence families (S, N)
GRAPH_LEADS = {"n": [(3,), (9,)], "no": [(3,), (9,)], "td": [(1, 1), (3, 2), (2, 9)], "tdo": [(1, 1), (3, 2), (2, 9)],
               "tdo_v2": [(1, 1), (3, 2), (2, 9)]}
TWO_OUTPUTS = ("n", "td")
SEQUENCE = ("td", "tdo", "tdo_v2")
# carried-state names of the sequence families and the LSTM module each belongs to (models/time_sensitive.py)
STATE_TAGS = {"td": {"pre": "pre_measurement_rnn", "post": "post_measurement_rnn"}, "tdo": {"rnn": "rnn"},
              "tdo_v2": {"img": "img_rnn", "proprio": "proprio_rnn"}}


def case_id(case):
    return "-".join("x" if v is None else str(int(v)) if isinstance(v, bool) else str(v) for v in case)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _u(g, *shape):
    return torch.rand(*shape, generator=g) * 2.0 - 1.0


def linear_data(case, seed=0):
    """-> w [N, K], b [N] or None, two (x [M, K], dy [M, N]) pairs, an addend [M, N]"""
    m, n, k, relu, bias = case
    g = _gen(7000 + 131 * m + 17 * n + k + seed)
    d = dict(w=_u(g, n, k) / k ** 0.5 * 1.5, b=_u(g, n) * 0.5 if bias else None)
    for i in (1, 2):
        d["x%d" % i] = torch.randn(m, k, generator=g)
        d["dy%d" % i] = torch.randn(m, n, generator=g)
    d["add"] = torch.randn(m, n, generator=g)
    return d


def lstm_data(case, seed=0):
    """-> the four parameters (torch gate order), x [S*N, I], dh [S*N, H] and (h0, c0) [N, H] or None"""
    s, n, i, h, given = case
    g = _gen(9000 + 1009 * s + 131 * n + 17 * i + h + seed)
    d = dict(w_ih=_u(g, 4 * h, i) / i ** 0.5 * 1.5, w_hh=_u(g, 4 * h, h) / h ** 0.5 * 1.5, b_ih=_u(g, 4 * h) * 0.5, b_hh=_u(g, 4 * h) * 0.5,
             x=torch.randn(s * n, i, generator=g), dh=torch.randn(s * n, h, generator=g), h0=None, c0=None)
    if given:
        d["h0"] = torch.tanh(torch.randn(n, h, generator=g)) * 0.7
        d["c0"] = torch.randn(n, h, generator=g) * 0.7
    return d


def graph_data(kind, lead, fdim, hidden, seed=0):
    """Inputs of one head-graph step: feat [B, fdim] (the feature columns of the rows), x0bar [B, 7], one output gradient [B, 7] per
    output, and a non-zero carried (h, c) [N, hid] per LSTM of a sequence family (hidden: tag -> hid)."""
    b = 1
    for v in lead:
        b *= v
    g = _gen(5000 + 977 * len(kind) + 31 * b + lead[-1] + seed)
    d = dict(feat=torch.randn(b, fdim, generator=g), x0bar=torch.randn(b, 7, generator=g) * 0.5,
             d_outs=[torch.randn(b, 7, generator=g) for _ in range(2 if kind in TWO_OUTPUTS else 1)], state={})
    for tag, hid in hidden.items():
        d["state"][tag] = (torch.tanh(torch.randn(lead[-1], hid, generator=g)) * 0.7, torch.randn(lead[-1], hid, generator=g) * 0.7)
    return d
