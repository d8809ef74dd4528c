"""fp64 reference, with bounds, of the training telemetry (rpe_param_stats + rpe_param_stats_finalize, csrc/telemetry.hip): per tensor
of four fp32 arenas p, g, m, v the row

    0 sum g^2   1 sum p^2   2 sum d^2   3 max|g|   4 max|p|   5 non-finite g   6 g == 0   7 non-finite p   8 stamp   9 sticky step

with d = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps), bc1 = 1 - b1^t, bc2 = 1 - b2^t, everything widened to fp64 first.  A non-finite
element is counted and left out of every sum and maximum; a non-finite d is left out of sum d^2; a skipped step (state[3] != 0)
reports sum d^2 = 0; column 9 keeps the first stamp at which column 5 or 7 was non-zero.

Bounds (derived, in the manner of tests/_bounds.py; u = 2^-53, fp64's unit roundoff, takes the place of u32 there):
- columns 3 .. 9 are exact: bits are compared.
- columns 0, 1: every term x^2 is exact in fp64 (a 24-bit significand squares into 48 bits; the exponent range of fp32 squared lies
  inside fp64's), so only the order of the additions can differ.  Any order of n - 1 additions of non-negative terms errs by at most
  gamma(n - 1) S with gamma(k) = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  The reference
  sum is math.fsum, which is correctly rounded: for n = 1 both are exact, for n = 2 both are the one correctly rounded sum, and from
  n = 3 on the kernel's tree (depth about log2 n) stays far enough below n - 1 sequential additions for the reference's half ulp.
  The bound is below two ulps of the sum for n < 5, so there a difference of one ulp -- the smallest there is -- already exceeds half
  of it: the half-bound gate of tests/test_telemetry_cpu.py is held from n = 64 on, smaller tensors at the full bound.
- column 2: every term carries a relative bound r, carried through the operations as Fx does it -- a rounding costs EW u (EW = 3:
  one for the kernel, one for the reference, one spare, which is what keeps a correct evaluation at half the bound), pow costs TR u
  (TR = 4), and 1 - b^t divides pow's error by the difference, which is where the bound grows (b2 = 0.999, t = 1: a factor 1000).
  m and v are exact operands, v >= 0 and eps >= 0, so nothing else cancels and r is ONE number per (t, b1, b2).  Then
  |err| <= (r + gamma(n - 1) (1 + r)) S.
n is the tensor's element count, whatever share of it is finite: more terms than were added only widens nothing that matters."""
import math

import numpy as np

from _bounds import EW, TR

U64 = 2.0 ** -53
COLS = 10
SUM_COLS, EXACT_COLS = (0, 1, 2), (3, 4, 5, 6, 7, 8, 9)


def gamma(k):
    return 0.0 if k <= 0 else k * U64 / (1.0 - k * U64)


def _div(ra, rb):
    """relative bound of a quotient of two values with relative bounds ra, rb"""
    return (ra + rb) / (1.0 - rb) + EW * U64


def direction_rel_bound(step, b1, b2):
    """r: the relative bound of one term d^2 (see the module docstring); inf where a bias correction is 0 (step 0)"""
    def complement(b):                      # 1 - b^t
        pw = b ** step
        c = 1.0 - pw
        return math.inf if c <= 0.0 else TR * U64 * pw / c + EW * U64
    r1, r2 = complement(b1), complement(b2)
    if not (r1 < 0.5 and r2 < 0.5):
        return math.inf
    rs = r2 + EW * U64                      # sqrt(bc2): the square root halves a relative error; taken whole
    num = _div(0.0, r1)                     # m / bc1
    den = _div(EW * U64, rs) + EW * U64     # sqrt(v) / sqrt(bc2), then + eps: two non-negative terms, eps exact
    d = _div(num, den)
    return 2.0 * d + d * d + EW * U64       # d d


def direction(m, v, step, b1, b2, eps):
    """d in fp64 from the fp32 moments, in the kernel's order of operations"""
    bc1, bc2s = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    with np.errstate(all="ignore"):
        return (m.astype(np.float64) / np.float64(bc1)) / (np.sqrt(v.astype(np.float64)) / np.float64(bc2s) + np.float64(eps))


def _pairwise(t):
    n = 1
    while n < max(1, t.size):
        n *= 2
    a = np.zeros(n, dtype=np.float64)
    a[:t.size] = t
    while a.size > 1:
        a = a[:a.size // 2] + a[a.size // 2:]
    return float(a[0])


def total(terms, order="exact"):
    """the sum of fp64 terms: exact (math.fsum, correctly rounded), forward / reversed (one after the other), pairwise (a tree)"""
    if order == "exact":
        if terms.size > 4096 and np.finfo(np.longdouble).nmant >= 63:
            # large tensors: numpy's pairwise sum in extended precision (u_ext <= 2^-64): its error, about log2(n) u_ext relative, is
            # thousands of times below u, so the rounded result is fsum's but for a rare double rounding of one more half ulp
            return float(np.sum(terms.astype(np.longdouble)))
        return math.fsum(terms.tolist())
    if order in ("forward", "reversed"):
        t = terms if order == "forward" else terms[::-1]
        return float(np.cumsum(t)[-1]) if t.size else 0.0
    if order == "pairwise":
        return _pairwise(terms)
    raise ValueError(order)


def tensor_row(p, g, m, v, step, b1, b2, eps, skip=False, order="exact"):
    """the eight reduced columns of one tensor (fp32 numpy arrays) -> (row (8,), bound (8,)), fp64"""
    p64, g64 = p.astype(np.float64), g.astype(np.float64)
    gf, pf = np.isfinite(g64), np.isfinite(p64)
    d = direction(m, v, step, b1, b2, eps)
    d = d[np.isfinite(d)]
    n = p.size
    g2, p2, d2 = total(g64[gf] ** 2, order), total(p64[pf] ** 2, order), 0.0 if skip else total(d * d, order)
    r = direction_rel_bound(step, b1, b2)
    row = np.array([g2, p2, d2, np.abs(g64[gf]).max(initial=0.0), np.abs(p64[pf]).max(initial=0.0), (~gf).sum(), (g64 == 0.0).sum(), (~pf).sum()],
                   dtype=np.float64)
    d2_bound = 0.0 if d2 == 0.0 else (r + gamma(n - 1) * (1.0 + r)) * d2
    return row, np.array([gamma(n - 1) * g2, gamma(n - 1) * p2, d2_bound, 0, 0, 0, 0, 0], dtype=np.float64)


def table_ref(p, g, m, v, entries, step, b1, b2, eps, skip=False, prev=None, order="exact"):
    """p, g, m, v: flat fp32 numpy arenas; entries: [(offset, numel)] -> (out (T, COLS), bound (T, COLS)) of one measured step.
    prev: the table before the step (its column 9 is kept where set); None: zeros."""
    out, bnd = np.zeros((len(entries), COLS)), np.zeros((len(entries), COLS))
    for t, (off, n) in enumerate(entries):
        sl = slice(off, off + n)
        out[t, :8], bnd[t, :8] = tensor_row(p[sl], g[sl], m[sl], v[sl], step, b1, b2, eps, skip, order)
        out[t, 8] = step
        before = 0.0 if prev is None else prev[t, 9]
        out[t, 9] = before if before != 0.0 else (step if out[t, 5] or out[t, 7] else 0.0)
    return out, bnd


def check_table(got, ref, bnd, label):
    """-> worst err / bound over the three sums (0 where the bound is 0 and the value exact); asserts columns 3 .. 9 bit-equal and the
    sums finite and within their bound.  Prints every figure before it asserts."""
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    worst = 0.0
    for c in SUM_COLS:
        err = np.abs(got[:, c] - ref[:, c])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0.0, 0.0, err / bnd[:, c])
        print("TELEMETRY %-44s col %d worst err/bound %.3f" % (label, c, float(np.nanmax(ratio)) if ratio.size else 0.0))
        assert np.isfinite(got[:, c]).all(), "%s: column %d is not finite: %s" % (label, c, got[:, c])
        assert (err <= bnd[:, c]).all(), "%s: column %d out of bound at tensors %s: got %s ref %s bound %s" % (
            label, c, np.nonzero(err > bnd[:, c])[0].tolist(), got[err > bnd[:, c], c], ref[err > bnd[:, c], c], bnd[err > bnd[:, c], c])
        worst = max(worst, float(np.nanmax(ratio)) if ratio.size else 0.0)
    for c in EXACT_COLS:
        assert (got[:, c].view(np.int64) == ref[:, c].view(np.int64)).all(), "%s: column %d differs: got %s ref %s" % (label, c, got[:, c], ref[:, c])
    return worst
