"""The head-dropout rule ("Head dropout"; csrc/dropout.hip) restated in numpy -- what the kernel is compared with, bit for bit.

Element (r, c) of an fp32 [n][ld] matrix, c the ABSOLUTE column, at step `step` of site `site` under the 64-bit `seed`:
    words = Philox4x32-10 at counter (r, c >> 2, step, 0x44524F50 + site), key (seed low word, seed high word)
    word  = words[c & 3];  kept iff word >= thresh
    kept: x * scale, one fp32 multiply;  dropped: +0.0 by selection (a NaN or an infinity does not survive, -0 does not appear)
with thresh = min(2^32 - 1, round(p 2^32)) and scale = float32(1 / (1 - p)) divided in double, for 0 <= p < 1.  Only the columns
[c0, c1) are touched; an element's mask depends on nothing but (seed, step, site, r, c)."""
import numpy as np

from _augment_oracle import philox4x32

PURPOSE = 0x44524F50      # "DROP"; + site
SITES = 4


def thresh_scale(p):
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("p must lie in [0, 1); got %r" % (p,))
    return min(2 ** 32 - 1, int(round(p * 2 ** 32))), np.float32(1.0 / (1.0 - p))


def words(seed, step, site, rows, cols):
    """-> uint32 [len(rows), len(cols)]: the word of every element (r, c), r in rows, c in cols (absolute indices)"""
    if not 0 <= site < SITES:
        raise ValueError("site must lie in [0, %d)" % SITES)
    r = np.asarray(rows, dtype=np.uint64)[:, None]
    c = np.asarray(cols, dtype=np.uint64)[None, :]
    w = philox4x32((r, c >> np.uint64(2), int(step) & 0xFFFFFFFF, PURPOSE + site), (int(seed) & 0xFFFFFFFF, int(seed) >> 32))
    lane = np.broadcast_to(c & np.uint64(3), w[0].shape)
    return np.choose(lane.astype(np.int64), [np.broadcast_to(x, lane.shape) for x in w]).astype(np.uint32)


def keep_mask(seed, step, site, n, c0, c1, p):
    """-> bool [n, c1 - c0]: True where element (r, c0 + j) is kept"""
    thresh, _ = thresh_scale(p)
    return words(seed, step, site, np.arange(n), np.arange(c0, c1)) >= np.uint32(thresh)


def dropout_rows(x, seed, step, site, p, c0=0, c1=None, out=None):
    """x fp32 [n, ld] -> the matrix the kernel leaves: columns [c0, c1) dropped, every other column as `out` held it (x itself when
    out is None: the in-place form)"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    n, ld = x.shape
    c1 = ld if c1 is None else c1
    if not (n >= 1 and 0 <= c0 < c1 <= ld):
        raise ValueError("need n >= 1 and 0 <= c0 < c1 <= ld")
    _, scale = thresh_scale(p)
    res = np.array(x if out is None else out, dtype=np.float32, copy=True)
    keep = keep_mask(seed, step, site, n, c0, c1, p)
    with np.errstate(all="ignore"):
        res[:, c0:c1] = np.where(keep, x[:, c0:c1] * scale, np.float32(0.0))
    return res


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)
