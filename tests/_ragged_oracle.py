"""numpy restatement of the device code for episodes of unequal length, written from the specification (DESIGN.md "Minibatch sampling",
"Unequal lengths"; include/rpe_hip.h) and not from the kernels.

The window index (rpe_sample_windows_ragged) is unsigned / Python-integer arithmetic, so the kernel is compared with `np.array_equal`;
the keyed bijection and the gather are those of tests/_sampler_oracle.py.  The statistics (rpe_error_stats_ragged) are float64 numpy
over the valid entries.

    desc: a dict with the fields of rpe_sample_desc (seed, E, T, S, stride, N, shuffle)
    window_table(desc, sel, lengths)        -> (K_e list, P list of E + 1 prefix sums, M)
    window_index(desc, sel, lengths, step)  -> (1 + 2 N,) int32, the table the index kernel writes
    valid_windows(desc, sel, lengths)       -> every (episode number in the file, t0) that exists, in table order
    error_stats(err, lengths)               -> (3 + 2 E,) float64: mean, population std, max, sum[E], mean[E] over the valid entries
    valid_mask(lengths, T)                  -> (E, T) bool
"""
import numpy as np

from _sampler_oracle import gather, permute  # noqa: F401  (gather: re-exported for the tests)


def window_table(desc, sel, lengths):
    """lengths: one entry per episode IN THE FILE, read through sel"""
    t, s, stride = int(desc["T"]), int(desc["S"]), int(desc["stride"])
    ks = []
    for e in range(int(desc["E"])):
        n = min(max(int(lengths[int(sel[e])]), 0), t)
        ks.append((n - s) // stride + 1 if n >= s else 0)
    prefix = [0]
    for k in ks:
        prefix.append(prefix[-1] + k)
    return ks, prefix, prefix[-1]


def window_index(desc, sel, lengths, step):
    n, stride = int(desc["N"]), int(desc["stride"])
    _, prefix, m = window_table(desc, sel, lengths)
    out = np.zeros(1 + 2 * n, dtype=np.int64)
    out[0] = int(step)
    for i in range(n):
        if m == 0:
            out[1 + 2 * i], out[2 + 2 * i] = int(sel[0]), 0
            continue
        g = int(step) * n + i
        epoch, pos = divmod(g, m)
        w = int(permute([pos], m, epoch, desc["seed"])[0]) if desc["shuffle"] else pos
        e = max(j for j in range(int(desc["E"])) if prefix[j] <= w)     # the largest index with P_e <= w
        out[1 + 2 * i] = int(sel[e])
        out[2 + 2 * i] = (w - prefix[e]) * stride
    out[0] = out[0] - (1 << 32) if out[0] >= (1 << 31) else out[0]      # the counter is stored as 32 bits
    return out.astype(np.int32)


def window_index_fast(desc, sel, lengths, step):
    """window_index with the episode found by np.searchsorted: the same table for thousands of episodes (checked against window_index
    in tests/test_ragged_cpu.py)"""
    n, stride = int(desc["N"]), int(desc["stride"])
    _, prefix, m = window_table(desc, sel, lengths)
    sel = np.asarray(sel, dtype=np.int64)
    out = np.zeros(1 + 2 * n, dtype=np.int64)
    out[0] = int(step) - (1 << 32) if int(step) >= (1 << 31) else int(step)
    if m == 0:
        out[1::2] = sel[0]
        return out.astype(np.int32)
    g = int(step) * n + np.arange(n, dtype=object)
    w = np.zeros(n, dtype=np.int64)
    for i in range(n):
        epoch, pos = divmod(int(g[i]), m)
        w[i] = int(permute([pos], m, epoch, desc["seed"])[0]) if desc["shuffle"] else pos
    p = np.asarray(prefix[:-1], dtype=np.int64)
    e = np.searchsorted(p, w, side="right") - 1
    out[1::2] = sel[e]
    out[2::2] = (w - p[e]) * stride
    return out.astype(np.int32)


def valid_windows(desc, sel, lengths):
    ks, _, _ = window_table(desc, sel, lengths)
    return [(int(sel[e]), j * int(desc["stride"])) for e, k in enumerate(ks) for j in range(k)]


def valid_mask(lengths, t):
    return np.arange(int(t))[None, :] < np.asarray(lengths)[:, None]


def error_stats(err, lengths):
    x = np.asarray(err, dtype=np.float64)
    rows = [x[e, :int(n)] for e, n in enumerate(lengths)]
    flat = np.concatenate(rows)
    with np.errstate(invalid="ignore"):
        return np.concatenate([[flat.mean(), flat.std(), np.nan if np.isnan(flat).any() else flat.max()], [r.sum() for r in rows], [r.mean() for r in rows]])
