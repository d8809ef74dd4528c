"""numpy restatement of the device minibatch sampler (rpe_sample_windows, rpe_gather_rows), written from its specification (DESIGN.md
"Minibatch sampling") and not from the kernels.  Everything is unsigned / Python-integer arithmetic, so the kernels are compared with
`np.array_equal` -- there is nothing to round.

    desc: a dict with the fields of rpe_sample_desc (seed, E, T, S, stride, N, shuffle)
    window_counts(desc)            -> (K, M)
    permute(pos, M, epoch, seed)   -> the epoch's keyed bijection of [0, M) at the positions `pos`
    window_index(desc, sel, step)  -> (1 + 2 N,) int32, the table the index kernel writes
    gather(pool, index, S)         -> (S, N, ...) array, the rows the gather kernel copies
"""
import numpy as np

from _augment_oracle import philox4x32

PURPOSE = 0x53414D50


def window_counts(desc):
    k = (int(desc["T"]) - int(desc["S"])) // int(desc["stride"]) + 1
    return k, int(desc["E"]) * k


def half_bits(m):
    return (max(int(m - 1).bit_length(), 2) + 1) // 2


def _feistel(x, h, epoch, seed):
    """one pass of the 4-round balanced Feistel network over 2h bits: x uint64 array -> uint64 array"""
    mask = np.uint64((1 << h) - 1)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    left, right = x >> np.uint64(h), x & mask
    for r in range(4):
        f = philox4x32((right, r, epoch & 0xFFFFFFFF, PURPOSE), key)[0]
        left, right = right, left ^ (f & mask)
    return (left << np.uint64(h)) | right


def permute(pos, m, epoch, seed, walks=None):
    """pos: integers in [0, M) -> their images under the bijection of (seed, epoch); `walks`, a list, receives the number of passes"""
    m, epoch, seed = int(m), int(epoch), int(seed)
    x = np.asarray(pos, dtype=np.uint64).copy()
    if m == 1:
        return np.zeros_like(x)
    h = half_bits(m)
    todo = np.ones(x.shape, dtype=bool)
    passes = 0
    while todo.any():      # cycle walking: again while the value is >= M
        x[todo] = _feistel(x[todo], h, epoch, seed)
        todo &= x >= np.uint64(m)
        passes += 1
    if walks is not None:
        walks.append(passes)
    return x


def window_index(desc, sel, step):
    n, stride = int(desc["N"]), int(desc["stride"])
    k, m = window_counts(desc)
    sel = np.asarray(sel)
    out = np.zeros(1 + 2 * n, dtype=np.int64)
    out[0] = int(step)
    for i in range(n):
        g = int(step) * n + i
        epoch, pos = divmod(g, m)
        w = int(permute([pos], m, epoch, desc["seed"])[0]) if desc["shuffle"] else pos
        out[1 + 2 * i] = sel[w // k]
        out[2 + 2 * i] = (w % k) * stride
    out[0] = out[0] - (1 << 32) if out[0] >= (1 << 31) else out[0]     # the counter is stored as 32 bits
    return out.astype(np.int32)


def gather(pool, index, s):
    """pool (E_file, T, ...) -> (S, N, ...): out[j, n] = pool[episode[n], t0[n] + j]"""
    index = np.asarray(index)
    ep, t0 = index[1::2], index[2::2]
    return np.stack([pool[ep, t0 + j] for j in range(int(s))], 0)
