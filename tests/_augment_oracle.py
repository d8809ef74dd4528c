"""numpy restatement of the device frame augmentation (rpe_augment_frames_u8), written from its specification and not from the
kernel: Philox4x32-10, the parameter draws and the five integer stages.  Everything is int64 / uint64 arithmetic, so the kernel is
compared with `np.array_equal` -- there is nothing to round.

    desc: a dict with the fields of rpe_augment_desc (`neutral_desc` gives the identity settings)
    params_table(desc, B, Hs, Ws, step) -> (1 + 8 G,) int32, the table the parameter kernel writes
    augment(frames, desc, step)         -> (out uint8 of frames' shape, params table, per-frame sums of grey(v1))
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
Q1 = 65536


def philox4x32(counter, key, rounds=10):
    """counter: four arrays (or ints) of 32-bit words, key: two; -> four uint64 arrays holding 32-bit words"""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in np.broadcast_arrays(*counter)]
    k = [np.asarray(x, dtype=np.uint64) & MASK for x in key]
    for r in range(rounds):
        if r:
            k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]     # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
    return c


def draw(r, n):
    """bounded draw over n values from 32-bit words r: (r * n) >> 32"""
    return ((np.asarray(r, dtype=np.uint64) * np.uint64(int(n))) >> np.uint64(32)).astype(np.int64)


def neutral_desc(**kw):
    d = dict(seed=0, qb_lo=Q1, qb_hi=Q1, qc_lo=Q1, qc_hi=Q1, qs_lo=Q1, qs_hi=Q1, noise_q=0, erase_thresh=0, eh_lo=1, eh_hi=1, ew_lo=1, ew_hi=1,
             fill_mode=0, fill_rgb=(124, 116, 104), group=0)
    unknown = set(kw) - set(d)
    assert not unknown, unknown
    d.update(kw)
    return d


def _key(desc):
    seed = int(desc["seed"])
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def stream_params(desc, G, Hs, Ws, step):
    """the draws of streams 0 .. G-1 at `step`: dict of (G,) int64 arrays qb qc qs erase top left h w"""
    g = np.arange(G, dtype=np.uint64)
    r = philox4x32((g, 0, step, 0), _key(desc))
    p = {}
    for name, word in (("qb", r[0]), ("qc", r[1]), ("qs", r[2])):
        lo, hi = desc[name + "_lo"], desc[name + "_hi"]
        p[name] = lo + draw(word, hi - lo + 1)
    p["erase"] = (r[3] < np.uint64(desc["erase_thresh"])).astype(np.int64)
    r = philox4x32((g, 0, step, 1), _key(desc))
    p["h"] = desc["eh_lo"] + draw(r[0], desc["eh_hi"] - desc["eh_lo"] + 1)
    p["w"] = desc["ew_lo"] + draw(r[1], desc["ew_hi"] - desc["ew_lo"] + 1)
    p["top"] = ((r[2] * (np.uint64(Hs) - p["h"].astype(np.uint64) + np.uint64(1))) >> np.uint64(32)).astype(np.int64)
    p["left"] = ((r[3] * (np.uint64(Ws) - p["w"].astype(np.uint64) + np.uint64(1))) >> np.uint64(32)).astype(np.int64)
    return p


def num_streams(desc, B):
    return desc["group"] if desc["group"] > 0 else B


def params_table(desc, B, Hs, Ws, step):
    G = num_streams(desc, B)
    p = stream_params(desc, G, Hs, Ws, step)
    rows = np.stack([p[k] for k in ("qb", "qc", "qs", "erase", "top", "left", "h", "w")], 1)
    step32 = np.array([step & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)
    return np.concatenate([step32, rows.reshape(-1).astype(np.int32)])


def grey(v):
    return (77 * v[..., 0] + 150 * v[..., 1] + 29 * v[..., 2] + 128) >> 8


def _clamp(v):
    return np.clip(v, 0, 255)


def augment(frames, desc, step):
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.shape[-1] == 3 and frames.ndim >= 4
    Hs, Ws = frames.shape[-3:-1]
    v = frames.reshape(-1, Hs, Ws, 3).astype(np.int64)
    B, P = v.shape[0], Hs * Ws
    G = num_streams(desc, B)
    p = stream_params(desc, G, Hs, Ws, step)
    stream = np.arange(B) % G if desc["group"] > 0 else np.arange(B)
    per = lambda name: p[name][stream].reshape(B, 1, 1, 1)
    qb, qc, qs = per("qb"), per("qc"), per("qs")
    # 1 brightness
    v1 = _clamp((v * qb + 32768) >> 16)
    # 2 contrast
    sums = grey(v1).reshape(B, -1).sum(1)
    m = ((sums + P // 2) // P).reshape(B, 1, 1, 1)
    v2 = _clamp((v1 * qc + m * (Q1 - qc) + 32768) >> 16)
    # 3 saturation
    g = grey(v2)[..., None]
    v3 = _clamp((v2 * qs + g * (Q1 - qs) + 32768) >> 16)
    # 4 noise, 5 the random fill: purpose 2, counter (pixel, frame, step, 2)
    pix = np.arange(P, dtype=np.uint64).reshape(1, Hs, Ws)
    fr = np.arange(B, dtype=np.uint64).reshape(B, 1, 1)
    r = philox4x32((pix, fr, step, 2), _key(desc))
    byte_sum = lambda w: sum(((w >> np.uint64(8 * i)) & np.uint64(255)).astype(np.int64) for i in range(4))
    n = np.stack([(((byte_sum(r[c]) - 510) * int(desc["noise_q"])) + 32768) >> 16 for c in range(3)], -1)
    v4 = _clamp(v3 + n)
    # 5 erase
    y = np.arange(Hs).reshape(1, Hs, 1)
    x = np.arange(Ws).reshape(1, 1, Ws)
    e = lambda name: p[name][stream].reshape(B, 1, 1)
    inside = (e("erase") != 0) & (y >= e("top")) & (y < e("top") + e("h")) & (x >= e("left")) & (x < e("left") + e("w"))
    if desc["fill_mode"] == 1:
        fill = np.stack([((r[3] >> np.uint64(8 * c)) & np.uint64(255)).astype(np.int64) for c in range(3)], -1)
    else:
        fill = np.broadcast_to(np.asarray(desc["fill_rgb"], dtype=np.int64), v4.shape)
    out = np.where(inside[..., None], fill, v4).astype(np.uint8).reshape(frames.shape)
    return out, params_table(desc, B, Hs, Ws, step), sums.astype(np.uint64)
