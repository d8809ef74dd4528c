"""numpy restatement of the device frame blur (rpe_blur_frames_u8), written from its specification (DESIGN.md "Frame blur") and not
from the kernel: the stream draws, the separable integer Gaussian and the nearest-pixel motion blur, both with a replicate border.
Everything is int64 arithmetic, so the kernel is compared with `np.array_equal` -- there is nothing to round.

    desc: a dict with the arguments of ops.blur_desc, i.e. the fields of rpe_blur_desc (`neutral_desc` blurs nothing)
    gauss_taps(sigma)                   -> (R, [w_0 .. w_R]), the host's table of one sigma
    directions(nd)                      -> (cx, cy), the Q8 direction components
    blur_params_table(desc, B, step)    -> (1 + 4 G,) int32, the table the parameter kernel writes
    blur(frames, desc, step)            -> (out uint8 of frames' shape, params table)
"""
import math

import numpy as np

from _augment_oracle import draw, philox4x32

PURPOSE = 0x424C5552   # "BLUR"
FULL = 2 ** 32 - 1
TAP_SUM = 2048
LIMIT = 2 ** 31


def gauss_taps(sigma):
    sigma = float(sigma)
    if sigma == 0.0:
        return 0, [TAP_SUM]
    r = min(8, max(1, int(math.ceil(3.0 * sigma))))
    g = [math.exp(-k * k / (2.0 * sigma * sigma)) for k in range(r + 1)]
    total = g[0] + 2.0 * sum(g[1:])
    w = [int(round(TAP_SUM * v / total)) for v in g]
    w[0] = TAP_SUM - 2 * sum(w[1:])
    return r, w


def directions(nd):
    return ([int(round(256.0 * math.cos(math.pi * d / nd))) for d in range(nd)], [int(round(256.0 * math.sin(math.pi * d / nd))) for d in range(nd)])


def neutral_desc(**kw):
    d = dict(seed=0, gauss_thresh=0, motion_thresh=0, radius=(0,), taps=((TAP_SUM,),), n_lengths=1, dir_cx=(256,), dir_cy=(0,), group=0)
    unknown = set(kw) - set(d)
    assert not unknown, unknown
    d.update(kw)
    return d


def num_streams(desc, B):
    return desc["group"] if desc["group"] > 0 else B


def _key(desc):
    seed = int(desc["seed"])
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def stream_params(desc, G, step):
    """the draws of streams 0 .. G-1 at `step`: dict of (G,) int64 arrays kind level L d"""
    assert desc["gauss_thresh"] + desc["motion_thresh"] <= FULL
    r = philox4x32((np.arange(G, dtype=np.uint64), 0, step, PURPOSE), _key(desc))
    r0 = r[0].astype(np.int64)
    kind = np.where(r0 < desc["gauss_thresh"], 1, np.where(r0 < desc["gauss_thresh"] + desc["motion_thresh"], 2, 0)).astype(np.int64)
    return dict(kind=kind, level=draw(r[1], len(desc["radius"])), L=3 + 2 * draw(r[2], desc["n_lengths"]), d=draw(r[3], len(desc["dir_cx"])))


def blur_params_table(desc, B, step):
    p = stream_params(desc, num_streams(desc, B), step)
    rows = np.stack([p[k] for k in ("kind", "level", "L", "d")], 1)
    step32 = np.array([step & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)
    return np.concatenate([step32, rows.reshape(-1).astype(np.int32)])


def blur_gauss(v, radius, taps):
    """v int64 (Hs, Ws, C) -> the Gaussian blur with half-kernel taps[0 .. radius], replicate border"""
    hs, ws = v.shape[:2]
    w = [int(t) for t in taps[:radius + 1]]
    assert all(t >= 0 for t in w) and w[0] + 2 * sum(w[1:]) == TAP_SUM
    x, y = np.arange(ws), np.arange(hs)
    h = np.zeros_like(v)
    for k in range(-radius, radius + 1):
        h += w[abs(k)] * v[:, np.clip(x + k, 0, ws - 1)]
    assert h.max() <= 255 * TAP_SUM
    acc = np.zeros_like(v)
    for k in range(-radius, radius + 1):
        acc += w[abs(k)] * h[np.clip(y + k, 0, hs - 1)]
    acc += 1 << 21
    assert acc.max() < LIMIT
    return acc >> 22


def motion_offsets(length, cx, cy):
    """the (dx, dy) of the taps t = -(L-1)/2 .. (L-1)/2, with floor shifts"""
    assert length % 2 == 1 and 3 <= length <= 15 and abs(cx) <= 256 and abs(cy) <= 256
    t = np.arange(-(length - 1) // 2, (length - 1) // 2 + 1, dtype=np.int64)
    return (t * cx + 128) >> 8, (t * cy + 128) >> 8


def blur_motion(v, length, cx, cy):
    """v int64 (Hs, Ws, C) -> the motion blur of odd `length` along the Q8 direction (cx, cy), replicate border"""
    hs, ws = v.shape[:2]
    dx, dy = motion_offsets(length, cx, cy)
    assert np.abs(dx).max() <= 7 and np.abs(dy).max() <= 7
    x, y = np.arange(ws), np.arange(hs)
    s = np.zeros_like(v)
    for ox, oy in zip(dx, dy):
        s += v[np.clip(y + oy, 0, hs - 1)][:, np.clip(x + ox, 0, ws - 1)]
    n = 2 * s + length
    assert n.max() < LIMIT
    return n // (2 * length)


def blur(frames, desc, step):
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.shape[-1] == 3 and frames.ndim >= 4
    hs, ws = frames.shape[-3:-1]
    v = frames.reshape(-1, hs, ws, 3).astype(np.int64)
    B = v.shape[0]
    G = num_streams(desc, B)
    p = stream_params(desc, G, step)
    out = np.empty_like(v)
    for b in range(B):
        g = b % G if desc["group"] > 0 else b
        kind = int(p["kind"][g])
        if kind == 1:
            s = int(p["level"][g])
            out[b] = blur_gauss(v[b], int(desc["radius"][s]), desc["taps"][s])
        elif kind == 2:
            d = int(p["d"][g])
            out[b] = blur_motion(v[b], int(p["L"][g]), int(desc["dir_cx"][d]), int(desc["dir_cy"][d]))
        else:
            out[b] = v[b]
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8).reshape(frames.shape), blur_params_table(desc, B, step)
