"""numpy restatement of the occlusion-sensitivity specification (DESIGN.md "Occlusion sensitivity"; include/rpe_hip.h), written from the
specification and not from the kernels: the grid, the occluded batch, the per-pixel map, the overlay, and the displacement in float64.
The kernels are compared with it in tests/test_gpu_saliency.py; its own properties are checked in tests/test_saliency_cpu.py."""
import numpy as np


def pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def grid(hs, ws, patch, stride):
    """-> (Gy, Gx, tops, lefts)"""
    (ph, pw), (sy, sx) = pair(patch), pair(stride)
    gy = -(-(hs - ph) // sy) + 1
    gx = -(-(ws - pw) // sx) + 1
    return gy, gx, [min(g * sy, hs - ph) for g in range(gy)], [min(g * sx, ws - pw) for g in range(gx)]


def rectangles(hs, ws, patch, stride):
    """-> [(top, left)] in the order k = gy Gx + gx"""
    _, _, tops, lefts = grid(hs, ws, patch, stride)
    return [(t, l) for t in tops for l in lefts]


def occluded_batch(frame, patch, stride, fill, b, k0):
    """frame uint8 (Hs, Ws, 3) -> uint8 (b, Hs, Ws, 3): row 0 the frame, row r >= 1 with rectangle k0 + r - 1 filled, rows past K the frame"""
    hs, ws = frame.shape[:2]
    ph, pw = pair(patch)
    rects = rectangles(hs, ws, patch, stride)
    out = np.repeat(frame[None], b, axis=0).copy()
    for r in range(1, b):
        k = k0 + r - 1
        if k < len(rects):
            t, l = rects[k]
            out[r, t:t + ph, l:l + pw] = np.asarray(fill, dtype=np.uint8)
    return out


def coverage(hs, ws, patch, stride):
    """int (Hs, Ws): how many rectangles cover each pixel"""
    ph, pw = pair(patch)
    n = np.zeros((hs, ws), dtype=np.int64)
    for t, l in rectangles(hs, ws, patch, stride):
        n[t:t + ph, l:l + pw] += 1
    return n


def saliency_map(scores, hs, ws, patch, stride):
    """scores fp32 (M, K) -> (maps fp32 (M, Hs, Ws), minmax fp32 (M, 2)): an fp32 sum from 0 over the covering rectangles in ascending k
    (ascending gy, then gx), one rounded add each, then one rounded division by the count; minmax over the finite values, (+inf, -inf)
    without one"""
    ph, pw = pair(patch)
    scores = np.asarray(scores, dtype=np.float32).reshape(len(scores), -1)
    rects = rectangles(hs, ws, patch, stride)
    assert scores.shape[1] == len(rects)
    acc = np.zeros((scores.shape[0], hs, ws), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, (t, l) in enumerate(rects):
            acc[:, t:t + ph, l:l + pw] = acc[:, t:t + ph, l:l + pw] + scores[:, k, None, None]     # float32 + float32: one rounding
        maps = acc / coverage(hs, ws, patch, stride).astype(np.float32)[None]
    assert maps.dtype == np.float32
    return maps, finite_minmax(maps)


def finite_minmax(maps):
    mm = np.empty((maps.shape[0], 2), dtype=np.float32)
    for m in range(maps.shape[0]):
        v = maps[m][np.isfinite(maps[m])]
        mm[m] = (v.min(), v.max()) if v.size else (np.inf, -np.inf)
    return mm


def overlay(frame, smap, lo, hi, table, alpha_q8, fade):
    """-> uint8 (Hs, Ws, 3).  The colour index in fp32, one rounded operation each; everything behind it in integers."""
    smap = np.asarray(smap, dtype=np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    finite = np.isfinite(smap)
    k = np.zeros(smap.shape, dtype=np.int64)
    if hi != lo:
        with np.errstate(invalid="ignore", over="ignore"):
            t = (np.where(finite, smap, lo) - lo) / (hi - lo)          # float32 throughout
            assert t.dtype == np.float32
            k = np.minimum(255, (t * np.float32(256)).astype(np.int64))
    a = (alpha_q8 * k) >> 8 if fade else np.full(smap.shape, alpha_q8, dtype=np.int64)
    f = frame.astype(np.int64)
    out = (f * (256 - a)[..., None] + table.astype(np.int64)[k] * a[..., None] + 128) >> 8
    out = np.where(finite[..., None], out, f)
    return out.astype(np.uint8)


def pose_displacement(pred, ref):
    """float64 throughout, rounded once: pred (n, 7), ref (7,) fp32 -> (pos (n,), ori (n,)) fp32"""
    p, r = np.asarray(pred, dtype=np.float64).reshape(-1, 7), np.asarray(ref, dtype=np.float64).reshape(7)
    with np.errstate(invalid="ignore", divide="ignore"):
        pos = np.sqrt(((p[:, :3] - r[:3]) ** 2).sum(-1))
        a = p[:, 3:] / np.sqrt((p[:, 3:] ** 2).sum(-1, keepdims=True))
        b = r[3:] / np.sqrt((r[3:] ** 2).sum())
        dm, dp = np.sqrt(((a - b) ** 2).sum(-1)), np.sqrt(((a + b) ** 2).sum(-1))
        ori = 4.0 * np.arctan2(np.minimum(dm, dp), np.maximum(dm, dp))
    return pos.astype(np.float32), ori.astype(np.float32)
