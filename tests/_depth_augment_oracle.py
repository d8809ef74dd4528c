"""numpy fp64 restatement of the device depth augmentation (rpe_augment_depth_f32), written from its specification ("Depth
augmentation") and not from the kernel.  Stages 1-3 are float64 with every product and every sum rounded on its own -- numpy never
fuses -- and ONE rounding to float32 at the end, so the kernel is compared with `np.array_equal` on the uint32 view of the floats.

    desc: a dict with the fields of rpe_depth_augment_desc (`neutral_desc` gives the identity settings)
    params_table(desc, B, Hs, Ws, step) -> (1 + 17 G,) int32, the table the parameter kernel writes
    pixel_words(desc, B, Hs, Ws, step)  -> the four Philox words of every pixel, (B, Hs, Ws) uint64 each
    noise_T(r)                          -> the integer T of the noise stage from those words
    augment(depth, desc, step, rgb_params=None) -> (out float32 of depth's shape, params table)
        rgb_params: the table _augment_oracle.params_table gives for the same batch and group -- the shared occluder
"""
import numpy as np

from _augment_oracle import draw, philox4x32

PURPOSE_COUNT, PURPOSE_RECT, PURPOSE_PIXEL = 0x44455048, 0x44455052, 0x44455058
ROW = 17
T_STD = float(np.sqrt(2.0 * (2 ** 32 - 1)))
U32 = 0xFFFFFFFF


def neutral_desc(**kw):
    d = dict(seed=0, n0=0.0, n1=0.0, n2=0.0, q=0.0, inv_q=0.0, lo=-np.inf, hi=np.inf, drop_thresh=0, hole_lo=0, hole_hi=0, hh_lo=1, hh_hi=1, hw_lo=1,
             hw_hi=1, hole_value=0.0, occluder_value=0.0, group=0)
    unknown = set(kw) - set(d)
    assert not unknown, unknown
    d.update(kw)
    return d


def sigma_to_n(*sigmas):
    """the host's conversion of standard-deviation coefficients to the kernel's: sigma / sqrt(2 (2^32 - 1)), in double"""
    return tuple(float(s) / T_STD for s in sigmas)


def _key(desc):
    seed = int(desc["seed"])
    return seed & U32, (seed >> 32) & U32


def num_streams(desc, B):
    return desc["group"] if desc["group"] > 0 else B


def frame_hw(shape):
    """(Hs, Ws) of (..., Hs, Ws, 1) or (..., 1, H, W); a trailing 1 decides for channels-last"""
    if len(shape) >= 4 and shape[-1] == 1:
        return shape[-3], shape[-2]
    assert len(shape) >= 4 and shape[-3] == 1, shape
    return shape[-2], shape[-1]


def _draw32(r, n):
    """a bounded draw whose range is taken modulo 2^32, as the kernel's unsigned arithmetic does (ranges are in [1, 2^31) for every
    descriptor the entry point checks; with hole_hi == 0 the rectangle bounds are unchecked and may be anything)"""
    if np.ndim(n) == 0:
        return draw(r, int(n) & U32)
    n = np.asarray(n, dtype=np.int64) & np.int64(U32)
    return ((np.asarray(r, dtype=np.uint64) * n.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)


def _wrap32(v):
    """int64 values as the int32 the kernel's table holds"""
    return (np.asarray(v, dtype=np.int64) & np.int64(U32)).astype(np.uint32).view(np.int32)


def stream_params(desc, G, Hs, Ws, step):
    """the draws of streams 0 .. G-1 at `step`: count (G,), and top, left, h, w (G, 4), int64"""
    g = np.arange(G, dtype=np.uint64)
    r = philox4x32((g, 0, step, PURPOSE_COUNT), _key(desc))
    p = {"count": desc["hole_lo"] + _draw32(r[0], desc["hole_hi"] - desc["hole_lo"] + 1)}
    cols = {k: [] for k in ("top", "left", "h", "w")}
    for j in range(4):
        r = philox4x32((g, j, step, PURPOSE_RECT), _key(desc))
        h = desc["hh_lo"] + _draw32(r[0], desc["hh_hi"] - desc["hh_lo"] + 1)
        w = desc["hw_lo"] + _draw32(r[1], desc["hw_hi"] - desc["hw_lo"] + 1)
        cols["h"].append(h)
        cols["w"].append(w)
        cols["top"].append(_draw32(r[2], Hs - h + 1))
        cols["left"].append(_draw32(r[3], Ws - w + 1))
    for k, v in cols.items():
        p[k] = np.stack(v, 1)
    return p


def params_table(desc, B, Hs, Ws, step):
    G = num_streams(desc, B)
    p = stream_params(desc, G, Hs, Ws, step)
    rects = np.stack([p[k] for k in ("top", "left", "h", "w")], 2).reshape(G, 16)      # per stream: 4 x (top, left, h, w)
    rows = np.concatenate([p["count"].reshape(G, 1), rects], 1)
    step32 = np.array([step & U32], dtype=np.uint32).view(np.int32)
    return np.concatenate([step32, _wrap32(rows.reshape(-1))])


def pixel_words(desc, B, Hs, Ws, step):
    pix = np.arange(Hs * Ws, dtype=np.uint64).reshape(1, Hs, Ws)
    fr = np.arange(B, dtype=np.uint64).reshape(B, 1, 1)
    return philox4x32((pix, fr, step, PURPOSE_PIXEL), _key(desc))


def noise_T(r):
    """T = 2 (h0 + .. + h5) - 6 * 65535 over the six 16-bit halves of r0, r1, r2"""
    m = np.uint64(0xFFFF)
    s = sum((w & m).astype(np.int64) + (w >> np.uint64(16)).astype(np.int64) for w in r[:3])
    return 2 * s - 6 * 65535


def augment(depth, desc, step, rgb_params=None):
    depth = np.asarray(depth)
    assert depth.dtype == np.float32
    Hs, Ws = frame_hw(depth.shape)
    d32 = np.ascontiguousarray(depth).reshape(-1, Hs, Ws)
    B = d32.shape[0]
    G = num_streams(desc, B)
    stream = np.arange(B) % G if desc["group"] > 0 else np.arange(B)
    n0, n1, n2, q, inv_q, lo, hi = (np.float64(desc[k]) for k in ("n0", "n1", "n2", "q", "inv_q", "lo", "hi"))
    noise = n0 != 0 or n1 != 0 or n2 != 0
    quant = q > 0
    clamp = not (lo == -np.inf and hi == np.inf)
    drop = int(desc["drop_thresh"]) != 0
    r = pixel_words(desc, B, Hs, Ws, step) if (noise or drop) else None
    bits = d32.view(np.uint32)
    out = bits.copy()
    if noise or quant or clamp:
        with np.errstate(all="ignore"):
            d = d32.astype(np.float64)
            v = d
            if noise:
                sd = (n0 + n1 * d) + (n2 * d) * d
                v = d + sd * noise_T(r).astype(np.float64)
            if quant:
                v = np.rint(v * inv_q) * q
            if clamp:
                v = np.where(v < lo, lo, v)
                v = np.where(v > hi, hi, v)
            staged = v.astype(np.float32).view(np.uint32)
        out = np.where(np.isfinite(d32), staged, bits)       # a non-finite input keeps its bit pattern
    hole_bits = np.array([desc["hole_value"]], dtype=np.float32).view(np.uint32)[0]
    occl_bits = np.array([desc["occluder_value"]], dtype=np.float32).view(np.uint32)[0]
    if drop:
        out = np.where(r[3] < np.uint64(desc["drop_thresh"]), hole_bits, out)
    y = np.arange(Hs).reshape(1, Hs, 1)
    x = np.arange(Ws).reshape(1, 1, Ws)
    if desc["hole_hi"] > 0:
        p = stream_params(desc, G, Hs, Ws, step)
        e = lambda name, j: p[name][stream, j].reshape(B, 1, 1)
        count = p["count"][stream].reshape(B, 1, 1)
        for j in range(4):
            inside = (j < count) & (y >= e("top", j)) & (y < e("top", j) + e("h", j)) & (x >= e("left", j)) & (x < e("left", j) + e("w", j))
            out = np.where(inside, hole_bits, out)
    if rgb_params is not None:
        t = np.asarray(rgb_params, dtype=np.int64)[1:1 + 8 * G].reshape(G, 8)[stream]           # qb qc qs erase top left h w
        e = lambda c: t[:, c].reshape(B, 1, 1)
        inside = (e(3) != 0) & (y >= e(4)) & (y < e(4) + e(6)) & (x >= e(5)) & (x < e(5) + e(7))
        out = np.where(inside, occl_bits, out)
    return out.astype(np.uint32).view(np.float32).reshape(depth.shape), params_table(desc, B, Hs, Ws, step)
