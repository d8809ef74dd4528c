"""The pose overlay restated in numpy: what csrc/overlay.hip must compute, value for value (DESIGN.md "Pose overlay",
include/rpe_hip.h).  Projection in float64 with the header's order of operations; drawing in int64, with the int64 bound of every
product asserted where it is formed."""
import numpy as np

INVALID = -2 ** 31
NEAR = 2.0 ** -10
CLAMP_Q4 = 2 ** 17
AXIS_Q4 = 2 ** 13
MAX_RADIUS_Q4 = 256
SUB = ((-4, -4), (4, -4), (-4, 4), (4, 4))      # subsample s: bit 0 picks x, bit 1 picks y

# the extreme values behind the capsule's box test, and the products they allow (asserted in `capsule_cover`)
V_MAX = AXIS_Q4 + MAX_RADIUS_Q4 + 8
DOT_MAX = 2 * AXIS_Q4 * V_MAX
INT64_MAX = 2 ** 63 - 1


def style(rgb=(255, 255, 255), alpha_q8=256, r_q4=64, hw_q4=24, axis_rgb=((255, 0, 0), (0, 255, 0), (0, 0, 255)), trail=0, trail_r_q4=32):
    return dict(rgb=tuple(rgb), alpha_q8=int(alpha_q8), r_q4=int(r_q4), hw_q4=int(hw_q4), axis_rgb=tuple(tuple(c) for c in axis_rgb), trail=int(trail),
                trail_r_q4=int(trail_r_q4))


# ---------------------------------------------------------------------------------------------------------------- projection
def _hom(P, X):
    """rows of P (3, 4) applied to X (3,), ((P0 x + P1 y) + P2 z) + P3, float64"""
    return [((P[r, 0] * X[0] + P[r, 1] * X[1]) + P[r, 2] * X[2]) + P[r, 3] for r in range(3)]


def project_point(P, X, detail=None):
    """-> (u_q4, v_q4) or (INVALID, INVALID).  detail: a list that receives (16 u + 0.5, 16 v + 0.5, w) for the generator's screening"""
    with np.errstate(all="ignore"):
        uw, vw, w = _hom(P, X)
        if detail is not None:
            detail.append((16.0 * (uw / w) + 0.5, 16.0 * (vw / w) + 0.5, w))
        if not (np.isfinite(uw) and np.isfinite(vw) and np.isfinite(w)) or not (w > NEAR):
            return INVALID, INVALID
        a, b = np.floor(16.0 * (uw / w) + 0.5), np.floor(16.0 * (vw / w) + 0.5)
    return int(min(max(a, -CLAMP_Q4), CLAMP_Q4)), int(min(max(b, -CLAMP_Q4), CLAMP_Q4))


def bar_length(err, full, width, detail=None):
    with np.errstate(all="ignore"):
        v = (np.float64(err) / np.float64(full)) * np.float64(width)
    if detail is not None:
        detail.append(v)
    if np.isnan(v):
        return 0
    return int(min(max(np.floor(v), 0.0), float(width)))


def project_poses(poses, cam, cam_index, axis_len, pos_err=None, ori_err=None, pos_full=0.1, ori_full=0.5, width=0, detail=None):
    """poses (F, G, 7) float32, cam (C, 3, 4) float64, cam_index (F,) -> (points (F, G, 4, 2) int32, bars (F, 2) int32).  detail: a list
    that receives, per frame, the list of every (16 u + 0.5, 16 v + 0.5, w) and bar value computed for it."""
    poses = np.asarray(poses, dtype=np.float32)
    cam = np.asarray(cam, dtype=np.float64).reshape(-1, 3, 4)
    F, G = poses.shape[:2]
    points = np.full((F, G, 4, 2), INVALID, dtype=np.int64)
    bars = np.zeros((F, 2), dtype=np.int64)
    axis_len = np.float64(axis_len)
    for f in range(F):
        pts, barv = [], []
        if pos_err is not None:
            bars[f] = bar_length(pos_err[f], pos_full, width, barv), bar_length(ori_err[f], ori_full, width, barv)
        ci = int(cam_index[f])
        if 0 <= ci < len(cam):
            P = cam[ci]
            for g in range(G):
                p = poses[f, g].astype(np.float64)
                X, (qx, qy, qz, qw) = p[:3], p[3:]
                c = project_point(P, X, pts)
                points[f, g, 0] = c
                with np.errstate(all="ignore"):
                    n = np.sqrt(((qx * qx + qy * qy) + qz * qz) + qw * qw)
                    if c[0] == INVALID or not (n > 0.0 and n < np.inf):
                        continue
                    a, b, cc, d = qx / n, qy / n, qz / n, qw / n
                    cols = ((1.0 - 2.0 * (b * b + cc * cc), 2.0 * (a * b + cc * d), 2.0 * (a * cc - b * d)),
                            (2.0 * (a * b - cc * d), 1.0 - 2.0 * (a * a + cc * cc), 2.0 * (b * cc + a * d)),
                            (2.0 * (a * cc + b * d), 2.0 * (b * cc - a * d), 1.0 - 2.0 * (a * a + b * b)))
                    for k in range(3):
                        t = project_point(P, [X[0] + axis_len * cols[k][0], X[1] + axis_len * cols[k][1], X[2] + axis_len * cols[k][2]], pts)
                        if t[0] != INVALID and (abs(t[0] - c[0]) > AXIS_Q4 or abs(t[1] - c[1]) > AXIS_Q4):
                            t = (INVALID, INVALID)
                        points[f, g, 1 + k] = t
        if detail is not None:
            detail.append((pts, barv))
    return points.astype(np.int32), bars.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- drawing
def point_ok(u, v):
    return u != INVALID and v != INVALID and abs(u) <= CLAMP_Q4 and abs(v) <= CLAMP_Q4


def axis_ok(cu, cv, tu, tv):
    return point_ok(cu, cv) and point_ok(tu, tv) and abs(tu - cu) <= AXIS_Q4 and abs(tv - cv) <= AXIS_Q4


def _grid(hs, ws):
    y, x = np.mgrid[0:hs, 0:ws].astype(np.int64)
    return 16 * x, 16 * y


def disc_mask(hs, ws, cu, cv, r):
    """(hs, ws) int64: bit s set where subsample s of the pixel lies inside the disc"""
    sx, sy = _grid(hs, ws)
    m = np.zeros((hs, ws), dtype=np.int64)
    for s, (ox, oy) in enumerate(SUB):
        dx, dy = sx + ox - int(cu), sy + oy - int(cv)
        m |= (dx * dx + dy * dy <= int(r) * int(r)).astype(np.int64) << s
    return m


def popcount4(m):
    return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1)


def disc_cover(hs, ws, cu, cv, r):
    return popcount4(disc_mask(hs, ws, cu, cv, r))


def capsule_cover(hs, ws, cu, cv, tu, tv, hw):
    """(hs, ws) int64 coverage 0..4 of the capsule from (cu, cv) to (tu, tv), half-width hw; only pixels behind the box test are
    evaluated, which is what keeps every product inside int64 (asserted)"""
    cu, cv, tu, tv, hw = int(cu), int(cv), int(tu), int(tv), int(hw)
    sx, sy = _grid(hs, ws)
    box = (sx + 4 >= min(cu, tu) - hw) & (sx - 4 <= max(cu, tu) + hw) & (sy + 4 >= min(cv, tv) - hw) & (sy - 4 <= max(cv, tv) + hw)
    ex, ey = tu - cu, tv - cv
    L, hh = ex * ex + ey * ey, hw * hw
    assert abs(ex) <= AXIS_Q4 and abs(ey) <= AXIS_Q4 and 0 <= hw <= MAX_RADIUS_Q4
    assert DOT_MAX < 2 ** 28 and DOT_MAX * DOT_MAX < 2 ** 56 < INT64_MAX and hh * L <= 2 ** 43
    cov = np.zeros((hs, ws), dtype=np.int64)
    for ox, oy in SUB:
        vx, vy = (sx + ox - cu)[box], (sy + oy - cv)[box]
        if vx.size:
            assert np.abs(vx).max() <= V_MAX and np.abs(vy).max() <= V_MAX
        t = vx * ex + vy * ey
        x = vx * ey - vy * ex
        if t.size:
            assert np.abs(t).max() <= DOT_MAX and np.abs(x).max() <= DOT_MAX
        inside = np.where(t <= 0, vx * vx + vy * vy <= hh, np.where(t >= L, (vx - ex) ** 2 + (vy - ey) ** 2 <= hh, x * x <= hh * L))
        cov[box] += inside.astype(np.int64)
    return cov


def blend(img, colour, w):
    """img (hs, ws, 3) int64 in place: (px (1024 - w) + colour w + 512) >> 10 with w (hs, ws) in [0, 1024]"""
    w = w[..., None]
    img[...] = (img * (1024 - w) + np.asarray(colour, dtype=np.int64) * w + 512) >> 10


def draw_poses(frames, points, bars, styles, frames_per_episode=1, first=0, bar_px=0, bar_rgb=((255, 255, 255), (255, 255, 255)), flip=False):
    """frames (n, hs, ws, 3) uint8; points (F, G, 4, 2), bars (F, 2) with F >= first + n; styles: G dicts of `style` -> uint8 like frames"""
    frames = np.asarray(frames)
    n, hs, ws, _ = frames.shape
    points, bars = np.asarray(points, dtype=np.int64), np.asarray(bars, dtype=np.int64)
    G = points.shape[1]
    assert len(styles) == G and frames.dtype == np.uint8
    out = np.empty_like(frames)
    for i in range(n):
        gf = first + i
        t = gf % frames_per_episode
        img = frames[i].astype(np.int64)
        for g, st in enumerate(styles):           # the trails, under everything else
            m = np.zeros((hs, ws), dtype=np.int64)
            for k in range(1, min(st["trail"], t) + 1):
                u, v = points[gf - k, g, 0]
                if point_ok(u, v):
                    m |= disc_mask(hs, ws, u, v, st["trail_r_q4"])
            blend(img, st["rgb"], popcount4(m) * (st["alpha_q8"] >> 1))
        for g, st in enumerate(styles):
            cu, cv = points[gf, g, 0]
            for k in range(3):
                tu, tv = points[gf, g, 1 + k]
                if axis_ok(cu, cv, tu, tv):
                    blend(img, st["axis_rgb"][k], capsule_cover(hs, ws, cu, cv, tu, tv, st["hw_q4"]) * st["alpha_q8"])
            if point_ok(cu, cv):
                blend(img, st["rgb"], disc_cover(hs, ws, cu, cv, st["r_q4"]) * st["alpha_q8"])
        if flip:
            img = img[::-1].copy()
        if bar_px > 0:                             # (in output rows: after the flip)
            x = np.arange(ws)
            for band in range(2):
                rows = slice(hs - 2 * bar_px + band * bar_px, hs - bar_px + band * bar_px)
                on = (x < bars[gf, band])[None, :, None]
                img[rows] = np.where(on, np.asarray(bar_rgb[band], dtype=np.int64), img[rows] >> 1)
        assert img.min() >= 0 and img.max() <= 255
        out[i] = img.astype(np.uint8)
    return out


def flip_camera_rows(P, hs):
    """the matrix whose row coordinate is hs - 1 - v: row 1 becomes (hs - 1) row 2 - row 1"""
    P = np.array(P, dtype=np.float64)
    P[..., 1, :] = (hs - 1) * P[..., 2, :] - P[..., 1, :]
    return P
