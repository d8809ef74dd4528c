"""The box renderer of rendered episodes in numpy (DESIGN.md "Rendered episodes"): the specification a device kernel will have to
reproduce value for value.  float64 in a fixed order of operations, one numpy operation per rounding; vectorised over the pixels of a
frame, which changes nothing per pixel."""
import numpy as np

ID_PLANE, ID_SKY = 254, 255


def scene(P, near, far, bodies, plane=None, sky=(150, 180, 220), ss=1):
    """the numbers of a scene as a dict: Minv = M^-1 and centre = -Minv p4 of P = [M | p4] (numpy float64);
    bodies: list of (half (3,), six face colours); plane: None or (z0, s, colour, colour)"""
    P = np.asarray(P, dtype=np.float64)
    minv = np.linalg.inv(P[:, :3])
    return dict(Minv=minv, centre=-(minv @ P[:, 3]), near=np.float64(near), far=np.float64(far),
                bodies=[(np.asarray(h, dtype=np.float64), np.asarray(c, dtype=np.uint8).reshape(6, 3)) for h, c in bodies],
                plane=None if plane is None else (np.float64(plane[0]), np.float64(plane[1]), np.asarray(plane[2:], dtype=np.uint8).reshape(2, 3)),
                sky=np.asarray(sky, dtype=np.uint8), ss=int(ss))


def body_table(pose, centre):
    """-> (rows R e_i (3, 3), o (3,)) of one pose, or None for a body that is skipped"""
    p = np.asarray(pose, dtype=np.float32).astype(np.float64)
    x, (qx, qy, qz, qw) = p[:3], p[3:]
    with np.errstate(all="ignore"):
        n = np.sqrt(((qx * qx + qy * qy) + qz * qz) + qw * qw)
        if not (n > 0.0 and n < np.inf and np.isfinite(x).all()):
            return None
        a, b, c, d = qx / n, qy / n, qz / n, qw / n
    rows = np.array([[1.0 - 2.0 * (b * b + c * c), 2.0 * (a * b + c * d), 2.0 * (a * c - b * d)],
                     [2.0 * (a * b - c * d), 1.0 - 2.0 * (a * a + c * c), 2.0 * (b * c + a * d)],
                     [2.0 * (a * c + b * d), 2.0 * (b * c - a * d), 1.0 - 2.0 * (a * a + b * b)]], dtype=np.float64)
    e = centre - x
    o = np.array([(rows[i, 0] * e[0] + rows[i, 1] * e[1]) + rows[i, 2] * e[2] for i in range(3)], dtype=np.float64)
    return rows, o


def trace(sc, tables, u, v):
    """the rays through the stored positions (u, v) (arrays of one shape) -> (t float64, inf for the sky; rgb uint8 (..., 3); id uint8)"""
    M, c = sc["Minv"], sc["centre"]
    near, far = sc["near"], sc["far"]
    with np.errstate(all="ignore"):
        d = [(M[i, 0] * u + M[i, 1] * v) + M[i, 2] for i in range(3)]
        best = np.full(u.shape, np.inf)
        ids = np.full(u.shape, ID_SKY, dtype=np.uint8)
        rgb = np.empty(u.shape + (3,), dtype=np.uint8)
        rgb[...] = sc["sky"]
        for g, tab in enumerate(tables):
            if tab is None:
                continue
            rows, o = tab
            half, faces = sc["bodies"][g]
            tn, tf = np.full(u.shape, -np.inf), np.full(u.shape, np.inf)
            face = np.zeros(u.shape, dtype=np.int64)
            miss = np.zeros(u.shape, dtype=bool)
            for i in range(3):
                dd = (rows[i, 0] * d[0] + rows[i, 1] * d[1]) + rows[i, 2] * d[2]
                zero = dd == 0.0
                miss |= zero & (np.abs(o[i]) > half[i])
                t1, t2 = (-half[i] - o[i]) / dd, (half[i] - o[i]) / dd
                lo, hi = np.where(t1 < t2, t1, t2), np.where(t1 < t2, t2, t1)
                up = ~zero & (lo > tn)
                tn = np.where(up, lo, tn)
                face = np.where(up, 2 * i + np.where(dd > 0.0, 0, 1), face)
                tf = np.where(~zero & (hi < tf), hi, tf)
            hit = ~miss & (tn <= tf) & (near <= tn) & (tn <= far) & (tn < best)
            best = np.where(hit, tn, best)
            ids = np.where(hit, np.uint8(g), ids)
            rgb = np.where(hit[..., None], faces[face], rgb)
        if sc["plane"] is not None:
            z0, s, cols = sc["plane"]
            t = (z0 - c[2]) / d[2]
            hit = (d[2] != 0.0) & (near <= t) & (t <= far) & (t < best)
            ix = np.floor((c[0] + t * d[0]) / s)
            iy = np.floor((c[1] + t * d[1]) / s)
            par = (np.where(hit, ix, 0.0).astype(np.int64) + np.where(hit, iy, 0.0).astype(np.int64)) & 1
            best = np.where(hit, t, best)
            ids = np.where(hit, np.uint8(ID_PLANE), ids)
            rgb = np.where(hit[..., None], cols[par], rgb)
    return best, rgb, ids


def render(poses, sc, hs, ws):
    """poses (F, G, 7) float32 -> (frames (F, hs, ws, 3) uint8, depth (F, hs, ws) float32, ids (F, hs, ws) uint8)"""
    poses = np.asarray(poses, dtype=np.float32)
    F, G = poses.shape[:2]
    assert G == len(sc["bodies"]), (G, len(sc["bodies"]))
    y, x = np.mgrid[0:hs, 0:ws].astype(np.float64)
    near, far, ss = sc["near"], sc["far"], sc["ss"]
    offs = ((0.0, 0.0),) if ss == 1 else ((-0.25, -0.25), (0.25, -0.25), (-0.25, 0.25), (0.25, 0.25))
    frames = np.empty((F, hs, ws, 3), dtype=np.uint8)
    depth = np.empty((F, hs, ws), dtype=np.float32)
    ids = np.empty((F, hs, ws), dtype=np.uint8)
    for f in range(F):
        tables = [body_table(poses[f, g], sc["centre"]) for g in range(G)]
        acc = np.zeros((hs, ws, 3), dtype=np.int64)
        for ox, oy in offs:
            acc += trace(sc, tables, x + ox, y + oy)[1]
        frames[f] = (acc + (ss * ss) // 2) // (ss * ss)
        w, _, ids[f] = trace(sc, tables, x, y)
        with np.errstate(all="ignore"):
            z = (far * (w - near)) / (w * (far - near))
        depth[f] = np.where(ids[f] == ID_SKY, np.float32(1.0), z.astype(np.float32))
    return frames, depth, ids


def zbuffer(w, near, far):
    """the normalised z-buffer value of projective depth w, float64"""
    near, far = np.float64(near), np.float64(far)
    return (far * (np.asarray(w, dtype=np.float64) - near)) / (np.asarray(w, dtype=np.float64) * (far - near))
