"""numpy restatement of the device measurement noise (rpe_measurement_noise), written from its specification (DESIGN.md "Measurement
noise") and not from the kernel.  Everything is fp64 with one rounding to fp32 at the end; the kernel evaluates the same formulas
with another maths library, so it is compared within ONE fp32 ulp, and at most 1 element in 1000 may differ at all (`compare`).

    scale_picks(seed, n, num_scales, step)      -> (N,) int64: the scale index every lane draws
    normals(seed, rows, step)                   -> (len(rows), 7) fp64 standard normals of the rows r = s N + n
    unit_noise(seed, S, N, rho, step)           -> (S, N, 7) fp64: the AR(1) noise e along s, unit variance
    measure(x0, seed, scales, rho, step)        -> (out fp32 of x0's shape, picks int32 (1 + N,)); scales are VARIANCES
    compare(got, want)                          -> (elements beyond one ulp, elements that differ at all)
"""
import numpy as np

from _augment_oracle import philox4x32

PICK_PURPOSE = 0x4D45414B
DRAW_PURPOSE = 0x4D454153
TWO_M32 = 2.0 ** -32


def _key(seed):
    seed = int(seed)
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def scale_picks(seed, n, num_scales, step):
    if int(num_scales) == 1:
        return np.zeros(int(n), dtype=np.int64)      # no draw
    r0 = philox4x32((np.arange(int(n), dtype=np.uint64), 0, int(step) & 0xFFFFFFFF, PICK_PURPOSE), _key(seed))[0]
    return ((r0 * np.uint64(int(num_scales))) >> np.uint64(32)).astype(np.int64)


def uniforms(seed, rows, step):
    """(u1, u2), each (len(rows), 7) fp64: u1 in (0, 1), u2 in [0, 1)"""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    comp = np.arange(7, dtype=np.uint64).reshape(1, 7)
    r = philox4x32((rows, comp, int(step) & 0xFFFFFFFF, DRAW_PURPOSE), _key(seed))
    return (r[0].astype(np.float64) + 0.5) * TWO_M32, r[1].astype(np.float64) * TWO_M32


def normals(seed, rows, step):
    u1, u2 = uniforms(seed, rows, step)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def unit_noise(seed, s, n, rho, step):
    s, n, rho = int(s), int(n), float(rho)
    z = normals(seed, np.arange(s * n), step).reshape(s, n, 7)
    e = np.empty_like(z)
    e[0] = z[0]
    fresh = np.sqrt(1.0 - rho * rho)
    for t in range(1, s):
        e[t] = rho * e[t - 1] + fresh * z[t]
    return e


def measure(x0, seed, scales, rho, step):
    x0 = np.asarray(x0)
    assert x0.dtype == np.float32 and x0.shape[-1] == 7 and x0.ndim in (2, 3)
    s, n = (1, x0.shape[0]) if x0.ndim == 2 else x0.shape[:2]
    scales = [float(v) for v in scales]
    assert 1 <= len(scales) <= 8
    sigma = np.sqrt(np.asarray(scales, dtype=np.float64))
    k = scale_picks(seed, n, len(scales), step)
    e = unit_noise(seed, s, n, rho, step)
    v = x0.reshape(s, n, 7).astype(np.float64) + sigma[k].reshape(1, n, 1) * e
    q = v[..., 3:]
    norm = np.sqrt(q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2] + q[..., 3] * q[..., 3])
    with np.errstate(divide="ignore", invalid="ignore"):      # a zero norm yields what IEEE division yields
        out = np.concatenate([v[..., :3], q / norm[..., None]], -1).astype(np.float32).reshape(x0.shape)
    step32 = np.array([int(step) & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)
    return out, np.concatenate([step32, k.astype(np.int32)])


def compare(got, want):
    """-> (number of elements further than one fp32 ulp of the oracle's value, number of elements that differ at all)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    return int((diff > np.abs(np.spacing(want)).astype(np.float64)).sum()), int((got != want).sum())
