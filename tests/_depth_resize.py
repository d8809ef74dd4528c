"""TEST CODE ONLY: numpy restatement of the depth transform the reference applies on the host (ToPILImage -> Resize(256) ->
CenterCrop(224) -> ToTensor on a float32 (H, W, 1) array), i.e. Pillow's mode-F bilinear resample (Resample.c: precompute_coeffs,
ImagingResampleHorizontal_32bpc, ImagingResampleVertical_32bpc) followed by torchvision's centre crop.  Written from Pillow's C,
scalar loop for the coefficients and tap-by-tap double accumulation for the passes; tests/golden/resize_pil_f32.npz (Pillow's own
output, tools/gen_depth_resize_golden.py) pins it bit for bit (tests/test_recorded_cpu.py)."""
import math

import numpy as np


def tables(in_size, out_size):
    """-> (bounds [out, 2] int32 = first tap, tap count; weights [out, ksize] float64)"""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 1.0 * filterscale                 # the triangle filter's support is 1
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.float64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        ww = 0.0
        ss = 1.0 / filterscale
        xmin = int(center - support + 0.5)      # C's (int): truncation
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) * ss)
            w = 1.0 - a if a < 1.0 else 0.0
            kk[xx, x] = w
            ww += w
        if ww != 0.0:
            for x in range(xmax):
                kk[xx, x] /= ww
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def resample_rows(img, bounds, kk):
    """one pass along the LAST axis of a float32 array: out[..., x] = (float32) sum_t (double) img[..., first + t] * k[x][t], the sum
    starting at 0.0 and taken in ascending tap order"""
    img = np.asarray(img, dtype=np.float32)
    first, count = bounds[:, 0].astype(np.int64), bounds[:, 1]
    acc = np.zeros(img.shape[:-1] + (bounds.shape[0],), dtype=np.float64)
    for t in range(kk.shape[1]):
        idx = np.minimum(first + t, img.shape[-1] - 1)
        prod = img[..., idx].astype(np.float64) * kk[:, t]
        acc = np.where(t < count, acc + prod, acc)
    return acc.astype(np.float32)


def resized_hw(h, w, size=256):
    """torchvision Resize(int): the shorter side becomes `size`"""
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        return int(size * h / w), size
    return size, int(size * w / h)


def resize(frames, hr, wr):
    """(..., Hs, Ws) float32 -> (..., hr, wr): horizontal pass first, its fp32 result feeds the vertical one; a pass whose size does
    not change is skipped, as in ImagingResample"""
    x = np.asarray(frames, dtype=np.float32)
    hs, ws = x.shape[-2:]
    if wr != ws:
        x = resample_rows(x, *tables(ws, wr))
    if hr != hs:
        x = np.swapaxes(resample_rows(np.swapaxes(x, -1, -2), *tables(hs, hr)), -1, -2)
    return np.ascontiguousarray(x)


def depth_transform(frames, crop=(224, 224), size=256):
    """(..., Hs, Ws) float32 raw depth -> (..., ch, cw) float32: Resize(size), CenterCrop(crop); ToTensor leaves floats as they are"""
    hs, ws = np.shape(frames)[-2:]
    hr, wr = resized_hw(hs, ws, size)
    ch, cw = crop
    top, left = int(round((hr - ch) / 2.0)), int(round((wr - cw) / 2.0))
    return np.ascontiguousarray(resize(frames, hr, wr)[..., top:top + ch, left:left + cw])
