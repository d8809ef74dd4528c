"""Shared by tools/gen_visualize_golden.py and the visualisation tests: the two fixture configurations, their seeded weights with
pretrained-like BatchNorm statistics, the oracle's eval-mode maps, and a numpy restatement of the mosaic arithmetic."""
import math
import zlib

import numpy as np
import torch

from oracle import pose_oracle as po

LAYERS = ("f0", "f9", "f1", "f2", "f3", "f4", "a0", "d0")
# name -> (kind, cfg, weight seed, data seed).  `no` on ResNet-18 without proprioception is the one naive configuration the
# reference's visualize_layer runs as written; `tdo` on ResNet-50 is what its script shows (visuals/ of the reference).
VIS_CASES = {
    "no_r18": ("no", dict(latent_dim=64, hidden=[32, 16], use_depth=True, no_proprioception=True, depth=18), 81, 801),
    "tdo_r50": ("tdo", dict(latent_dim=64, hidden=32, use_depth=True, no_proprioception=False), 82, 802),
}
SAMPLE_STRIDE = 997
WHOLE_MAX = 128 * 1024   # maps of at most this many values are stored whole


def perturbed_state(kind, cfg, seed):
    """po.make_state with every BatchNorm's gamma in [0.25, 0.75], running_var in [0.5, 2] and running_mean ~ N(0, 0.5^2): the fold
    of an inference forward is then far from an identity, activations stay O(1) through 50 layers (gamma up to 3 drives a ResNet-50
    to 1e12) and dozens of channels die (constant maps), which the mosaic has to draw."""
    sd = po.make_state(kind, cfg, seed)
    for key in list(sd):
        if not key.endswith(".running_mean"):
            continue
        stem = key[:-len("running_mean")]
        for leaf in ("running_mean", "running_var", "weight"):
            k = stem + leaf
            g = torch.Generator().manual_seed((int(seed) * 7919 + zlib.crc32(("vis:" + k).encode())) % (2 ** 31 - 1))
            shape = sd[k].shape
            if leaf == "running_mean":
                sd[k] = torch.randn(shape, generator=g) * 0.5
            elif leaf == "running_var":
                sd[k] = 0.5 + 1.5 * torch.rand(shape, generator=g)
            else:
                sd[k] = 0.25 + 0.5 * torch.rand(shape, generator=g)
    return sd


def case_inputs(name):
    """(img (1,3,224,224), depth (1,1,224,224)) of a fixture case"""
    b = po.synth_batch((1,), VIS_CASES[name][3], with_depth=True)
    return b["img"], b["depth"]


def oracle_maps(kind, cfg, sd, img, depth, dtype=torch.float32):
    """The eight layers of the oracle's eval-mode forward for img (B,3,H,W) / depth (B,1,H,W), each (B, C, H, W) in `dtype`."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    fpre = "feature_net." if kind in ("n", "td") else "feature_net.module."
    with torch.no_grad():
        _, maps = po.resnet50_forward(sd, fpre, img.to(dtype), False, cfg.get("depth", 50))
        out = {"f%d" % k: v for k, v in maps.items()}
        k = po.hook_pools(9)
        if kind == "td":
            aw, ab, dw, db = sd["~aux_nets.0.0.weight"], sd["~aux_nets.0.0.bias"], sd["~depth_nets.0.%d.weight" % k], sd["~depth_nets.0.%d.bias" % k]
        else:
            aw, ab = sd["aux_nets.0.module.0.weight"], sd["aux_nets.0.module.0.bias"]
            dw, db = sd["depth_nets.0.module.%d.weight" % k], sd["depth_nets.0.module.%d.bias" % k]
        b = img.shape[0]
        a = po.aux_head(maps[9], aw, ab)
        side = int(math.isqrt(a.shape[1]))
        out["a0"] = a.view(b, 1, side, side)
        out["d0"] = po.depth_head(depth.to(dtype), dw, db, k).view(b, 1, side, side)
    return out


def finite_minmax(planes):
    """numpy (C,H,W) fp32 -> (C,2) fp32: each channel's range over finite values (+inf, -inf without one)"""
    c = planes.shape[0]
    out = np.empty((c, 2), np.float32)
    for i in range(c):
        v = planes[i][np.isfinite(planes[i])]
        out[i] = (v.min(), v.max()) if v.size else (np.inf, -np.inf)
    return out


def mosaic_t256(planes, minmax):
    """t * 256 of every pixel in fp32 (one correctly rounded operation each); nan where the pixel draws as index 0 by rule"""
    planes = np.asarray(planes, np.float32)
    lo, hi = minmax[:, 0].astype(np.float32)[:, None, None], minmax[:, 1].astype(np.float32)[:, None, None]
    with np.errstate(all="ignore"):
        t = ((planes - lo) / (hi - lo)).astype(np.float32) * np.float32(256.0)
    dead = ~np.isfinite(planes) | np.broadcast_to(hi == lo, planes.shape) | np.broadcast_to(~np.isfinite(hi - lo), planes.shape)
    return np.where(dead, np.float32(np.nan), t).astype(np.float32)


def mosaic_tiles(planes, minmax):
    """(C,H,W) uint8 colour indices: min(255, (int)(t * 256)), 0 for dead channels and non-finite pixels"""
    t = mosaic_t256(planes, minmax)
    with np.errstate(all="ignore"):
        idx = np.minimum(255, np.nan_to_num(t, nan=0.0).astype(np.int64))
    return idx.astype(np.uint8)


def mosaic(planes, minmax, cols, gutter, flip_y):
    """The whole index image: tile c at cell (c // cols, c % cols), pitch (H + gutter, W + gutter), everything else 0."""
    c, h, w = planes.shape
    rows = -(-c // cols)
    out = np.zeros((rows * (h + gutter) - gutter, cols * (w + gutter) - gutter), np.uint8)
    tiles = mosaic_tiles(planes, minmax)
    for i in range(c):
        r0, c0 = (i // cols) * (h + gutter), (i % cols) * (w + gutter)
        out[r0:r0 + h, c0:c0 + w] = tiles[i][::-1] if flip_y else tiles[i]
    return out


def grid_cols(c):
    return int(math.ceil(math.sqrt(c)))
