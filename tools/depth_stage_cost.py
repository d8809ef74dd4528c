"""Diagnostic (GPU box): what the device depth transform (ops.stage_depth -> rpe_stage_depth_f32_resized) costs for 256 raw fp32
depth frames, next to the host transform it replaces (ToPILImage -> Resize(256) -> CenterCrop(224) through Pillow, one frame at a
time on one thread; skipped when Pillow is not installed).

  256 x 256 frames : Resize(256) changes nothing -> the kernel is a crop copy
  512 x 512 frames : 2x downsample, 5 x 5 taps per output pixel

Kernel time: HIP events around `iters` back-to-back launches after warm-up, divided by `iters`.  GB/s: the bytes the algorithm
needs -- every source pixel the crop window's taps read, once, plus the output written -- over that time.

usage: python tools/depth_stage_cost.py [iterations]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgb_proprioceptive_pose_estimator_amd import ops  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.util.data_utils import crop_origin, pil_bilinear_tables_f64, resized_hw  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
B, CROP, SIZE = 256, (224, 224), 256


def needed_bytes(hs, ws):
    """source pixels inside the tap ranges of the crop window's rows and columns + output pixels, 4 bytes each, per batch"""
    hr, wr = resized_hw(hs, ws, SIZE)
    top, left = crop_origin(hr, wr, *CROP)
    span = []
    for i, o, first, n in ((hs, hr, top, CROP[0]), (ws, wr, left, CROP[1])):
        if i == o:
            span.append(n)
        else:
            b = pil_bilinear_tables_f64(i, o)[0]
            span.append(int(b[first + n - 1, 0] + b[first + n - 1, 1] - b[first, 0]))
    return 4 * B * (span[0] * span[1] + CROP[0] * CROP[1])


def host_transform_ms(frames):
    try:
        from PIL import Image
    except ImportError:
        return None
    hs, ws = frames.shape[1:3]
    hr, wr = resized_hw(hs, ws, SIZE)
    top, left = crop_origin(hr, wr, *CROP)
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    for f in frames:
        im = Image.fromarray(f[..., 0])                 # ToPILImage: float32 (H, W, 1) -> mode F
        if (hr, wr) != (hs, ws):
            im = im.resize((wr, hr), Image.BILINEAR)    # Resize(256)
        im = im.crop((left, top, left + CROP[1], top + CROP[0]))
        torch.from_numpy(np.asarray(im, dtype=np.float32).copy()).unsqueeze(0)   # ToTensor
    return (time.perf_counter() - t0) * 1e3


print("device: %s; %d frames per call, %d timed launches per figure" % (torch.cuda.get_device_name(0), B, iters))
for hw in (256, 512):
    rng = np.random.default_rng(hw)
    frames = (0.5 + 9.5 * rng.random((B, hw, hw, 1))).astype(np.float32)
    raw = torch.from_numpy(frames).cuda()
    for _ in range(5):
        ops.stage_depth(raw, CROP, SIZE)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        ops.stage_depth(raw, CROP, SIZE)
    stop.record()
    torch.cuda.synchronize()
    ms = start.elapsed_time(stop) / iters
    nbytes = needed_bytes(hw, hw)
    host = host_transform_ms(frames)
    print("depth %dx%d x%d -> %dx%d  kernel %8.4f ms  %7.1f MB needed  %7.1f GB/s   host Pillow transform, 1 thread: %s"
          % (hw, hw, B, CROP[0], CROP[1], ms, nbytes / 1e6, nbytes / ms / 1e6, "not measured (no Pillow)" if host is None else "%.1f ms" % host))
