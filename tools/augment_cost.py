"""Diagnostic (GPU box): what the device frame augmentation (util.data_utils.FrameAugment -> rpe_augment_frames_u8) costs in front
of the staging of 256 recorded 256 x 256 uint8 frames (rpe_stage_frames_u8: centre crop to 224 x 224, normalise, NHWC4 in bf16) --
forward staging only, no model, no optimiser.

Every variant -- each feature alone, then all together -- is timed against the bare staging in ONE process: blocks of `iters`
back-to-back calls between HIP events, the two forms alternated block by block, after a warm-up of both.  Reported per variant: the
mean time of a call of each form, the range of the block means, the difference, and that difference as a share of one train step
(--step_ms: `ms_per_step` of `bench.py --gpus 1` at batch 256 with the augmentation off, measured on the same box).  The bytes the
augmentation needs: the frames read once and written once, read once more where the contrast mean is wanted.

A record, not a bar.  Writes profiles/augment_cost.txt (or --out).

usage: python tools/augment_cost.py --step_ms MS [--iters N] [--blocks N] [--out FILE]"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgb_proprioceptive_pose_estimator_amd import ops  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd._lib import RPE_BF16, lib  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.util.data_utils import IMAGENET_MEAN, IMAGENET_STD, FrameAugment  # noqa: E402

B, HS, H = 256, 256, 224
VARIANTS = [
    ("brightness", dict(brightness=0.3)),
    ("contrast", dict(contrast=0.3)),
    ("saturation", dict(saturation=0.3)),
    ("noise", dict(noise_std=4.0)),
    ("erase (mean fill)", dict(erase_prob=0.5)),
    ("erase (noise fill)", dict(erase_prob=0.5, erase_fill="noise")),
    ("all together", dict(brightness=0.3, contrast=0.3, saturation=0.3, noise_std=4.0, erase_prob=0.5, erase_fill="noise")),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step_ms", type=float, required=True, help="ms_per_step of bench.py --gpus 1 (batch 256) on the same box, augmentation off")
    ap.add_argument("--iters", type=int, default=20, help="calls per timed block")
    ap.add_argument("--blocks", type=int, default=10, help="timed blocks per form, alternated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_cost.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_cost.py: no GPU visible; a CPU run measures nothing")
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (B, HS, HS, 3), generator=g, dtype=torch.uint8).cuda()   # (recorded frames are this: raw uint8, channels last)
    x4 = torch.empty(lib.rpe_x4_bytes(RPE_BF16, B, H, H), dtype=torch.uint8, device="cuda")
    mean3, std3 = (ctypes.c_float * 3)(*IMAGENET_MEAN), (ctypes.c_float * 3)(*IMAGENET_STD)
    aug_out = torch.empty_like(frames)

    def stage(src):
        lib.rpe_stage_frames_u8(RPE_BF16, ops._p(src), ops._p(x4), B, HS, HS, H, H, mean3, std3, ops._stream())

    def block(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / args.iters

    lines = ["device: %s; %d uint8 frames of %dx%d staged to %dx%d bf16 NHWC4 per call; %d blocks of %d calls per form, alternated; step = %.3f ms "
             "(bench.py --gpus 1, augmentation off)" % (torch.cuda.get_device_name(0), B, HS, HS, H, H, args.blocks, args.iters, args.step_ms)]
    frame_mb = frames.numel() / 1e6
    for name, kw in VARIANTS:
        aug = FrameAugment(seed=1, **kw)
        bare = lambda: stage(frames)
        with_aug = lambda: stage(aug(frames, out=aug_out))
        for _ in range(3):
            bare(), with_aug()
        torch.cuda.synchronize()
        t = {"bare": [], "aug": []}
        for _ in range(args.blocks):
            t["bare"].append(block(bare))
            t["aug"].append(block(with_aug))
        mb, ma = sum(t["bare"]) / args.blocks, sum(t["aug"]) / args.blocks
        need_mb = frame_mb * (3 if "contrast" in kw else 2)
        d = ma - mb
        lines.append("%-20s staging %7.4f ms (%7.4f .. %7.4f)   augment + staging %7.4f ms (%7.4f .. %7.4f)   augmentation %+8.4f ms = %5.2f %% of a step   "
                     "%6.1f MB needed -> %7.1f GB/s" % (name, mb, min(t["bare"]), max(t["bare"]), ma, min(t["aug"]), max(t["aug"]), d, 100.0 * d / args.step_ms,
                                                      need_mb, need_mb / max(d, 1e-9)))   # MB / ms = GB/s
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
