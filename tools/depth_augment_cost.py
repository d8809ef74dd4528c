"""Diagnostic (GPU box): what the device depth augmentation (util.data_utils.DepthAugment -> rpe_augment_depth_f32, two launches)
costs in front of the staging of 256 recorded 256 x 256 fp32 depth frames (rpe_stage_depth_f32_resized through ops.stage_depth:
resize 256, centre crop to 224 x 224) -- forward staging only, no model, no optimiser.

Every variant -- each feature alone, then all together -- is timed in ONE process in three forms: the bare staging, the device
augmentation + staging, and a torch eager formulation of the same transforms + staging (`randn` for the noise, `round` for the
quantisation, `clamp`, a Bernoulli mask from `rand`, slice assignment for the rectangles; its rectangles are drawn on the host once,
outside the timing).  Blocks of `iters` back-to-back calls between HIP events, the three forms alternated block by block, after a
warm-up of all.  Reported per variant: the mean time of a call of each form, the range of the block means, the differences to the
bare staging, and the device augmentation as a share of one train step (--step_ms: `ms_per_step` of `bench.py --gpus 1` at batch 256
with the augmentation off, measured on the same box).  The bytes the augmentation needs: the frames read once and written once.

A record, not a bar.  Writes profiles/depth_augment_cost.txt (or --out).

usage: python tools/depth_augment_cost.py --step_ms MS [--iters N] [--blocks N] [--out FILE]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgb_proprioceptive_pose_estimator_amd import ops  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.util.data_utils import DepthAugment, FrameAugment  # noqa: E402

B, HS, H = 256, 256, 224
VARIANTS = [
    ("noise constant", dict(noise=(0.01,))),
    ("noise quadratic", dict(noise=(0.01, 0.01, 0.01))),
    ("quantisation", dict(quant=0.001)),
    ("clamp", dict(clamp=(0.6, 2.4))),
    ("dropout", dict(drop_prob=0.02)),
    ("holes", dict(holes=(1, 4))),
    ("shared occluder", dict(share=True)),
    ("all together", dict(noise=(0.01, 0.01, 0.01), quant=0.001, clamp=(0.6, 2.4), drop_prob=0.02, holes=(1, 4), share=True)),
]


def eager_form(kw, depth, gen):
    """the same transforms as one torch eager function of the depth batch -> a new tensor"""
    noise = tuple(kw.get("noise", ())) + (0.0,) * (3 - len(kw.get("noise", ())))
    rects = []
    if "holes" in kw or kw.get("share"):
        for _ in range((4 if "holes" in kw else 0) + (1 if kw.get("share") else 0)):
            h, w = (int(torch.randint(5, 39, (1,), generator=gen)) for _ in range(2))
            rects.append((int(torch.randint(0, HS - h + 1, (1,), generator=gen)), int(torch.randint(0, HS - w + 1, (1,), generator=gen)), h, w))

    def fn():
        v = depth
        if any(noise):
            v = v + (noise[0] + noise[1] * depth + noise[2] * depth * depth) * torch.randn_like(depth)
        if "quant" in kw:
            v = torch.round(v * (1.0 / kw["quant"])) * kw["quant"]
        if "clamp" in kw:
            v = v.clamp(*kw["clamp"])
        if v is depth:
            v = depth.clone()
        if "drop_prob" in kw:
            v.masked_fill_(torch.rand_like(depth) < kw["drop_prob"], 0.0)
        for top, left, h, w in rects:      # (one rectangle for the whole batch per slice assignment: cheaper than the per-frame draw it stands for)
            v[:, top:top + h, left:left + w] = 0.0
        return v
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step_ms", type=float, required=True, help="ms_per_step of bench.py --gpus 1 (batch 256) on the same box, augmentation off")
    ap.add_argument("--iters", type=int, default=20, help="calls per timed block")
    ap.add_argument("--blocks", type=int, default=10, help="timed blocks per form, alternated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_augment_cost.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("depth_augment_cost.py: no GPU visible; a CPU run measures nothing")
    g = torch.Generator().manual_seed(0)
    depth = (0.5 + 2.0 * torch.rand(B, HS, HS, 1, generator=g)).cuda()        # (recorded depth is this: raw fp32, channels last)
    frames = torch.randint(0, 256, (B, HS, HS, 3), generator=g, dtype=torch.uint8).cuda()
    aug_out = torch.empty_like(depth)

    def stage(src):
        return ops.stage_depth(src, (H, H), HS)

    def block(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / args.iters

    lines = ["device: %s; %d fp32 depth frames of %dx%d staged to %dx%d per call; %d blocks of %d calls per form, alternated; step = %.3f ms "
             "(bench.py --gpus 1, augmentation off)" % (torch.cuda.get_device_name(0), B, HS, HS, H, H, args.blocks, args.iters, args.step_ms)]
    need_mb = 2 * depth.numel() * 4 / 1e6
    for name, kw in VARIANTS:
        kw = dict(kw)
        share = kw.pop("share", False)
        rgb = None
        if share:
            rgb = FrameAugment(erase_prob=0.5, seed=1)
            rgb(frames)                                                         # the table of the batch, written once: the depth launch reads it
        aug = DepthAugment(seed=1, share_erase=rgb, **kw)
        eager = eager_form(dict(kw, share=share), depth.reshape(B, HS, HS), g)
        forms = {"bare": lambda: stage(depth), "aug": lambda: stage(aug(depth, out=aug_out)), "eager": lambda: stage(eager().reshape(B, HS, HS, 1))}
        for _ in range(3):
            for fn in forms.values():
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in forms}
        for _ in range(args.blocks):
            for k, fn in forms.items():
                t[k].append(block(fn))
        m = {k: sum(v) / args.blocks for k, v in t.items()}
        d, de = m["aug"] - m["bare"], m["eager"] - m["bare"]
        lines.append("%-16s staging %7.4f ms (%7.4f .. %7.4f)   augment + staging %7.4f ms (%7.4f .. %7.4f)   eager + staging %7.4f ms (%7.4f .. %7.4f)   "
                     "augmentation %+8.4f ms = %5.2f %% of a step (eager %+8.4f ms)   %6.1f MB needed -> %7.1f GB/s"
                     % (name, m["bare"], min(t["bare"]), max(t["bare"]), m["aug"], min(t["aug"]), max(t["aug"]), m["eager"], min(t["eager"]), max(t["eager"]),
                        d, 100.0 * d / args.step_ms, de, need_mb, need_mb / max(d, 1e-9)))   # MB / ms = GB/s
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
