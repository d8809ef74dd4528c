"""Diagnostic (GPU box): what the device frame blur (rpe_blur_frames_u8, the stage util.data_utils.FrameAugment puts in front of
rpe_augment_frames_u8) costs on 256 recorded 256 x 256 uint8 frames -- no model, no optimiser.

Every variant -- the three kinds alone (copy, Gaussian at several radii, motion at the shortest and at drawn lengths) and a drawn
mixture -- is timed in ONE process against
  (a) the bare staging of the same frames (rpe_stage_frames_u8: centre crop to 224 x 224, normalise, NHWC4 in bf16), which the
      pipeline runs anyway,
  (b) a plain device copy of the frame buffer (the floor by bytes: the frames read once and written once),
  (c) a torch formulation of the same blur: uint8 NHWC -> float NCHW, replicate padding, depthwise conv2d (two 1-D passes for the
      Gaussian, one 15 x 15 line kernel for the motion blur), round, back to uint8 NHWC,
in blocks of `iters` back-to-back calls between HIP events, the forms alternated block by block, after a warm-up of all of them.
Reported per variant: the mean time of a call of each form, the range of the block means, and the blur's time over (b) and under (c).
The blur launch does not advance the step counter, so every call of a variant draws the same numbers: a mixture stays that mixture.

A record, not a bar.  Writes profiles/blur_cost.txt (or --out).

usage: python tools/blur_cost.py [--iters N] [--blocks N] [--out FILE]"""
import argparse
import ctypes
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgb_proprioceptive_pose_estimator_amd import ops  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd._lib import RPE_BF16, lib  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.util.data_utils import IMAGENET_MEAN, IMAGENET_STD, FrameAugment, blur_directions, blur_gaussian_taps  # noqa: E402

B, HS, H = 256, 256, 224
FULL = 2 ** 32 - 1


def gauss_fields(sigma):
    r, w = blur_gaussian_taps(sigma)
    return dict(gauss_thresh=FULL, radius=[r], taps=[w])


def motion_fields(n_lengths):
    cx, cy = blur_directions()
    return dict(motion_thresh=FULL, n_lengths=n_lengths, dir_cx=cx, dir_cy=cy)


def variants():
    mixed = FrameAugment(blur_prob=1 / 3, motion_blur_prob=1 / 3, seed=1).blur_desc_fields()
    return [("copy (kind 0)", dict(seed=1), None),
            ("gaussian R = 2", dict(seed=1, **gauss_fields(0.5)), ("gauss", 0.5)),
            ("gaussian R = 6", dict(seed=1, **gauss_fields(2.0)), ("gauss", 2.0)),
            ("gaussian R = 8", dict(seed=1, **gauss_fields(4.0)), ("gauss", 4.0)),
            ("motion L = 3", dict(seed=1, **motion_fields(1)), ("motion", 3)),
            ("motion L = 3 .. 15", dict(seed=1, **motion_fields(7)), ("motion", 15)),
            ("mixed 1/3 1/3 1/3", mixed, ("mixed", 1.25, 9))]


def torch_gauss(x, sigma):
    """x float (B, 3, H, W) -> the separable Gaussian of blur_gaussian_taps(sigma)'s radius, replicate border"""
    r, w = blur_gaussian_taps(sigma)
    k = torch.tensor([w[abs(i)] for i in range(-r, r + 1)], dtype=torch.float32, device=x.device) / 2048.0
    x = F.conv2d(F.pad(x, (r, r, 0, 0), mode="replicate"), k.view(1, 1, 1, -1).expand(3, 1, 1, -1), groups=3)
    return F.conv2d(F.pad(x, (0, 0, r, r), mode="replicate"), k.view(1, 1, -1, 1).expand(3, 1, -1, 1), groups=3)


def torch_motion(x, length):
    """x float (B, 3, H, W) -> a linear motion blur of `length` along the diagonal as one depthwise 15 x 15 convolution"""
    k = torch.zeros((15, 15), dtype=torch.float32, device=x.device)
    for t in range(-(length - 1) // 2, (length - 1) // 2 + 1):
        d = (t * 181 + 128) >> 8
        k[7 + d, 7 + d] += 1.0 / length
    return F.conv2d(F.pad(x, (7, 7, 7, 7), mode="replicate"), k.view(1, 1, 15, 15).expand(3, 1, 15, 15), groups=3)


def torch_form(frames, what):
    """the torch formulation of one variant: uint8 NHWC in, uint8 NHWC out"""
    x = frames.permute(0, 3, 1, 2).float()
    if what[0] == "gauss":
        y = torch_gauss(x, what[1])
    elif what[0] == "motion":
        y = torch_motion(x, what[1])
    else:   # a third of the batch each way
        n = x.shape[0] // 3
        y = torch.cat([torch_gauss(x[:n], what[1]), torch_motion(x[n:2 * n], what[2]), x[2 * n:]])
    return (y + 0.5).floor().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="calls per timed block")
    ap.add_argument("--blocks", type=int, default=10, help="timed blocks per form, alternated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blur_cost.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("blur_cost.py: no GPU visible; a CPU run measures nothing")
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (B, HS, HS, 3), generator=g, dtype=torch.uint8).cuda()   # (recorded frames are this: raw uint8, channels last)
    x4 = torch.empty(lib.rpe_x4_bytes(RPE_BF16, B, H, H), dtype=torch.uint8, device="cuda")
    mean3, std3 = (ctypes.c_float * 3)(*IMAGENET_MEAN), (ctypes.c_float * 3)(*IMAGENET_STD)
    out = torch.empty_like(frames)
    state = torch.zeros(1, dtype=torch.int32, device="cuda")
    params = torch.empty(1 + 4 * B, dtype=torch.int32, device="cuda")

    def stage():
        lib.rpe_stage_frames_u8(RPE_BF16, ops._p(frames), ops._p(x4), B, HS, HS, H, H, mean3, std3, ops._stream())

    def copy():
        out.copy_(frames)

    def block(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / args.iters

    frame_mb = frames.numel() / 1e6
    lines = ["device: %s; %d uint8 frames of %dx%d (%.1f MB, read once and written once = %.1f MB); %d blocks of %d calls per form, alternated"
             % (torch.cuda.get_device_name(0), B, HS, HS, frame_mb, 2 * frame_mb, args.blocks, args.iters)]
    for name, fields, what in variants():
        desc = ops.blur_desc(**fields)
        forms = {"blur": lambda: ops.blur_frames_u8(frames, desc, state, out=out, params=params), "stage": stage, "copy": copy}
        if what is not None:
            forms["torch"] = lambda: torch_form(frames, what)
        for _ in range(3):
            for fn in forms.values():
                fn()
        torch.cuda.synchronize()
        kinds = params[1::4].cpu().tolist()
        t = {k: [] for k in forms}
        for _ in range(args.blocks):
            for k, fn in forms.items():
                t[k].append(block(fn))
        mean = {k: sum(v) / len(v) for k, v in t.items()}
        cell = lambda k: "%s %7.4f ms (%7.4f .. %7.4f)" % (k, mean[k], min(t[k]), max(t[k]))
        line = "%-20s kinds 0/1/2 = %3d/%3d/%3d   %s   (a) %s   (b) %s   blur / (b) = %5.2f   %6.1f GB/s of the %.1f MB" % (
            name, kinds.count(0), kinds.count(1), kinds.count(2), cell("blur"), cell("stage"), cell("copy"), mean["blur"] / mean["copy"],
            2 * frame_mb / mean["blur"], 2 * frame_mb)
        if what is not None:
            line += "   (c) %s   (c) / blur = %5.1f" % (cell("torch"), mean["torch"] / mean["blur"])
        lines.append(line)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
