"""Diagnostic (GPU box): what it costs to draw the measurement noise of one batch on the device -- poses only, no model, no optimiser.
Two forms, timed in ONE process, alternated block by block after a warm-up of both:

  (a) util.data_utils.MeasurementNoise -> rpe_measurement_noise: the two launches (parameter kernel + apply kernel) into a fixed buffer
  (b) torch's eager formulation on the device, what refresh_data computes on the host:
      x0bar = x0 + sigma * randn_like(x0); cat(x0bar[..., :3], x0bar[..., 3:] / x0bar[..., 3:].norm(dim=-1, keepdim=True))

at the shapes (1, 256, 7) -- a flat batch of 256 frames -- and (4, 64, 7) -- 64 windows of 4 timesteps.  (a) runs with one scale and
white noise, the only setting (b) has a counterpart for, and once more with three scales and correlation 0.9 (the AR(1) walk along S).
Blocks of `iters` back-to-back calls between HIP events.  Reported per form: the mean time of a call, the range of the block means,
and with --step_ms the share of one train step (`ms_per_step` of `bench.py --gpus 1` at batch 256 on the same box).

A record, not a bar: the feature buys fresh noise inside a captured step, not speed.  Writes profiles/measure_noise_cost.txt (or --out).

usage: python tools/measure_noise_cost.py [--step_ms MS] [--iters N] [--blocks N] [--out FILE]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgb_proprioceptive_pose_estimator_amd.util.data_utils import MeasurementNoise  # noqa: E402

SHAPES = [(1, 256, 7), (4, 64, 7)]
SCALE = 0.001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step_ms", type=float, default=None, help="ms_per_step of bench.py --gpus 1 (batch 256) on the same box")
    ap.add_argument("--iters", type=int, default=200, help="calls per timed block")
    ap.add_argument("--blocks", type=int, default=10, help="timed blocks per form, alternated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measure_noise_cost.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_noise_cost.py: no GPU visible; a CPU run measures nothing")
    dev = torch.device("cuda", 0)

    def events(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / args.iters

    lines = ["device: %s; measurement noise of one batch of poses, variance %g; %d blocks per form, alternated; %d calls per block%s"
             % (torch.cuda.get_device_name(0), SCALE, args.blocks, args.iters, "" if args.step_ms is None else "; step = %.3f ms (bench.py --gpus 1)" % args.step_ms)]
    for shape in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        x0 = torch.rand(shape, generator=g, device=dev)
        x0[..., 3:] /= x0[..., 3:].norm(dim=-1, keepdim=True)
        out = torch.empty_like(x0)
        white, coloured = MeasurementNoise(SCALE, seed=1), MeasurementNoise([SCALE, 10 * SCALE, 100 * SCALE], correlation=0.9, seed=1)
        sigma = SCALE ** 0.5

        def eager():
            x0bar = x0 + sigma * torch.randn_like(x0)
            return torch.cat([x0bar[..., :3], x0bar[..., 3:] / x0bar[..., 3:].norm(dim=-1, keepdim=True)], dim=-1)

        forms = [("(a)  rpe_measurement_noise, 2 launches", lambda: white(x0, out=out)),
                 ("(a') the same, 3 scales, correlation 0.9", lambda: coloured(x0, out=out)),
                 ("(b)  torch eager: randn_like, norm, divide, cat", eager)]
        for _ in range(3):
            for _, fn in forms:
                events(fn)
        # the two forms draw from the same distribution: noise of variance SCALE on the positions
        spread = (white(x0) - x0)[..., :3].std().item(), (eager() - x0)[..., :3].std().item()
        times = {name: [] for name, _ in forms}
        for _ in range(args.blocks):
            for name, fn in forms:
                times[name].append(events(fn))
        lines.append("shape %r (%d rows): position noise std (a) %.4f, (b) %.4f, asked %.4f" % (shape, x0.numel() // 7, spread[0], spread[1], sigma))
        mean = {}
        for name, _ in forms:
            t = times[name]
            mean[name] = sum(t) / len(t)
            share = "" if args.step_ms is None else "   = %6.3f %% of a step" % (100.0 * mean[name] / args.step_ms)
            lines.append("  %-48s %8.4f ms (%8.4f .. %8.4f)%s" % (name, mean[name], min(t), max(t), share))
        lines.append("  (a) / (b) = %.3f   (a') / (b) = %.3f" % (mean[forms[0][0]] / mean[forms[2][0]], mean[forms[1][0]] / mean[forms[2][0]]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
