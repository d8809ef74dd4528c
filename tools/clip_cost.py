"""Diagnostic (GPU box): what FusedAdam.step() costs ALONE over the parameter arena of the default ResNet-50 `tdo_v2` model, with and
without the on-device gradient-norm clip and the decoupled weight decay.  Four optimizers over the same arena and the same random
gradient, alternated in one process:

  plain        rpe_adam_step per segment, the step count on the host
  capturable   step bump + rpe_adam_step_amp per segment (what a captured train step replays)
  clip         step bump + rpe_grad_sumsq per segment + rpe_clip_coef + rpe_adamw_step_clip per segment
  clip+decay   the same launches with weight_decay = 1e-2

Time: HIP events around blocks of `block` back-to-back steps after a warm-up, `rounds` blocks per variant, the variants taking
turns block by block; per step: the mean over all blocks and the spread (min .. max) of the block means.  GB/s: the bytes the
update needs (p, m, v read and written, g read: 28 B per element; the norm pass reads g once more: 32 B) over that time.

usage: python tools/clip_cost.py [output file, default profiles/clip_cost.txt] [rounds, default 10] [block, default 25]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam, FusedAdamW  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.scripts.train_model import build_model, build_parser  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "clip_cost.txt")
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 10
block = int(sys.argv[3]) if len(sys.argv) > 3 else 25
assert rounds * block >= 200, "at least 200 timed steps per variant"

torch.cuda.set_device(0)
args = build_parser().parse_args(["--model", "tdo_v2", "--obj_name", "cube"])
model = build_model(args, torch.bfloat16).cuda().train()
model._materialize(torch.device("cuda", 0))
arena = model._arena
segs = arena.trainable_segments()
n = sum(hi - lo for lo, hi in segs)
arena.grad.copy_(torch.randn(arena.numel, generator=torch.Generator().manual_seed(0)) * 0.1)

params = list(model.parameters())
variants = [
    ("plain", FusedAdam(params, lr=1e-5), 28),
    ("capturable", FusedAdam(params, lr=1e-5, capturable=True), 28),
    ("clip", FusedAdam(params, lr=1e-5, max_grad_norm=1.0), 32),
    ("clip+decay", FusedAdamW(params, lr=1e-5, weight_decay=1e-2, max_grad_norm=1.0), 32),
]
for _, opt, _ in variants:      # warm-up: moments, state blocks and the partials buffer exist, code objects are loaded
    for _ in range(5):
        opt.step()
torch.cuda.synchronize()
times = {name: [] for name, _, _ in variants}
for _ in range(rounds):
    for name, opt, _ in variants:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(block):
            opt.step()
        stop.record()
        torch.cuda.synchronize()
        times[name].append(start.elapsed_time(stop) / block)

lines = ["device: %s; FusedAdam.step() alone, arena of %s: %d trainable elements in %d segment(s); %d blocks of %d steps per variant, alternated"
         % (torch.cuda.get_device_name(0), type(model).__name__, n, len(segs), rounds, block)]
base = sum(times["capturable"]) / rounds
for name, _, nbytes in variants:
    t = times[name]
    mean = sum(t) / len(t)
    lines.append("%-11s %8.4f ms per step  (blocks %8.4f .. %8.4f)  %7.1f GB/s of the %d B per element it needs  %+6.1f %% vs capturable"
                 % (name, mean, min(t), max(t), nbytes * n / mean / 1e6, nbytes, 100.0 * (mean / base - 1.0)))
clip = variants[2][1]
lines.append("last clipped step: gradient norm %.6g, coefficient %.6g" % (clip.grad_norm.item(), clip.clip_coef.item()))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
