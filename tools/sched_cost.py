"""Diagnostic (GPU box): what the on-device learning-rate schedule, the weight average and a second param group add to
FusedAdam.step() ALONE over the parameter arena of the default ResNet-50 `tdo_v2` model.  Four optimizers over the same arena and the
same random gradient, alternated in one process:

  plain           step bump + rpe_adam_step_amp per segment (capturable: what a captured train step replays today)
  scheduled       step bump + rpe_lr_schedule + rpe_adamw_step_sched per segment
  scheduled+ema   the same launches with the average written by the update kernel (8 B per element more: ema read and written)
  two groups      scheduled, the trunk as a param group of its own at lr x 0.1 (util.model_utils.lr_param_groups): one update launch
                  per group segment

Time: HIP events around blocks of `block` back-to-back steps after a warm-up, `rounds` blocks per variant, the variants taking
turns block by block; per step: the mean over all blocks and the spread (min .. max) of the block means.  GB/s: the bytes the
update needs (p, m, v read and written, g read: 28 B per element; with the average 36 B) over that time.

usage: python tools/sched_cost.py [output file, default profiles/sched_cost.txt] [rounds, default 10] [block, default 25]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam, LRSchedule  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.scripts.train_model import build_model, build_parser  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.util.model_utils import lr_param_groups  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sched_cost.txt")
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
schedule = lambda: LRSchedule("cosine", warmup_steps=100, total_steps=100000, min_factor=0.01)
groups = [dict({k: v for k, v in g.items() if k != "lr_scale"}, lr=1e-5 * g.get("lr_scale", 1.0)) for g in lr_param_groups(model, 0.1)]
variants = [
    ("plain", FusedAdam(params, lr=1e-5, capturable=True), 28),
    ("scheduled", FusedAdam(params, lr=1e-5, lr_schedule=schedule()), 28),
    ("scheduled+ema", FusedAdam(params, lr=1e-5, lr_schedule=schedule(), ema_decay=0.999), 36),
    ("two groups", FusedAdam(groups, lr=1e-5, lr_schedule=schedule()), 28),
]
for _, opt, _ in variants:      # warm-up: moments, average, state and schedule blocks exist, code objects are loaded
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

two = variants[3][1]
launches = sum(len(s) for _, s in two._groups(arena))
lines = ["device: %s; FusedAdam.step() alone, arena of %s: %d trainable elements in %d segment(s) (two groups: %d update launches); "
         "%d blocks of %d steps per variant, alternated" % (torch.cuda.get_device_name(0), type(model).__name__, n, len(segs), launches, rounds, block)]
base = sum(times["plain"]) / rounds
for name, _, nbytes in variants:
    t = times[name]
    mean = sum(t) / len(t)
    lines.append("%-14s %8.4f ms per step  (blocks %8.4f .. %8.4f)  %7.1f GB/s of the %d B per element it needs  x%.3f of plain"
                 % (name, mean, min(t), max(t), nbytes * n / mean / 1e6, nbytes, mean / base))
sched = variants[1][1]
lines.append("last scheduled step: e = %d, factor %.6g" % (int(sched.steps_scheduled.item()), sched.lr_factor.item()))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
