"""Diagnostic (GPU box): what the training telemetry (FusedAdam(telemetry=K): rpe_param_stats + rpe_param_stats_finalize after the
update) costs per optimizer step over the parameter arena of the ResNet-50 `no` model, next to the torch formulation one would
otherwise write.  Variants over the same arena and the same random gradient, alternated block by block in one process:

  plain          rpe_adam_step per segment, the step count on the host                       (unchanged by the telemetry option)
  capturable     step bump + rpe_adam_step_amp per segment: telemetry OFF, the launches telemetry adds its two to
  telemetry=1    the capturable launches + the two telemetry launches, every step measured
  telemetry=50   the same launches, the device measures every 50th step (the other 49 return at the gate)
  pass alone     ops.param_stats by itself, every call measured: the time the GB/s figure is taken from
  torch          torch._foreach_norm over the gradient views, the same over the parameters, and a non-finite count per tensor
                 (torch.isfinite(g).logical_not().sum()), stacked on the device; no .tolist(), so no host synchronisation is timed.
                 Its time between the two events includes the gaps the device waits for the host to issue the next launch.

Time: HIP events around blocks of `block` back-to-back calls after a warm-up, `rounds` blocks per variant, the variants taking turns;
per call: the mean over all blocks and the spread (min .. max) of the block means.  GB/s of the pass: the 16 B per element it must
read (p, g, m, v once each) over the time of `pass alone`.

usage: python tools/telemetry_cost.py [output file, default profiles/telemetry_cost.txt] [rounds, default 10] [block, default 25]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgb_proprioceptive_pose_estimator_amd import ops  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.scripts.train_model import build_model, build_parser  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "telemetry_cost.txt")
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 10
block = int(sys.argv[3]) if len(sys.argv) > 3 else 25
assert rounds * block >= 200, "at least 200 timed calls per variant"

torch.cuda.set_device(0)
args = build_parser().parse_args(["--model", "no", "--obj_name", "cube"])
model = build_model(args, torch.bfloat16).cuda().train()
model._materialize(torch.device("cuda", 0))
arena = model._arena
segs = arena.trainable_segments()
n = sum(hi - lo for lo, hi in segs)
arena.grad.copy_(torch.randn(arena.numel, generator=torch.Generator().manual_seed(0)) * 0.1)

params = list(model.parameters())
opts = {"plain": FusedAdam(params, lr=1e-5), "capturable": FusedAdam(params, lr=1e-5, capturable=True),
        "telemetry=1": FusedAdam(params, lr=1e-5, capturable=True, telemetry=1),
        "telemetry=50": FusedAdam(params, lr=1e-5, capturable=True, telemetry=50)}
for opt in opts.values():      # warm-up: moments, state blocks, tables and partial rows exist, code objects are loaded
    for _ in range(5):
        opt.step()
tele = opts["telemetry=1"]
table, table_host, partials, out = tele._tele[1][0]
g0 = tele.param_groups[0]
grads, weights = [p._rpe_grad for p in params if p.requires_grad], [p.data for p in params if p.requires_grad]


def pass_alone():
    ops.param_stats(arena.flat, arena.grad, tele._m, tele._v, table, table_host, partials, out, g0["betas"][0], g0["betas"][1], g0["eps"], tele._dev_state, 1)


def torch_formulation():
    return (torch.stack(torch._foreach_norm(grads)), torch.stack(torch._foreach_norm(weights)),
            torch.stack([torch.isfinite(g).logical_not().sum() for g in grads]))


calls = [(name, opt.step) for name, opt in opts.items()] + [("pass alone", pass_alone), ("torch", torch_formulation)]
for _ in range(3):
    pass_alone(), torch_formulation()
torch.cuda.synchronize()
times = {name: [] for name, _ in calls}
for _ in range(rounds):
    for name, call in calls:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(block):
            call()
        stop.record()
        torch.cuda.synchronize()
        times[name].append(start.elapsed_time(stop) / block)

mean = {name: sum(t) / len(t) for name, t in times.items()}
rows = ops.param_stats_total_rows(table_host)
lines = ["device: %s; arena of %s: %d trainable elements in %d tensors (%d segment(s)), %d partial rows; %d blocks of %d calls per variant, alternated"
         % (torch.cuda.get_device_name(0), type(model).__name__, n, table_host.shape[0], len(segs), rows, rounds, block)]
for name, _ in calls:
    t = times[name]
    lines.append("%-13s %8.4f ms per call  (blocks %8.4f .. %8.4f)" % (name, mean[name], min(t), max(t))
                 + ("" if name in ("pass alone", "torch") else "  %+6.1f %% vs capturable  %+6.1f %% vs plain"
                    % (100.0 * (mean[name] / mean["capturable"] - 1.0), 100.0 * (mean[name] / mean["plain"] - 1.0))))
nbytes = 16 * n
lines.append("rpe_param_stats + finalize alone: %.4f ms for the %.3f GB they must read: %.1f GB/s" % (mean["pass alone"], nbytes / 1e9, nbytes / mean["pass alone"] / 1e6))
lines.append("telemetry=1 adds %.4f ms per step to the capturable step (%.4f ms), telemetry=50 adds %.4f ms; the torch formulation takes %.4f ms (%d launches' worth of host issue included)"
             % (mean["telemetry=1"] - mean["capturable"], mean["capturable"], mean["telemetry=50"] - mean["capturable"], mean["torch"], 2 + 3 * len(grads)))
lines.append("every=1 %s than the torch formulation" % ("costs MORE" if mean["pass alone"] > mean["torch"] else "costs less"))
stamp = tele.param_stats[:, 8]
lines.append("last measured step: stamp %d .. %d, global gradient norm %.6g, non-finite elements %d"
             % (stamp.min().item(), stamp.max().item(), tele.param_stats[:, 0].sum().sqrt().item(), tele.param_stats[:, [5, 7]].sum().item()))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
