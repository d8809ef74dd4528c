"""Diagnostic (GPU box): what the two launches that episodes of unequal length put in a step cost beside their dense counterparts.
Index tables and pose rows only -- no pixels, no model, no optimiser.  Timed in ONE process, alternated block by block after a warm-up
of all forms:

  (a)  rpe_sample_windows         1,000 selected episodes of 100 timesteps, N = 256 windows of one timestep, shuffled
  (b)  rpe_sample_windows_ragged  the same selection with lengths drawn from [1, 100]: the window table is scanned into LDS at every
                                  launch and every draw ends in a binary search over it
  (b') rpe_sample_windows_ragged  with every length = 100: the same table as (a), bit for bit
  (c)  rpe_pose_loss              2,560 rows (256 lanes x 10 timesteps), metric "combined", mode "pose", with the gradient
  (d)  rpe_pose_loss_masked       the same rows under a mask that keeps about 70 % of them
  (d') rpe_pose_loss_masked       under an all-ones mask: the same result as (c), bit for bit

Blocks of `iters` back-to-back calls between HIP events.  Reported per form: the mean time of a call and the range of the block means;
with --step_ms the share of one train step (`ms_per_step` of `bench.py --gpus 1` on the same box).  The dense train step issues none of
(b), (b'), (d), (d'): its launches are what they were.

A record, not a bar.  Writes profiles/ragged_cost.txt (or --out).

usage: python tools/ragged_cost.py [--step_ms MS] [--iters N] [--blocks N] [--out FILE]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgb_proprioceptive_pose_estimator_amd import ops  # noqa: E402

E, T, N, ROWS = 1000, 100, 256, 2560


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step_ms", type=float, default=None, help="ms_per_step of bench.py --gpus 1 on the same box")
    ap.add_argument("--iters", type=int, default=200, help="calls per timed block")
    ap.add_argument("--blocks", type=int, default=10, help="timed blocks per form, alternated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_cost.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ragged_cost.py: no GPU visible; a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    sel = torch.randperm(E, generator=g).to(torch.int32).to(dev)
    ragged = torch.randint(1, T + 1, (E,), generator=g).to(torch.int32).to(dev)
    full = torch.full((E,), T, dtype=torch.int32, device=dev)
    index = torch.zeros(1 + 2 * N, dtype=torch.int32, device=dev)
    states = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(3)]
    desc = ops.sample_desc(seed=1, E=E, T=T, S=1, stride=1, N=N, shuffle=1)
    pred = torch.randn(ROWS, 7, generator=g).to(dev)
    q = torch.randn(ROWS, 4, generator=g)
    truth = torch.cat([torch.randn(ROWS, 3, generator=g), q / q.norm(dim=-1, keepdim=True)], -1).to(dev)
    some = (torch.rand(ROWS, generator=g) < 0.7).to(torch.uint8).to(dev)
    ones = torch.ones(ROWS, dtype=torch.uint8, device=dev)
    loss = lambda valid: ops.pose_loss(pred, truth, 3, 1, 1.0, 0.5, 1e-4, valid=valid)

    # the forms that must agree do
    a, b = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2))
    assert torch.equal(ops.sample_windows(desc, sel, a), ops.sample_windows_ragged(desc, sel, full, b))
    assert all(torch.equal(x, y) for x, y in zip(loss(None), loss(ones)))

    def events(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / args.iters

    forms = [("(a)  sample_windows", lambda: ops.sample_windows(desc, sel, states[0], out=index)),
             ("(b)  sample_windows_ragged", lambda: ops.sample_windows_ragged(desc, sel, ragged, states[1], out=index)),
             ("(b') ... all lengths = T", lambda: ops.sample_windows_ragged(desc, sel, full, states[2], out=index)),
             ("(c)  pose_loss", lambda: loss(None)),
             ("(d)  pose_loss_masked, 70 % valid", lambda: loss(some)),
             ("(d') ... all valid", lambda: loss(ones))]
    for _ in range(3):
        for _, fn in forms:
            events(fn)
    times = {name: [] for name, _ in forms}
    for _ in range(args.blocks):
        for name, fn in forms:
            times[name].append(events(fn))
    lines = ["device: %s; index: %d selected episodes x %d timesteps, N = %d, S = 1, shuffled; loss: %d rows, combined / pose, with gradient; %d blocks per form, "
             "alternated; %d calls per block, issued from Python back to back (a call is a launch plus its wrapper)%s" % (
                 torch.cuda.get_device_name(0), E, T, N, ROWS, args.blocks, args.iters,
                 "" if args.step_ms is None else "; step = %.3f ms (bench.py --gpus 1)" % args.step_ms)]
    mean = {}
    for name, _ in forms:
        t = times[name]
        mean[name] = sum(t) / len(t)
        share = "" if args.step_ms is None else "   = %6.3f %% of a step" % (100.0 * mean[name] / args.step_ms)
        lines.append("%-36s %8.4f ms (%8.4f .. %8.4f)%s" % (name, mean[name], min(t), max(t), share))
    m = [mean[name] for name, _ in forms]
    lines.append("(b) / (a) = %.3f   (b') / (a) = %.3f   (d) / (c) = %.3f   (d') / (c) = %.3f" % (m[1] / m[0], m[2] / m[0], m[4] / m[3], m[5] / m[3]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
