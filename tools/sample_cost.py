"""Diagnostic (GPU box): what it costs to put one shuffled minibatch of recorded frames in front of the augmentation / staging kernels --
256 windows of one 256 x 256 x 3 uint8 frame drawn from a pool of 20 episodes x 100 timesteps (2,000 frames, 393 MB) resident in HBM.
Frames only, no model, no optimiser.  Four forms, timed in ONE process, alternated block by block after a warm-up of all of them:

  (a)  the sampler's two launches: rpe_sample_windows + rpe_gather_rows (ops.sample_windows, ops.gather_rows into a fixed buffer)
  (a') the gather launch alone, on a fixed index -- its bytes (the batch read once and written once) over its time is the achieved GB/s
  (b)  torch advanced indexing pool[e, t] with device index tensors (the index is given: drawing it is not timed)
  (c)  what the lockstep path does for a batch of this size: the batch lies assembled in pageable host memory and goes through
       util.data_utils.FramePrefetcher -- the memcpy into the pinned buffer on the calling thread, then PCIe (double buffered:
       the time per batch of a stream of batches, host clock around the loop and a device synchronise)

(a), (a'), (b): blocks of `iters` back-to-back calls between HIP events.  Reported per form: the mean time of a call, the range of the
block means, and with --step_ms the share of one train step (`ms_per_step` of `bench.py --gpus 1` at batch 256 on the same box).

A record, not a bar.  Writes profiles/sample_cost.txt (or --out).

usage: python tools/sample_cost.py [--step_ms MS] [--iters N] [--blocks N] [--out FILE]"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgb_proprioceptive_pose_estimator_amd import ops  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.util.data_utils import FramePrefetcher  # noqa: E402

E, T, N, HS = 20, 100, 256, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step_ms", type=float, default=None, help="ms_per_step of bench.py --gpus 1 (batch 256) on the same box")
    ap.add_argument("--iters", type=int, default=50, help="calls per timed block of the device forms")
    ap.add_argument("--host_iters", type=int, default=6, help="batches per timed block of the host form")
    ap.add_argument("--blocks", type=int, default=10, help="timed blocks per form, alternated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_cost.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_cost.py: no GPU visible; a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    pool = torch.randint(0, 256, (E, T, HS, HS, 3), generator=g, dtype=torch.uint8, device=dev)      # (recorded frames are this: raw uint8, channels last)
    sel = torch.arange(E, dtype=torch.int32, device=dev)
    state = torch.zeros(1, dtype=torch.int32, device=dev)
    index = torch.zeros(1 + 2 * N, dtype=torch.int32, device=dev)
    out = torch.empty((1, N, HS, HS, 3), dtype=torch.uint8, device=dev)
    desc = ops.sample_desc(seed=1, E=E, T=T, S=1, stride=1, N=N, shuffle=1)
    host_batch = torch.randint(0, 256, (1, N, HS, HS, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)   # pageable

    def sample_and_gather():
        ops.sample_windows(desc, sel, state, out=index)
        ops.gather_rows(pool, index, 1, T, out=out)

    def gather_only():
        ops.gather_rows(pool, index, 1, T, out=out)

    sample_and_gather()
    ep, t0 = index[1::2].long(), index[2::2].long()      # one batch's index as torch wants it

    def torch_index():
        return pool[ep, t0]

    def events(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / args.iters

    prefetcher = FramePrefetcher(None, dev)

    def host_stream():
        prefetcher.batches = ((host_batch,) for _ in range(args.host_iters))
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _batch in prefetcher:
            pass
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / args.host_iters

    forms = [("(a)  sample + gather, 2 launches", lambda: events(sample_and_gather)), ("(a') gather launch alone", lambda: events(gather_only)),
             ("(b)  torch pool[e, t]", lambda: events(torch_index)), ("(c)  FramePrefetcher from host", host_stream)]
    assert torch.equal(out[0], torch_index())      # the forms move the same bytes
    for _ in range(3):
        for _, run in forms:
            run()
    times = {name: [] for name, _ in forms}
    for _ in range(args.blocks):
        for name, run in forms:
            times[name].append(run())
    batch_mb = out.numel() / 1e6
    lines = ["device: %s; %d windows of one %dx%dx3 uint8 frame (%.1f MB) from a pool of %d x %d frames (%.0f MB in HBM); %d blocks per form, alternated; "
             "%d calls per block ((c): %d batches)%s" % (torch.cuda.get_device_name(0), N, HS, HS, batch_mb, E, T, pool.numel() / 1e6, args.blocks, args.iters,
                                                          args.host_iters, "" if args.step_ms is None else "; step = %.3f ms (bench.py --gpus 1)" % args.step_ms)]
    mean = {}
    for name, _ in forms:
        t = times[name]
        mean[name] = sum(t) / len(t)
        share = "" if args.step_ms is None else "   = %6.2f %% of a step" % (100.0 * mean[name] / args.step_ms)
        rate = "   %.1f MB read + %.1f MB written -> %7.1f GB/s" % (batch_mb, batch_mb, 2 * batch_mb / mean[name]) if name.startswith("(a')") else ""   # MB / ms = GB/s
        lines.append("%-34s %8.4f ms (%8.4f .. %8.4f)%s%s" % (name, mean[name], min(t), max(t), share, rate))
    a, b, c = (mean[forms[i][0]] for i in (0, 2, 3))
    lines.append("(a) / (b) = %.3f   (a) / (c) = %.4f" % (a / b, a / c))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
