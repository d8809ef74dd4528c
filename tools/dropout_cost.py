"""Diagnostic (GPU box): what head dropout costs.  Two measurements in ONE process, every pair alternated block by block after a
warm-up of both forms:

  1 the launches alone, at the workload's row shapes -- 256 rows x the `tdo` feature width (latent 512 + aux 3136 of 3655 columns, the
    site-0 range) in place, and 256 x 512 (a hidden site) out of place -- against torch.nn.functional.dropout, eager, on the same
    tensors: (a) ops.dropout_rows, one launch; (a') ops.dropout_begin + ops.dropout_rows, what the first site of a step pays;
    (b) F.dropout(x, p, training=True, inplace=...).
  2 the whole `tdo` train step of bench.py's workload (bf16 trunk, (S, N) = (4, 64), latent 512, hidden 512, FusedAdam, eager issue):
    a model with set_dropout(feature=0.1, hidden=0.1) against the same model with dropout off -- which is the parent's step: with
    dropout off no launch is added (tests/test_gpu_dropout.py::test_dropout_off_changes_nothing).  +5 launches per step:
    one begin, two sites forward, two backward.

Blocks of `iters` back-to-back calls (or `step_iters` steps) between HIP events.  Reported per form: the mean over the blocks and their
range.  A record, not a bar.  Writes profiles/dropout_cost.txt (or --out).

usage: python tools/dropout_cost.py [--iters N] [--blocks N] [--step_iters N] [--step_blocks N] [--out FILE]"""
import argparse
import contextlib
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgb_proprioceptive_pose_estimator_amd import models as M, ops  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.util.data_utils import synthetic_batch  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import train_step  # noqa: E402

P = 0.1
ROWS, LATENT, AUX, HIDDEN = 256, 512, 3136, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="launches per timed block")
    ap.add_argument("--blocks", type=int, default=10, help="timed blocks per form, alternated")
    ap.add_argument("--step_iters", type=int, default=20, help="train steps per timed block")
    ap.add_argument("--step_blocks", type=int, default=6, help="timed blocks of train steps per form, alternated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_cost.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dropout_cost.py: no GPU visible; a CPU run measures nothing")
    dev = torch.device("cuda", 0)

    def events(fn, iters):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / iters

    def alternate(forms, iters, blocks, warm=3):
        for _ in range(warm):
            for _, fn in forms:
                events(fn, iters)
        times = {name: [] for name, _ in forms}
        for _ in range(blocks):
            for name, fn in forms:
                times[name].append(events(fn, iters))
        return times

    lines = ["device: %s; head dropout, p = %g; launches: %d blocks per form, alternated, %d calls per block; steps: %d blocks per form, alternated, %d steps "
             "per block" % (torch.cuda.get_device_name(0), P, args.blocks, args.iters, args.step_blocks, args.step_iters)]
    desc = ops.dropout_desc(P, 1)
    state, picks = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    width = LATENT + AUX + 7
    for label, cols, c1, inplace in (("site 0: %d rows x %d columns of %d, in place" % (ROWS, LATENT + AUX, width), width, LATENT + AUX, True),
                                     ("hidden site: %d rows x %d, out of place" % (ROWS, HIDDEN), HIDDEN, HIDDEN, False)):
        buf = torch.randn(ROWS, ops.pad4(cols), device=dev)
        x = buf[:, :cols]
        out = None if inplace else torch.empty_like(buf)[:, :cols]
        ref = buf.clone()[:, :c1] if inplace else x

        def rows():
            ops.dropout_rows(x, desc, picks, site=0, c1=c1, out=out)

        def begin_rows():
            ops.dropout_begin(state, picks)
            ops.dropout_rows(x, desc, picks, site=0, c1=c1, out=out)

        forms = [("(a)  dropout_rows, 1 launch", rows), ("(a') dropout_begin + dropout_rows, 2 launches", begin_rows),
                 ("(b)  torch eager F.dropout", lambda: F.dropout(ref, P, True, inplace))]
        times = alternate(forms, args.iters, args.blocks)
        mb = ROWS * c1 * 8 / 1e6
        lines.append("%s (%.2f MB read + written)" % (label, mb))
        mean = {}
        for name, _ in forms:
            t = times[name]
            mean[name] = sum(t) / len(t)
            lines.append("  %-48s %8.4f ms (%8.4f .. %8.4f)" % (name, mean[name], min(t), max(t)))
        lines.append("  (a) / (b) = %.3f   (a') / (b) = %.3f" % (mean[forms[0][0]] / mean[forms[2][0]], mean[forms[1][0]] / mean[forms[2][0]]))

    # the whole tdo step, dropout on against dropout off (= the parent's step)
    def make(on):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(sys.stderr):
            model = M.TemporallyDependentObjectStateEstimator("hammer", HIDDEN, 50, LATENT, 4, 0.1, False, (9,), False, False, False, compute_dtype=torch.bfloat16)
        model.cuda().train()
        if on:
            model.set_dropout(feature=P, hidden=P, seed=1)
        return model, FusedAdam(model.parameters(), lr=1e-3)

    mk = lambda: M.PoseDistanceLoss(distance_metric="combined", scale_factor=1.0, alpha=0.5, mode="pose")
    criterion = {"obj_loss": mk(), "val_loss": M.PoseDistanceLoss(mode="val")}
    b = synthetic_batch((4, ROWS // 4), 1234, with_depth=False, device=dev)
    batch = (b["img"], b["depth"], b["x0bar"], b["x0"], b["x1"], b["obj"])
    (m_off, o_off), (m_on, o_on) = make(False), make(True)
    forms = [("dropout off (the parent's step)", lambda: train_step(m_off, batch, criterion, o_off, True, "train", None)),
             ("dropout on: feature %g, hidden %g, +5 launches" % (P, P), lambda: train_step(m_on, batch, criterion, o_on, True, "train", None))]
    times = alternate(forms, args.step_iters, args.step_blocks, warm=4)
    lines.append("tdo train step, bf16, (S, N) = (4, %d), latent %d, hidden %d, FusedAdam, eager issue" % (ROWS // 4, LATENT, HIDDEN))
    mean = {}
    for name, _ in forms:
        t = times[name]
        mean[name] = sum(t) / len(t)
        lines.append("  %-48s %8.3f ms per step (%8.3f .. %8.3f)" % (name, mean[name], min(t), max(t)))
    d = mean[forms[1][0]] - mean[forms[0][0]]
    lines.append("  on - off = %+.3f ms per step = %+.2f %%; the counter after the run: %d steps" % (d, 100.0 * d / mean[forms[0][0]], m_on._drop_state.item()))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
