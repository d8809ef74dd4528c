"""TEST INFRASTRUCTURE ONLY -- generates tests/golden/pose_errors.npz by running the REFERENCE's own PoseDistanceLoss(mode="val")
(models/losses.py:95-113, imported through oracle/ref_stubs.py as oracle/gen_golden.py does) ONE SAMPLE AT A TIME, the way its
rollout() calls it once per step (util/learn_utils.py:455,492).  Run in the build container only, from the repository root:

    python -B tools/gen_pose_errors_golden.py <path to a checkout of the reference>

What is stored: 257 seeded (pred, truth) rows -- truth a random pose, prediction = another random pose + 0.3 * noise, the
construction of the oracle batch in tests/test_gpu_ops.py with its seeds (77, 1) -- the reference's position and orientation error
of every row (`pos`, `ori`, float64), and np.average / np.std of both as rollout() prints them.  Only numbers the reference computed
travel; none of its text does.

Every row must have |w| < 0.98 (w = the real part of qhat * truth^-1): there 2 acos(w) is well conditioned, d angle <= 10 d w, so
a per-sample relative tolerance on the angle means something.  The tool asserts it.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import pose_oracle as po  # noqa: E402
from oracle import ref_stubs  # noqa: E402

ref_stubs.install()
if len(sys.argv) < 2 or not os.path.isdir(sys.argv[1]):
    raise SystemExit(__doc__)
sys.path.insert(0, sys.argv[1])
from models.losses import PoseDistanceLoss  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pose_errors.npz")
N, DATA_SEED, NOISE_SEED, W_MAX = 257, 77, 1, 0.98


def rows():
    b = po.synth_batch((N,), DATA_SEED)   # (its frames are drawn first and not used; the poses follow them in the stream)
    pred = b["obj"] + 0.3 * torch.randn(N, 7, generator=torch.Generator().manual_seed(NOISE_SEED))
    return pred.contiguous(), b["x0"].contiguous()


def main():
    pred, truth = rows()
    q = pred[:, 3:].double()
    q = q / q.norm(dim=-1, keepdim=True)
    t = truth[:, 3:].double()
    w = (q * t).sum(-1) / (t * t).sum(-1)
    print("max |w| = %.4f" % w.abs().max().item())
    assert w.abs().max().item() < W_MAX, "a row is too close to |w| = 1 for a per-sample angle tolerance: choose other seeds"
    val = PoseDistanceLoss(mode="val")
    pos, ori = np.empty(N), np.empty(N)
    for i in range(N):
        pe, oe = val(pred[i:i + 1], truth[i:i + 1])
        pos[i], ori[i] = float(pe), float(oe)
    rec = dict(pred=pred.numpy(), truth=truth.numpy(), pos=pos, ori=ori, pos_average=np.average(pos), pos_std=np.std(pos),
               ori_average=np.average(ori), ori_std=np.std(ori), w_max=np.array(w.abs().max().item()))
    np.savez_compressed(OUT, **rec)
    print("%s: %d bytes; pos %.5f / %.5f m, ori %.5f / %.5f rad" % (OUT, os.path.getsize(OUT), rec["pos_average"], rec["pos_std"],
                                                                    rec["ori_average"], rec["ori_std"]))


if __name__ == "__main__":
    main()
