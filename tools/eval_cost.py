"""Diagnostic (GPU box): what scoring recorded episodes costs, batched against frame by frame.

Model tdo / ResNet-50 / bf16 at the scripts' default head sizes; data 10 recorded episodes x 20 steps of raw 256 x 256 uint8 frames
(seeded, written to a temporary file).  Three arms, ALTERNATED round after round in one process on one box, each timed with the host
clock around work that ends in a device synchronise, host -> device copies of the frames included:

  batched       util.learn_utils.evaluate_episodes: all episodes as lanes, max_frames 256 -> 25 timesteps per call
  frame graph   the loop of scripts/rollout.py: one frame per call at batch 1 through a captured hipGraph, PoseDistanceLoss(mode="val")
                and a .cpu() of the output per frame, mean / std in numpy at the end
  frame eager   the same loop with --no_graph

The first round of every arm is warm-up (plans, workspaces, the graph capture) and is printed but kept out of the median.  The arms
score the same episodes; the largest relative difference of their outputs is printed (bf16: batching changes which GEMM tiles run).

usage: python tools/eval_cost.py [rounds] [output file]"""
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgb_proprioceptive_pose_estimator_amd import models as M  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import GraphedRolloutFrame, evaluate_episodes  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
out_path = sys.argv[2] if len(sys.argv) > 2 else None
E, T, HW = 10, 20, 256
PARAMS = {"camera_name": "frontview", "noise_scale": 0.001}
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def episode_file(path):
    rng = np.random.default_rng(0)

    def poses():
        q = rng.normal(size=(E, T, 4))
        q = q / np.linalg.norm(q, axis=-1, keepdims=True)
        return np.concatenate([rng.random((E, T, 3)), np.where(q[..., 3:] < 0, -q, q)], -1).astype(np.float32)
    return RecordedEpisodeDataset.save(path, env_name="Lift", imgs=rng.integers(0, 256, (E, T, HW, HW, 3), dtype=np.uint8), true_self=poses(),
                                       true_obj=poses())


def frame_by_frame(model, ds, frame):
    """scripts/rollout.py's loop on `ds.data`; `frame` is the GraphedRolloutFrame or None (--no_graph)"""
    val = M.PoseDistanceLoss(mode="val")
    model.eval()
    model.rollout = True
    outs, pos_errs, ori_errs = [], [], []
    d = ds.data
    with torch.no_grad():
        for ep in range(E):
            model.reset_initial_state(1)
            img_e, x_e, obj_e = d["imgs"][ep].unsqueeze(1).cuda(), d["measurement_self"][ep].unsqueeze(1).cuda(), d["true_obj"][ep].unsqueeze(1).cuda()
            for t in range(T):
                img, x0bar = img_e[t:t + 1], x_e[t:t + 1]
                out = model(img, None, x0bar) if frame is None else frame(img, None, x0bar)
                pe, oe = val(out, obj_e[t].reshape(out.shape))
                pos_errs.append(float(pe)), ori_errs.append(float(oe))
                outs.append(out.reshape(7).cpu().numpy())
    model.rollout = False
    return np.stack(outs), (np.mean(pos_errs), np.std(pos_errs), np.mean(ori_errs), np.std(ori_errs))


def main():
    torch.manual_seed(3)
    model = M.TemporallyDependentObjectStateEstimator(object_name="cube", hidden_dim=512, num_resnet_layers=50, latent_dim=1024, sequence_length=10,
                                                      feature_layer_nums=(9,), use_depth=False, use_pretrained=False,
                                                      compute_dtype=torch.bfloat16).cuda().eval()
    with tempfile.TemporaryDirectory() as tmp:
        path = episode_file(os.path.join(tmp, "episodes.npz"))
        fresh = lambda: RecordedEpisodeDataset(path, obj_name="cube")   # same seed every time: the same measurement noise
        ds = fresh()
        ds.refresh_data(E, None, PARAMS["noise_scale"])
        model.rollout = True
        d = ds.data
        frame = GraphedRolloutFrame(model, d["imgs"][0, :1].unsqueeze(1).cuda(), None, d["measurement_self"][0, :1].unsqueeze(1).cuda())
        say("device: %s; tdo / ResNet-50 / bf16, %d episodes x %d steps of %dx%d frames; captured frame %s (replay %s ms, eager %s ms)"
            % (torch.cuda.get_device_name(0), E, T, HW, HW, "replays" if frame.replaying else "fell back to eager", frame.replay_ms, frame.eager_ms))
        times = {"batched": [], "frame graph": [], "frame eager": []}
        outs = {}
        for r in range(rounds):
            for arm in times:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if arm == "batched":
                    res = evaluate_episodes(model, fresh(), E, PARAMS, max_frames=256)
                    o = res.outputs.reshape(-1, 7).cpu().numpy()
                    stats = (res.pos_mean, res.pos_std, res.ori_mean, res.ori_std)
                else:
                    o, stats = frame_by_frame(model, ds, frame if arm == "frame graph" else None)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                times[arm].append(ms)
                outs[arm] = o
                say("round %d  %-11s %9.2f ms   pos %.5f / %.5f m, ori %.5f / %.5f rad%s" % ((r, arm, ms) + tuple(float(s) for s in stats) + ("   (warm-up)" if r == 0 else "",)))
        for arm, ts in times.items():
            kept = ts[1:] or ts
            say("%-11s median %9.2f ms  min %9.2f  max %9.2f  over %d rounds  = %.3f ms per frame" % (arm, statistics.median(kept), min(kept), max(kept), len(kept),
                                                                                                   statistics.median(kept) / (E * T)))
        ref = outs["frame eager"]
        for arm in ("batched", "frame graph"):
            say("%-11s vs frame eager: max |diff| / max |out| = %.2e" % (arm, np.abs(outs[arm] - ref).max() / np.abs(ref).max()))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
