#!/usr/bin/env python
"""Rollout entry point (model side) on the MI355X path.

The reference's scripts/rollout.py drives a Robosuite simulator and renders video (rollout.py:141-187,
util/learn_utils.py:258-539); the simulator is out of scope, so this script keeps what belongs to the model:
the constructor flags, loading a reference-format state_dict checkpoint (rollout.py:193), the fixed seeds
(np/torch = 3, rollout.py:50-51), `model.eval(); model.rollout = True; model.reset_initial_state(1)`
(learn_utils.py:322-323,342), one call per timestep with the LSTM state carried on the module
(learn_utils.py:446), the per-step error print-out and the `model_outputs.npy` dump.  Frames come from a
seeded synthetic episode instead of `env.step`, or -- with `--episodes FILE.npz` -- from episodes recorded
from the simulator elsewhere (util.data_utils.RecordedEpisodeDataset): raw uint8 frames and raw depth, which
the model resizes, crops and normalises on the device.

`--batched` scores all episodes in one batched pass instead (util.learn_utils.evaluate_episodes: the episodes advance together as
lanes of one batch, per-step errors and their statistics are computed on the device) and prints the reference's summary lines;
`--noise_scales` scores the same frames under several measurement-noise scales with one trunk pass.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rgb_proprioceptive_pose_estimator_amd.scripts.train_model import DTYPES, build_model, build_parser  # noqa: E402


def main(argv=None):
    p = build_parser()
    p.add_argument("--model_path", type=str, default=None, help="state_dict .pth to load (reference key names)")
    p.add_argument("--n_episodes", type=int, default=10)
    p.add_argument("--out", type=str, default="model_outputs.npy")
    p.add_argument("--no_graph", action="store_true", help="launch every frame eagerly instead of replaying one captured hipGraph "
                   "(a frame is ~90 launches on one stream; replay: 0.45 ms, eager: 1.05-1.27 ms at batch 1 -- profiles/r03_rollout_latency.txt)")
    p.add_argument("--batched", action="store_true", help="score all episodes in one batched pass (evaluate_episodes) instead of frame by frame")
    p.add_argument("--max_frames", type=int, default=256, help="(--batched) frames per trunk batch: max(1, max_frames // n_episodes) timesteps per call")
    p.add_argument("--noise_scales", nargs="+", type=float, default=None, metavar="S",
                   help="score the same frames under these measurement-noise scales with one trunk pass (implies --batched; --out holds the first scale)")
    p.add_argument("--errors_out", type=str, default=None, metavar="FILE.npz", help="(--batched) write pos_err, ori_err, poses and noise_scales here")
    args = p.parse_args(argv)
    if args.noise_scales is not None:
        args.batched = True
    if args.errors_out and not args.batched:
        raise SystemExit("rollout.py: --errors_out goes with --batched")
    from rgb_proprioceptive_pose_estimator_amd.models import PoseDistanceLoss
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset, synthetic_batch

    np.random.seed(3)
    torch.manual_seed(3)
    if not torch.cuda.is_available():
        raise SystemExit("rollout.py: no MI355X visible; this path has no CPU fallback")
    model = build_model(args, DTYPES[args.dtype])
    if args.model_path:
        model.load_state_dict(torch.load(args.model_path, map_location=torch.device("cpu")))
    if args.batched:
        return batched(args, model.cuda())
    model.cuda().eval()
    model.rollout = True
    val = PoseDistanceLoss(mode="val")
    outs, pos_errs, ori_errs = [], [], []
    two_arm = not hasattr(model, "object_name")
    frame = None   # the captured frame (util.learn_utils.GraphedRolloutFrame): built from the first frame's tensors
    recorded = None
    if args.episodes:   # the first --n_episodes episodes of the file, measurement noise drawn as train() draws it
        recorded = RecordedEpisodeDataset(args.episodes, use_depth=args.use_depth, obj_name=args.obj_name, seed=args.episodes_seed)
        if two_arm and not recorded.is_two_arm:
            raise SystemExit("rollout.py: model '{}' estimates the second arm's pose; {} is not a two-arm recording".format(args.model, args.episodes))
        recorded.refresh_data(args.n_episodes, args.camera_name, args.noise_scale)
        args.horizon = recorded.env.horizon
    with torch.no_grad():
        for ep in range(args.n_episodes):
            model.reset_initial_state(1)
            if recorded is None:
                ep_b = synthetic_batch((args.horizon, 1), 3 + ep, with_depth=args.use_depth, noise_scale=args.noise_scale)
            else:   # (T, 1, ...) like the synthetic episode, frames and depth raw
                d = recorded.data
                on_dev = lambda k: d[k][ep].unsqueeze(1).cuda() if k in d else None
                ep_b = {"img": on_dev("imgs"), "depth": on_dev("depths"), "x0bar": on_dev("measurement_self"), "x1": on_dev("true_other"),
                        "obj": on_dev("true_obj")}
            for t in range(args.horizon):
                if model.requires_sequence:
                    img, x0bar = ep_b["img"][t:t + 1], ep_b["x0bar"][t:t + 1]
                    depth = None if ep_b["depth"] is None else ep_b["depth"][t:t + 1]
                else:
                    img, x0bar = ep_b["img"][t], ep_b["x0bar"][t]
                    depth = None if ep_b["depth"] is None else ep_b["depth"][t]
                if frame is None and not args.no_graph:
                    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import GraphedRolloutFrame
                    frame = GraphedRolloutFrame(model, img.cuda(), None if depth is None else depth.cuda(), x0bar.cuda())
                    model.reset_initial_state(1)   # (capture and warm-up frames advanced the carried LSTM state)
                out = model(img, depth, x0bar) if frame is None else frame(img, depth, x0bar)
                out = out[-1] if isinstance(out, tuple) else out
                truth = (ep_b["x1"] if two_arm else ep_b["obj"])[t].reshape(out.shape)
                pe, oe = val(out, truth)
                pos_errs.append(float(pe)), ori_errs.append(float(oe))
                outs.append(out.reshape(7).cpu().numpy())
            print("episode {}: mean pos err {:.4f} m, mean ori err {:.4f} rad".format(ep, np.mean(pos_errs[-args.horizon:]), np.mean(ori_errs[-args.horizon:])))
    np.save(args.out, np.stack(outs))
    print("Mean pos err {:.4f} (std {:.4f}), mean ori err {:.4f} (std {:.4f})".format(np.mean(pos_errs), np.std(pos_errs), np.mean(ori_errs), np.std(ori_errs)))


def batched(args, model):
    """--batched: every episode at once through evaluate_episodes; same (E * T, 7) episode-major `--out` file as the frame-by-frame walk"""
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset, SyntheticEpisodeDataset
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import evaluate_episodes
    two_arm = not hasattr(model, "object_name")
    if args.episodes:
        dataset = RecordedEpisodeDataset(args.episodes, use_depth=args.use_depth, obj_name=args.obj_name, seed=args.episodes_seed)
        if two_arm and not dataset.is_two_arm:
            raise SystemExit("rollout.py: model '{}' estimates the second arm's pose; {} is not a two-arm recording".format(args.model, args.episodes))
    else:
        dataset = SyntheticEpisodeDataset(horizon=args.horizon, use_depth=args.use_depth, obj_name=args.obj_name, is_two_arm=two_arm,
                                          seed=args.episodes_seed, env_name=args.env)
    res = evaluate_episodes(model, dataset, args.n_episodes, {"camera_name": args.camera_name, "noise_scale": args.noise_scale},
                            max_frames=args.max_frames, noise_scales=args.noise_scales, noise_seed=args.episodes_seed)
    first = res.outputs if args.noise_scales is None else res.outputs[0]
    np.save(args.out, first.reshape(-1, 7).cpu().numpy())
    if args.errors_out:
        with open(args.errors_out, "wb") as f:   # (np.savez would append ".npz" to a bare name)
            np.savez(f, pos_err=res.pos_err.cpu().numpy(), ori_err=res.ori_err.cpu().numpy(), poses=res.poses.cpu().numpy(),
                     noise_scales=np.asarray([args.noise_scale] if args.noise_scales is None else args.noise_scales, dtype=np.float64))
    print(res.summary())
    return res


if __name__ == "__main__":
    main()
