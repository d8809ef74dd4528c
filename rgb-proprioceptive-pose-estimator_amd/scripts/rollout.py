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
`--noise_scales` scores the same frames under several measurement-noise scales with one trunk pass.  An `--episodes` file of episodes
of unequal length (a `lengths` array) is scored this way only: `--errors_out` gains `lengths`, the entries behind an episode's end are NaN.

`--video_out FILE.gif|FILE.npy` (needs `--episodes` and `--camera_matrix FILE.npy`; implies `--batched`) is the reference's recorded
video without the simulator: the estimated and the true pose are projected through the camera's matrix and drawn on the recorded
frames on the device (util.learn_utils.render_episodes).  The reference's two flags keep their names: `--record_video` writes
`test.gif`, and `--model_outputs_file FILE.npy` draws the estimates of an earlier run's `--out` file instead of running the model.
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
    p.add_argument("--video_out", type=str, default=None, metavar="FILE.gif|FILE.npy", help="draw the estimated and the true pose on the recorded frames and "
                   "write the video here (util.learn_utils.render_episodes; implies --batched, needs --episodes and --camera_matrix)")
    p.add_argument("--camera_matrix", type=str, default=None, metavar="FILE.npy", help="(--video_out) the camera's 3x4 (or 4x4) projection matrix in STORED "
                   "pixel coordinates, or one per episode (E, ., 4); util.learn_utils.flip_camera_rows converts a matrix of the upright picture")
    p.add_argument("--video_fps", type=float, default=None, help="(--video_out) frames per second of the gif (default 10)")
    p.add_argument("--video_episodes", type=int, default=None, metavar="N", help="(--video_out) draw the first N scored episodes only (default: all)")
    p.add_argument("--video_draw", nargs="+", default=None, choices=["truth", "estimate", "measurement"], help="(--video_out) the poses to draw, in drawing "
                   "order (default: truth estimate)")
    p.add_argument("--axis_len", type=float, default=None, help="(--video_out) length of the drawn orientation axes in metres (default 0.05)")
    p.add_argument("--trail", type=int, default=None, help="(--video_out) how many earlier positions of the episode stay visible (default 8)")
    p.add_argument("--no_flip", action="store_true", help="(--video_out) keep the rows as stored (default: written bottom up, robosuite stores frames upside down)")
    p.add_argument("--no_bars", action="store_true", help="(--video_out) no error bars along the bottom edge")
    p.add_argument("--record_video", action="store_true", help="the reference's flag: --video_out test.gif")
    p.add_argument("--model_outputs_file", type=str, default=None, metavar="FILE.npy", help="the reference's flag: draw the estimates of an earlier run's "
                   "--out file, (E T, 7) or positions only (E T, 3), instead of running the model")
    args = p.parse_args(argv)
    video = video_flags(args)
    if args.noise_scales is not None or video is not None:
        args.batched = True
    if args.errors_out and not args.batched:
        raise SystemExit("rollout.py: --errors_out goes with --batched")
    from rgb_proprioceptive_pose_estimator_amd.models import PoseDistanceLoss
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset, synthetic_batch

    if args.episodes and (not args.batched or args.model_outputs_file):   # episodes of unequal length are scored by evaluate_episodes only
        try:
            ragged = RecordedEpisodeDataset.file_lengths(args.episodes) is not None
        except (OSError, ValueError):
            ragged = False   # (the dataset reports an unreadable file)
        if ragged:
            raise SystemExit("rollout.py: {} holds episodes of unequal length; the frame-by-frame walk and --model_outputs_file do not know padding: "
                             "use --batched (alone, or with --video_out)".format(args.episodes))
    np.random.seed(3)
    torch.manual_seed(3)
    if not torch.cuda.is_available():
        raise SystemExit("rollout.py: no MI355X visible; this path has no CPU fallback")
    model = build_model(args, DTYPES[args.dtype])
    if args.model_path:
        model.load_state_dict(torch.load(args.model_path, map_location=torch.device("cpu")))
    if args.batched:
        return batched(args, model.cuda(), video)
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


def video_flags(args):
    """Checks the video flags without touching a device -> None, or what the video needs: its file, the camera matrices and the keyword
    arguments of render_episodes"""
    out = args.video_out or ("test.gif" if args.record_video else None)
    if out is None:
        for flag in ("camera_matrix", "video_fps", "video_episodes", "video_draw", "axis_len", "trail", "model_outputs_file"):
            if getattr(args, flag) is not None:
                raise SystemExit("rollout.py: --{} belongs to --video_out (or --record_video)".format(flag))
        if args.no_flip or args.no_bars:
            raise SystemExit("rollout.py: --no_flip and --no_bars belong to --video_out (or --record_video)")
        return None
    if os.path.splitext(out)[1].lower() not in (".gif", ".npy"):
        raise SystemExit("rollout.py: --video_out writes a .gif or a .npy; got {}".format(out))
    if not args.episodes:
        raise SystemExit("rollout.py: the video is drawn on recorded frames: --video_out needs --episodes FILE.npz")
    if not args.camera_matrix:
        raise SystemExit("rollout.py: --video_out needs --camera_matrix FILE.npy, the projection matrix of the recording camera")
    if args.model_outputs_file and args.noise_scales is not None:
        raise SystemExit("rollout.py: --model_outputs_file holds one set of estimates; it does not go with --noise_scales")
    fps = 10.0 if args.video_fps is None else args.video_fps
    if not fps > 0:
        raise SystemExit("rollout.py: --video_fps must be positive")
    n = args.n_episodes if args.video_episodes is None else args.video_episodes
    if not 1 <= n <= args.n_episodes:
        raise SystemExit("rollout.py: --video_episodes lies in [1, --n_episodes = {}]".format(args.n_episodes))
    draw = tuple(args.video_draw or ("truth", "estimate"))
    if len(set(draw)) != len(draw):
        raise SystemExit("rollout.py: --video_draw names a pose set twice")
    if args.trail is not None and not 0 <= args.trail <= 64:
        raise SystemExit("rollout.py: --trail lies in [0, 64]")
    try:
        camera = np.load(args.camera_matrix, allow_pickle=False)
    except (OSError, ValueError) as e:
        raise SystemExit("rollout.py: --camera_matrix {}: {}".format(args.camera_matrix, e))
    if camera.ndim not in (2, 3) or camera.shape[-1] != 4 or camera.shape[-2] not in (3, 4) or (camera.ndim == 3 and camera.shape[0] < n):
        raise SystemExit("rollout.py: --camera_matrix holds a (3, 4) or (4, 4) matrix, or one per episode; got {}".format(camera.shape))
    kwargs = dict(draw=draw, flip=not args.no_flip, bars=not args.no_bars)
    if args.axis_len is not None:
        kwargs["axis_len"] = args.axis_len
    if args.trail is not None:
        kwargs["trail"] = args.trail
    return dict(out=out, fps=fps, episodes=n, camera=camera if camera.ndim == 2 else camera[:n], kwargs=kwargs)


def outputs_from_file(path, dataset, model, args):
    """--model_outputs_file: an EpisodeEvaluation from the estimates an earlier run wrote to --out, (E T, 7), or positions only, (E T, 3)
    as the reference writes them (no orientation: discs without axes, no orientation error); the model does not run"""
    import types

    from rgb_proprioceptive_pose_estimator_amd import ops
    E = args.n_episodes
    dataset.refresh_data(E, args.camera_name, args.noise_scale)
    d = dataset.data
    truth = (d["true_obj"] if hasattr(model, "object_name") else d["true_other"]).cuda().contiguous()
    T = truth.shape[1]
    est = np.load(path, allow_pickle=False)
    if est.ndim != 2 or est.shape[0] != E * T or est.shape[1] not in (3, 7):
        raise SystemExit("rollout.py: --model_outputs_file must hold ({} x {}, 7) or (.., 3) estimates; got {}".format(E, T, est.shape))
    est = torch.from_numpy(np.ascontiguousarray(est, dtype=np.float32)).cuda().reshape(E, T, -1)
    if est.shape[-1] == 7:
        pos, ori, poses = ops.pose_errors(est, truth, 1e-4, want_pose=True)
    else:
        pos = (est - truth[..., :3]).norm(dim=-1)
        ori = torch.zeros_like(pos)
        poses = torch.cat([est, torch.zeros((E, T, 4), dtype=torch.float32, device=est.device)], dim=-1)
    return types.SimpleNamespace(outputs=est, poses=poses, pos_err=pos, ori_err=ori, truth=truth, measurements=d["measurement_self"].cuda(), noise_scales=None)


def write_episode_video(res, dataset, video):
    """the first video["episodes"] scored episodes of `res` drawn on their recorded frames (dataset.data["imgs"]) and written out"""
    import types

    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import render_episodes, write_video
    n = video["episodes"]
    lead = (lambda t: None if t is None else t[:n]) if res.noise_scales is None else (lambda t: None if t is None else t[:, :n])
    part = types.SimpleNamespace(poses=lead(res.poses), pos_err=lead(res.pos_err), ori_err=lead(res.ori_err), truth=None if res.truth is None else res.truth[:n],
                                 measurements=lead(res.measurements), noise_scales=res.noise_scales)
    pictures = render_episodes(part, dataset.data["imgs"][:n], video["camera"], **video["kwargs"])
    lengths = None if getattr(res, "lengths", None) is None else res.lengths[:n]   # episodes of unequal length: the padding is not written
    write_video(pictures, video["out"], fps=video["fps"], lengths=lengths)
    print("wrote {} frames to {}".format(pictures.shape[0] * pictures.shape[1] if lengths is None else int(lengths.sum()), video["out"]))
    return pictures


def batched(args, model, video=None):
    """--batched: every episode at once through evaluate_episodes; same (E * T, 7) episode-major `--out` file as the frame-by-frame walk"""
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset, SyntheticEpisodeDataset
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import evaluate_episodes
    two_arm = not hasattr(model, "object_name")
    if video is not None and args.model_outputs_file:   # the second pass of the reference's workflow: draw what an earlier run estimated
        dataset = RecordedEpisodeDataset(args.episodes, use_depth=False, obj_name=args.obj_name, seed=args.episodes_seed)
        if two_arm and not dataset.is_two_arm:
            raise SystemExit("rollout.py: model '{}' estimates the second arm's pose; {} is not a two-arm recording".format(args.model, args.episodes))
        res = outputs_from_file(args.model_outputs_file, dataset, model, args)
        write_episode_video(res, dataset, video)
        return res
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
                     noise_scales=np.asarray([args.noise_scale] if args.noise_scales is None else args.noise_scales, dtype=np.float64),
                     **({} if res.lengths is None else {"lengths": res.lengths}))
    print(res.summary())
    if video is not None:
        write_episode_video(res, dataset, video)
    return res


if __name__ == "__main__":
    main()
