#!/usr/bin/env python
"""Training entry point on the MI355X path.

Keeps every flag of the reference's scripts/train_model.py:17-47 (names, types, defaults) and its model-constructor
dispatch (:158-218), criterion dict (:100-105), Adam (:228) and train() call (:248-259).  The Robosuite environment
the reference builds at import time (:84-97) is replaced by seeded synthetic Robosuite-shaped episodes; flags that only
configure the simulator (--controller, --robots, --use_placement_initializer, --motion) are accepted and recorded.
Added flags: --dtype {bf16,f16,f32}, --optimizer {fused,torch}, --max_grad_norm, --weight_decay, --episodes_seed; the on-device
learning-rate schedule (--lr_schedule, --warmup_steps, --warmup_start_factor, --lr_total_steps, --lr_min_factor, --lr_step_size,
--lr_gamma), --trunk_lr_scale (the trunk as a param group of its own) and --ema_decay (writes `<checkpoint>.ema` beside the raw weights);
the on-device frame augmentation of recorded episodes (--aug_brightness, --aug_contrast, --aug_saturation, --aug_noise_std,
--aug_erase_prob, --aug_erase_scale, --aug_erase_fill, --aug_blur_prob, --aug_blur_sigma, --aug_motion_prob, --aug_motion_max_length,
--aug_per_frame, --aug_seed; all off by default, they need --episodes) and of
their depth frames (--aug_depth_noise, --aug_depth_drop_prob, --aug_depth_holes, --aug_depth_hole_scale, --aug_depth_hole_value,
--aug_depth_quant, --aug_depth_clamp, --aug_depth_share_erase, --aug_depth_occluder_value; off by default, they need --use_depth --episodes);
--resident (the --episodes file lives in HBM; an --episodes file of episodes of unequal length needs it and --batch_size) and, with it, --batch_size, --window_stride, --shuffle_seed (shuffled minibatches drawn on the
device instead of one chunk of every episode per step); --meas_noise_device / --meas_noise_scales, --meas_noise_correlation,
--meas_noise_seed (the measurement noise of the `train` phase drawn on the device, fresh at every step; off by default, any dataset).

Multi-GPU: launch with `python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 scripts/train_model.py ...`;
episodes are sharded over ranks and gradients SUM-all-reduced over RCCL.
"""
import argparse
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODELS = {'n', 'no', 'td', 'tdo', 'tdo_v2'}


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--model", type=str, default="n", help="Which mode to run. Options are 'n', 'no', 'td', 'tdo' or 'tdo_v2'")
    p.add_argument("--controller", type=str, default="OSC_POSE", help="(simulator only) controller name")
    p.add_argument("--camera_name", type=str, default="frontview", help="Name of camera to render for observations")
    p.add_argument("--horizon", type=int, default=100, help="Horizon per episode run")
    p.add_argument("--sequence_length", type=int, default=10, help="Sequence length for LSTMs")
    p.add_argument("--noise_scale", type=float, default=0.001, help="Noise scale for self measurements")
    p.add_argument("--latent_dim", type=int, default=1024, help="Dimension of output from ResNet")
    p.add_argument("--hidden_dim", nargs="+", type=int, default=[512], help="Hidden dimensions in FC network (naive only), or LSTM net (td/o only)")
    p.add_argument("--proprio_hidden_dim", type=int, default=64, help="Hidden dimensions in proprio LSTM net (tdo_v2 only)")
    p.add_argument("--lr", type=float, default=0.001, help="Learning rate for Adam optimizer")
    p.add_argument("--n_train_episodes_per_epoch", type=int, default=10, help="Number of training episodes per epoch")
    p.add_argument("--n_val_episodes_per_epoch", type=int, default=2, help="Number of validation episodes per epoch")
    p.add_argument("--env", type=str, default="TwoArmLift", help="Environment name (two-arm iff it contains 'TwoArm')")
    p.add_argument("--robots", nargs="+", type=str, default=["Panda", "Sawyer"], help="(simulator only) robot names")
    p.add_argument("--use_placement_initializer", action="store_true", help="(simulator only)")
    p.add_argument("--feature_extract", action="store_true", help="Whether ResNet will be set to feature extract mode or not")
    p.add_argument("--no_proprioception", action="store_true", help="If set, will not leverage proprioceptive measurements during training")
    p.add_argument("--use_depth", action="store_true", help="Whether to use depth or not")
    p.add_argument("--use_pretrained", action="store_true", help="Whether to use pretrained ResNet or not")
    p.add_argument("--obj_name", type=str, default=None, help="Object name to generate observations of")
    p.add_argument("--motion", type=str, default="random", help="Type of robot motion to use")
    p.add_argument("--distance_metric", type=str, default="l2", help="Distance metric to use for loss")
    p.add_argument("--loss_mode", type=str, default="pose", help="Type of loss to use. Options are 'position' or 'pose'")
    p.add_argument("--loss_scale_factor", type=float, default=1.0, help="Scaling factor for Pose loss")
    p.add_argument("--alpha", type=float, default=0.5, help="Orientation loss scaling factor relative to position error")
    p.add_argument("--n_epochs", type=int, default=5000, help="Number of epochs")
    p.add_argument("--load_checkpoint", action="store_true", help="Whether to load prior trained model")
    p.add_argument("--checkpoint_model_path", type=str, default="../log/runs/model.pth", help="Path to checkpoint .pth file to load into model")
    # additions
    p.add_argument("--dtype", choices=["bf16", "f16", "f32"], default="bf16",
                   help="compute dtype of the conv trunk (fp32 accumulate either way; f16 adds dynamic loss scaling and needs --optimizer fused)")
    p.add_argument("--optimizer", choices=["fused", "torch"], default="fused", help="FusedAdam (one HIP kernel) or torch.optim.Adam")
    p.add_argument("--max_grad_norm", type=float, default=None,
                   help="clip the global gradient norm to this value on the device before the Adam update (default: off; needs --optimizer fused)")
    p.add_argument("--weight_decay", type=float, default=0.0, help="decoupled weight decay (AdamW; default 0 = plain Adam)")
    p.add_argument("--lr_schedule", choices=["constant", "cosine", "step"], default=None,
                   help="learning-rate schedule evaluated on the device (optim.LRSchedule; default: none; needs --optimizer fused, like the flags below)")
    p.add_argument("--warmup_steps", type=int, default=None, help="linear warm-up over this many optimizer steps (default 0)")
    p.add_argument("--warmup_start_factor", type=float, default=None, help="the warm-up starts at lr times this (default 0.1)")
    p.add_argument("--lr_total_steps", type=int, default=None, help="cosine: the step at which lr reaches lr * lr_min_factor (required for cosine)")
    p.add_argument("--lr_min_factor", type=float, default=None, help="cosine: the final factor (default 0)")
    p.add_argument("--lr_step_size", type=int, default=None, help="step: multiply lr by lr_gamma every this many steps after the warm-up")
    p.add_argument("--lr_gamma", type=float, default=None, help="step: the factor (default 0.1)")
    p.add_argument("--trunk_lr_scale", type=float, default=None, help="train the ResNet trunk at lr times this, as a param group of its own (default: one group)")
    p.add_argument("--ema_decay", type=float, default=None,
                   help="keep an exponential moving average of the weights on the device, validate with it and save it as <checkpoint>.ema (default: off)")
    p.add_argument("--telemetry", type=int, nargs="?", const=1, default=None, metavar="K",
                   help="per-tensor gradient / weight / update norms, non-finite and zero counts, measured on the device every K-th optimizer "
                        "step (K = 1 when given without a value) and logged once per epoch; needs --optimizer fused (default: off)")
    p.add_argument("--telemetry_out", type=str, default=None, metavar="FILE.npz", help="with --telemetry: save the per-epoch tables and the parameter names")
    p.add_argument("--episodes_seed", type=int, default=1234, help="seed of the synthetic episode generator")
    p.add_argument("--no_save", action="store_true", help="do not write the best-validation checkpoint")
    p.add_argument("--episodes", type=str, default=None, metavar="FILE.npz",
                   help="recorded raw episodes (util.data_utils.RecordedEpisodeDataset: imgs uint8 (E,T,Hs,Ws,3), depths float32 (E,T,Hs,Ws,1), "
                        "true_self / true_other / true_obj (E,T,7)) instead of synthetic ones; the horizon is the file's")
    p.add_argument("--aug_brightness", type=float, default=None, help="augmentation (needs --episodes): brightness factor in [max(0, 1 - b), 1 + b] (default: off)")
    p.add_argument("--aug_contrast", type=float, default=None, help="augmentation: contrast factor range, as --aug_brightness (default: off)")
    p.add_argument("--aug_saturation", type=float, default=None, help="augmentation: saturation factor range, as --aug_brightness (default: off)")
    p.add_argument("--aug_noise_std", type=float, default=None, help="augmentation: sensor noise, standard deviation in grey levels (default: off)")
    p.add_argument("--aug_erase_prob", type=float, default=None, help="augmentation: probability of erasing one rectangle per frame (default: off)")
    p.add_argument("--aug_erase_scale", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="augmentation: each side of the erased rectangle as a fraction of the frame's (default 0.1 0.3)")
    p.add_argument("--aug_erase_fill", type=str, default=None, help="augmentation: 'mean' (ImageNet mean, the default), 'noise' (random bytes) or R,G,B bytes")
    p.add_argument("--aug_blur_prob", type=float, default=None, metavar="P", help="augmentation: probability of a Gaussian (defocus) blur per frame (default: off)")
    p.add_argument("--aug_blur_sigma", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="augmentation: the Gaussian blur's sigma range in pixels, 0 <= LO <= HI <= 4 (default 0.5 2.0)")
    p.add_argument("--aug_motion_prob", type=float, default=None, metavar="P", help="augmentation: probability of a linear motion blur per frame (default: off)")
    p.add_argument("--aug_motion_max_length", type=int, default=None, metavar="L", help="augmentation: the longest motion blur in pixels, odd, 3 .. 15 (default 9)")
    p.add_argument("--aug_per_frame", action="store_true",
                   help="augmentation: draw jitter and occluder per frame (default: per episode, kept through a chunk of --sequence_length steps)")
    p.add_argument("--aug_seed", type=int, default=None, help="augmentation: seed of the device generator (default 0; rank r uses seed + r)")
    p.add_argument("--aug_depth_noise", type=float, nargs="+", default=None, metavar="S",
                   help="depth augmentation (needs --use_depth --episodes): S0 [S1 [S2]], noise of standard deviation S0 + S1 d + S2 d^2 at depth d, "
                        "in the units of the recorded depth values (default: off)")
    p.add_argument("--aug_depth_drop_prob", type=float, default=None, metavar="P", help="depth augmentation: probability that a pixel becomes the hole value (default: off)")
    p.add_argument("--aug_depth_holes", type=int, nargs=2, default=None, metavar=("LO", "HI"),
                   help="depth augmentation: LO..HI hole rectangles per frame, at most 4 (default 0 0: off)")
    p.add_argument("--aug_depth_hole_scale", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                   help="depth augmentation: each side of a hole as a fraction of the frame's (default 0.02 0.15)")
    p.add_argument("--aug_depth_hole_value", type=float, default=None, metavar="V", help="depth augmentation: what dropped and hole pixels become (default 0)")
    p.add_argument("--aug_depth_quant", type=float, default=None, metavar="Q", help="depth augmentation: round to multiples of Q (default: off)")
    p.add_argument("--aug_depth_clamp", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="depth augmentation: limit to [LO, HI] (default: off)")
    p.add_argument("--aug_depth_share_erase", action="store_true",
                   help="depth augmentation: the rectangle --aug_erase_prob erases in the RGB frame is covered in depth as well (needs --aug_erase_prob)")
    p.add_argument("--aug_depth_occluder_value", type=float, default=None, metavar="V",
                   help="depth augmentation: what the shared occluder writes (default 0)")
    p.add_argument("--resident", action="store_true",
                   help="keep the whole --episodes file in HBM (util.data_utils.ResidentEpisodeDataset): batches are gathered on the device, no PCIe per step")
    p.add_argument("--batch_size", type=int, default=None,
                   help="train on shuffled minibatches of this many windows of --sequence_length steps (one frame for the models without a sequence), "
                        "drawn on the device (needs --episodes --resident; default: one chunk of every episode per step, in file order)")
    p.add_argument("--window_stride", type=int, default=None, help="sampling: distance of window starts (default: the window's length; 1 = every offset)")
    p.add_argument("--shuffle_seed", type=int, default=None, help="sampling: seed of the device sampler (default 0; rank r uses seed + r)")
    p.add_argument("--meas_noise_device", action="store_true",
                   help="draw the measurement noise of the train phase on the device, fresh at every step (util.data_utils.MeasurementNoise), "
                        "with the variance --noise_scale (default: the dataset's host draw, once per refresh)")
    p.add_argument("--meas_noise_scales", type=float, nargs="+", default=None, metavar="S",
                   help="device measurement noise with 1..8 variances instead of --noise_scale: every window draws one of them per step")
    p.add_argument("--meas_noise_correlation", type=float, default=None, metavar="R",
                   help="device measurement noise: AR(1) coefficient in [0, 1) along the --sequence_length steps of a window (default 0: white)")
    p.add_argument("--meas_noise_seed", type=int, default=None, metavar="K", help="device measurement noise: seed of the device generator (default 0; rank r uses K + r)")
    p.add_argument("--feature_dropout", type=float, default=0.0, metavar="P",
                   help="dropout on the feature columns the heads read (ResNet latent + aux head; never the proprioceptive columns), probability in "
                        "[0, 1), training forwards only, masks drawn on the device (PoseModelBase.set_dropout; default 0: off)")
    p.add_argument("--hidden_dropout", type=float, default=0.0, metavar="Q",
                   help="dropout on every step's LSTM output in front of the Linear that reads it (td / tdo / tdo_v2 only), probability in [0, 1) (default 0: off)")
    p.add_argument("--dropout_seed", type=int, default=0, metavar="K", help="dropout: seed of the device generator (default 0; rank r uses K + r)")
    return p


def apply_dropout(args, model=None, rank=0):
    """--feature_dropout / --hidden_dropout / --dropout_seed -> model.set_dropout(...), with the seed K + rank so that data-parallel
    replicas do not share masks.  Without a model the flags are only checked; with both probabilities 0 the model is left as built."""
    feature, hidden, seed = (getattr(args, k, d) for k, d in (("feature_dropout", 0.0), ("hidden_dropout", 0.0), ("dropout_seed", 0)))
    for flag, v in (("--feature_dropout", feature), ("--hidden_dropout", hidden)):
        if not 0.0 <= v < 1.0:
            raise SystemExit("%s must lie in [0, 1); got %r" % (flag, v))
    if not (0 <= seed and seed + rank < 2 ** 64):
        raise SystemExit("--dropout_seed must fit 64 unsigned bits (rank r uses K + r); got %d" % seed)
    if hidden > 0.0 and getattr(args, "model", None) in ("n", "no"):
        raise SystemExit("--hidden_dropout drops LSTM outputs: the models td, tdo and tdo_v2 have them, --model %s does not" % args.model)
    if model is not None and (feature > 0.0 or hidden > 0.0):
        model.set_dropout(feature=feature, hidden=hidden, seed=seed + rank)
    return model


def build_measurement_noise(args, rank=0):
    """--meas_noise_device / --meas_noise_scales / --meas_noise_correlation / --meas_noise_seed -> util.data_utils.MeasurementNoise,
    or None when none of them is given.  Any of the four turns the device draw on; the variances default to [--noise_scale].  They
    need no other flag: the draw takes the batch's true poses, which every dataset hands out."""
    scales, rho, seed = (getattr(args, k, None) for k in ("meas_noise_scales", "meas_noise_correlation", "meas_noise_seed"))
    if not getattr(args, "meas_noise_device", False) and scales is None and rho is None and seed is None:
        return None
    from rgb_proprioceptive_pose_estimator_amd.ops import MEASURE_MAX_SCALES
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import MeasurementNoise
    flag = "--meas_noise_scales" if scales is not None else "--noise_scale"
    scales = [args.noise_scale] if scales is None else list(scales)
    if not 1 <= len(scales) <= MEASURE_MAX_SCALES:
        raise SystemExit("%s takes 1..%d variances; got %d" % (flag, MEASURE_MAX_SCALES, len(scales)))
    if not all(v >= 0.0 and v != float("inf") for v in scales):
        raise SystemExit("%s: a variance is finite and not negative; got %r" % (flag, scales))
    rho = 0.0 if rho is None else rho
    if not 0.0 <= rho < 1.0:
        raise SystemExit("--meas_noise_correlation must lie in [0, 1); got %r" % rho)
    seed = (seed or 0)
    if not (0 <= seed and seed + rank < 2 ** 64):
        raise SystemExit("--meas_noise_seed must fit 64 unsigned bits (rank r uses K + r); got %d" % seed)
    return MeasurementNoise(scales, correlation=rho, seed=seed + rank)


def build_sampling(args):
    """--resident / --batch_size / --window_stride / --shuffle_seed -> the keyword arguments of train() that select minibatch
    sampling ({} when --batch_size is not given).  --resident needs --episodes, the other three need --episodes --resident."""
    if getattr(args, "resident", False) and not getattr(args, "episodes", None):
        raise SystemExit("--resident needs --episodes: it keeps a file of recorded episodes in HBM")
    batch_size = getattr(args, "batch_size", None)
    for flag in ("batch_size", "window_stride", "shuffle_seed"):
        if getattr(args, flag, None) is not None and not (getattr(args, "episodes", None) and getattr(args, "resident", False)):
            raise SystemExit("--%s needs --episodes --resident: minibatches are drawn on the device from episodes resident in HBM" % flag)
    if batch_size is None:
        for flag in ("window_stride", "shuffle_seed"):
            if getattr(args, flag, None) is not None:
                raise SystemExit("--%s needs --batch_size" % flag)
        return {}
    if batch_size < 1:
        raise SystemExit("--batch_size must be at least 1; got %d" % batch_size)
    if args.window_stride is not None and args.window_stride < 1:
        raise SystemExit("--window_stride must be at least 1; got %d" % args.window_stride)
    seed = args.shuffle_seed or 0
    if not 0 <= seed < 2 ** 64:
        raise SystemExit("--shuffle_seed must fit 64 unsigned bits; got %d" % seed)
    return dict(batch_size=batch_size, window_stride=args.window_stride, shuffle_seed=seed)


AUGMENT_FLAGS = ("aug_brightness", "aug_contrast", "aug_saturation", "aug_noise_std", "aug_erase_prob", "aug_erase_scale", "aug_erase_fill", "aug_seed")
BLUR_FLAGS = ("aug_blur_prob", "aug_blur_sigma", "aug_motion_prob", "aug_motion_max_length")


def build_augment(args, rank=0):
    """the --aug_* family -> util.data_utils.FrameAugment, or None when none of its flags is given.  The flags need --episodes: the
    synthetic episodes are preprocessed float images, which the augmentation does not take."""
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import FrameAugment
    given = {k: getattr(args, k, None) for k in AUGMENT_FLAGS + BLUR_FLAGS}
    if all(v is None for v in given.values()) and not getattr(args, "aug_per_frame", False):
        return None
    if not getattr(args, "episodes", None):
        raise SystemExit("the --aug_* flags need --episodes: the augmentation works on recorded raw uint8 frames")
    fill = given["aug_erase_fill"] or "mean"
    if fill not in ("mean", "noise"):
        try:
            fill = tuple(int(v) for v in fill.split(","))
        except ValueError:
            raise SystemExit("--aug_erase_fill is 'mean', 'noise' or R,G,B; got %r" % given["aug_erase_fill"])
    try:
        return FrameAugment(brightness=given["aug_brightness"] or 0.0, contrast=given["aug_contrast"] or 0.0, saturation=given["aug_saturation"] or 0.0,
                            noise_std=given["aug_noise_std"] or 0.0, erase_prob=given["aug_erase_prob"] or 0.0,
                            erase_scale=tuple(given["aug_erase_scale"] or (0.1, 0.3)), erase_fill=fill, per_episode=not args.aug_per_frame,
                            seed=(given["aug_seed"] or 0) + rank, blur_prob=given["aug_blur_prob"] or 0.0,
                            blur_sigma=tuple(given["aug_blur_sigma"] or (0.5, 2.0)), motion_blur_prob=given["aug_motion_prob"] or 0.0,
                            motion_blur_max_length=9 if given["aug_motion_max_length"] is None else given["aug_motion_max_length"])
    except ValueError as e:
        raise SystemExit("--aug_*: %s" % e)


DEPTH_AUGMENT_FLAGS = ("aug_depth_noise", "aug_depth_drop_prob", "aug_depth_holes", "aug_depth_hole_scale", "aug_depth_hole_value", "aug_depth_quant",
                       "aug_depth_clamp", "aug_depth_occluder_value")


def build_depth_augment(args, rank=0, augment=None):
    """the --aug_depth_* family -> util.data_utils.DepthAugment, or None when none of its flags is given.  The flags need --use_depth
    (a model that reads depth) and --episodes (recorded depth frames); --aug_depth_share_erase needs --aug_erase_prob and takes
    `augment`, the FrameAugment of the same rank (build_augment).  --aug_per_frame and --aug_seed hold for depth as for RGB."""
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import DepthAugment
    given = {k: getattr(args, k, None) for k in DEPTH_AUGMENT_FLAGS}
    share = bool(getattr(args, "aug_depth_share_erase", False))
    if all(v is None for v in given.values()) and not share:
        return None
    if not getattr(args, "use_depth", False):
        raise SystemExit("the --aug_depth_* flags need --use_depth: without it the model does not read depth")
    if not getattr(args, "episodes", None):
        raise SystemExit("the --aug_depth_* flags need --episodes: the augmentation works on recorded depth frames")
    if share and (getattr(args, "aug_erase_prob", None) is None or augment is None):
        raise SystemExit("--aug_depth_share_erase needs --aug_erase_prob: it covers in depth the rectangle the RGB augmentation erases")
    noise = given["aug_depth_noise"] or [0.0]
    if len(noise) > 3:
        raise SystemExit("--aug_depth_noise takes one to three coefficients S0 [S1 [S2]]; got %d" % len(noise))
    try:
        return DepthAugment(noise=tuple(noise), drop_prob=given["aug_depth_drop_prob"] or 0.0, holes=tuple(given["aug_depth_holes"] or (0, 0)),
                            hole_scale=tuple(given["aug_depth_hole_scale"] or (0.02, 0.15)), hole_value=given["aug_depth_hole_value"] or 0.0,
                            quant=given["aug_depth_quant"] or 0.0, clamp=None if given["aug_depth_clamp"] is None else tuple(given["aug_depth_clamp"]),
                            occluder_value=given["aug_depth_occluder_value"] or 0.0, per_frame=bool(getattr(args, "aug_per_frame", False)),
                            seed=(getattr(args, "aug_seed", None) or 0) + rank, share_erase=augment if share else None)
    except ValueError as e:
        raise SystemExit("--aug_depth_*: %s" % e)


DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def build_model(args, compute_dtype):
    from rgb_proprioceptive_pose_estimator_amd import models as M
    num_resnet_layers, feature_layer_nums = getattr(args, "resnet_layers", 50), (9,)   # (--resnet_layers: scripts/visualize_features.py)
    assert args.model in MODELS, "Error: Invalid model specified. Options are: {}".format(MODELS)
    if args.model == 'n':
        return M.NaiveEndEffectorStateEstimator(hidden_dims_pre_measurement=args.hidden_dim, hidden_dims_post_measurement=args.hidden_dim,
                                                num_resnet_layers=num_resnet_layers, latent_dim=args.latent_dim,
                                                feature_extract=args.feature_extract, compute_dtype=compute_dtype)
    if args.model == 'no':
        return M.NaiveObjectStateEstimator(object_name=args.obj_name, hidden_dims=args.hidden_dim, num_resnet_layers=num_resnet_layers,
                                           latent_dim=args.latent_dim, feature_extract=args.feature_extract,
                                           feature_layer_nums=feature_layer_nums, use_depth=args.use_depth, use_pretrained=args.use_pretrained,
                                           no_proprioception=args.no_proprioception, compute_dtype=compute_dtype)
    common = dict(num_resnet_layers=num_resnet_layers, latent_dim=args.latent_dim, sequence_length=args.sequence_length,
                  feature_extract=args.feature_extract, feature_layer_nums=feature_layer_nums, use_depth=args.use_depth,
                  use_pretrained=args.use_pretrained, device="cuda", compute_dtype=compute_dtype)
    if args.model == 'td':
        return M.TemporallyDependentStateEstimator(hidden_dim_pre_measurement=args.hidden_dim[0], hidden_dim_post_measurement=args.hidden_dim[0], **common)
    if args.model == 'tdo':
        return M.TemporallyDependentObjectStateEstimator(object_name=args.obj_name, hidden_dim=args.hidden_dim[0],
                                                         no_proprioception=args.no_proprioception, **common)
    return M.TemporallyDependentObjectStateEstimatorV2(object_name=args.obj_name, img_hidden_dim=args.hidden_dim[0],
                                                       proprio_hidden_dim=args.proprio_hidden_dim, **common)


SCHEDULE_FLAGS = ("lr_schedule", "warmup_steps", "warmup_start_factor", "lr_total_steps", "lr_min_factor", "lr_step_size", "lr_gamma")
FUSED_ONLY_FLAGS = SCHEDULE_FLAGS + ("trunk_lr_scale", "ema_decay", "telemetry")


def build_schedule(args):
    """the --lr_schedule family -> optim.LRSchedule, or None when none of its flags is given (a warm-up alone is a constant schedule)"""
    from rgb_proprioceptive_pose_estimator_amd.optim import LRSchedule
    given = {k: getattr(args, k, None) for k in SCHEDULE_FLAGS}
    if all(v is None for v in given.values()):
        return None
    kind = given["lr_schedule"] or "constant"
    if kind == "cosine" and given["lr_total_steps"] is None:
        raise SystemExit("--lr_schedule cosine needs --lr_total_steps")
    if kind == "step" and given["lr_step_size"] is None:
        raise SystemExit("--lr_schedule step needs --lr_step_size")
    kw = dict(warmup_steps=given["warmup_steps"], warmup_start_factor=given["warmup_start_factor"], total_steps=given["lr_total_steps"],
              min_factor=given["lr_min_factor"], step_size=given["lr_step_size"], gamma=given["lr_gamma"])
    return LRSchedule(kind, **{k: v for k, v in kw.items() if v is not None})


def build_optimizer(args, params):
    """--optimizer / --max_grad_norm / --weight_decay / the schedule flags / --ema_decay -> FusedAdam, FusedAdamW, torch.optim.Adam or
    torch.optim.AdamW.  params: parameters, or group dicts (util.model_utils.lr_param_groups: a group's `lr_scale` becomes lr * scale)."""
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam, FusedAdamW
    if args.dtype == "f16" and args.optimizer != "fused":
        raise SystemExit("--dtype f16 needs --optimizer fused: the loss-scale unscale / skip logic lives in FusedAdam.step (amp.py)")
    if args.max_grad_norm is not None and args.optimizer != "fused":
        raise SystemExit("--max_grad_norm needs --optimizer fused: the on-device norm and clip live in FusedAdam.step (optim.py)")
    for flag in FUSED_ONLY_FLAGS:
        if getattr(args, flag, None) is not None and args.optimizer != "fused":
            raise SystemExit("--%s needs --optimizer fused: the on-device schedule, the per-group update, the weight average and the telemetry "
                             "pass live in FusedAdam.step (optim.py)" % flag)
    if getattr(args, "telemetry_out", None) is not None and getattr(args, "telemetry", None) is None:
        raise SystemExit("--telemetry_out needs --telemetry")
    params = list(params)
    if params and isinstance(params[0], dict):
        params = [dict({k: v for k, v in g.items() if k != "lr_scale"}, **({"lr": args.lr * g["lr_scale"]} if "lr_scale" in g else {})) for g in params]
    extra = {}
    schedule, ema_decay = build_schedule(args), getattr(args, "ema_decay", None)
    if schedule is not None:
        extra["lr_schedule"] = schedule
    if ema_decay is not None:
        extra["ema_decay"] = ema_decay
    if getattr(args, "telemetry", None) is not None:
        extra["telemetry"] = args.telemetry
    if args.optimizer == "fused":
        if args.weight_decay:
            return FusedAdamW(params, lr=args.lr, weight_decay=args.weight_decay, max_grad_norm=args.max_grad_norm, **extra)
        return FusedAdam(params, lr=args.lr, max_grad_norm=args.max_grad_norm, **extra)
    if args.weight_decay:
        return torch.optim.AdamW(params, lr=args.lr, weight_decay=args.weight_decay)
    return torch.optim.Adam(params, lr=args.lr)


def check_ragged(args, sampling):
    """--episodes with a `lengths` array (episodes of unequal length) trains from shuffled minibatches only: without --resident
    --batch_size the run stops here, before anything is built"""
    if not getattr(args, "episodes", None) or sampling:
        return
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset
    try:
        lengths = RecordedEpisodeDataset.file_lengths(args.episodes)
    except (OSError, ValueError):
        return   # (the dataset reports an unreadable file)
    if lengths is not None:
        raise SystemExit("{} holds episodes of unequal length: they train from shuffled minibatches, which never draw padding -- give "
                         "--resident --batch_size B".format(args.episodes))


def main(argv=None):
    args = build_parser().parse_args(argv)
    build_depth_augment(args, augment=build_augment(args))   # (a flag that cannot be honoured stops the run before anything is built)
    sampling = build_sampling(args)
    build_measurement_noise(args)
    apply_dropout(args)
    check_ragged(args, sampling)
    from rgb_proprioceptive_pose_estimator_amd.dist import init_from_env
    from rgb_proprioceptive_pose_estimator_amd.models import PoseDistanceLoss
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset, ResidentEpisodeDataset, SyntheticEpisodeDataset
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import train
    from rgb_proprioceptive_pose_estimator_amd.util.model_utils import lr_param_groups

    rank, world, local = init_from_env()
    if not torch.cuda.is_available():
        raise SystemExit("train_model.py: no MI355X visible; this path has no CPU fallback")
    torch.cuda.set_device(local)
    device = "cuda:%d" % local
    if rank == 0:
        print("*" * 20 + "\nRunning experiment:\n")
        for k, v in sorted(vars(args).items()):
            print("{}: {}".format(k, v))
        print("world size: {}\n".format(world) + "*" * 20)
    if args.model in ('no', 'tdo', 'tdo_v2') and args.obj_name is None:
        raise SystemExit("--obj_name is required for object-pose models (e.g. cube, hammer, robot1_eef)")
    crit = lambda: PoseDistanceLoss(distance_metric=args.distance_metric, scale_factor=args.loss_scale_factor, alpha=args.alpha, mode=args.loss_mode)
    criterion = {"x0_loss": crit(), "x1_loss": crit(), "obj_loss": crit(), "val_loss": PoseDistanceLoss(mode="val")}
    torch.manual_seed(0)
    model = build_model(args, DTYPES[args.dtype])
    if args.load_checkpoint:
        model.load_state_dict(torch.load(args.checkpoint_model_path, map_location="cpu"))
    apply_dropout(args, model, rank)
    optimizer = build_optimizer(args, lr_param_groups(model, args.trunk_lr_scale))
    if args.episodes:
        kw = dict(use_depth=args.use_depth, obj_name=args.obj_name, seed=args.episodes_seed + 1000 * rank)
        dataset = ResidentEpisodeDataset(args.episodes, device=device, **kw) if args.resident else RecordedEpisodeDataset(args.episodes, **kw)
        if args.horizon != build_parser().get_default("horizon") and args.horizon != dataset.env.horizon and rank == 0:
            warnings.warn("--horizon {} ignored: the episodes of {} have {} steps".format(args.horizon, args.episodes, dataset.env.horizon))
        args.horizon = dataset.env.horizon
    else:
        dataset = SyntheticEpisodeDataset(horizon=args.horizon, use_depth=args.use_depth, obj_name=args.obj_name, is_two_arm="TwoArm" in args.env,
                                          motion=args.motion, seed=args.episodes_seed + 1000 * rank, device=device, env_name=args.env)
    params = {"camera_name": args.camera_name, "noise_scale": args.noise_scale}
    if rank == 0:
        print("Training...")
    telemetry_log = [] if args.telemetry_out is not None else None
    augment = build_augment(args, rank)
    result = train(model=model, dataset=dataset, criterion=criterion, optimizer=optimizer, num_epochs=args.n_epochs,
                   num_train_episodes_per_epoch=args.n_train_episodes_per_epoch, num_val_episodes_per_epoch=args.n_val_episodes_per_epoch,
                   params=params, device=device, save_model=not args.no_save, augment=augment,
                   depth_augment=build_depth_augment(args, rank, augment), measurement_noise=build_measurement_noise(args, rank), telemetry=args.telemetry, telemetry_log=telemetry_log, **sampling)
    if telemetry_log and rank == 0:
        save_telemetry(args.telemetry_out, telemetry_log)
    return result


def save_telemetry(path, log):
    """--telemetry_out: `names` (T,) and one (epochs, T) array per figure of util.learn_utils.telemetry_report"""
    import numpy as np
    names = list(log[0])
    np.savez(path, names=np.array(names), **{k: np.array([[epoch[n][k] for n in names] for epoch in log], dtype=np.float64) for k in log[0][names[0]]})


if __name__ == "__main__":
    main()
