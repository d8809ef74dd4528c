#!/usr/bin/env python
"""Layer visualisation entry point (model side) on the MI355X path.

The reference's scripts/visualize_features.py steps a Robosuite simulator and, between steps, asks for a layer string and shows
that layer's output for the current camera frame (visualize_features.py:190-234, util/model_utils.py:10-107).  The simulator is out
of scope, so this script keeps what belongs to the model: the constructor flags (the simulator's are accepted and ignored, as in
rollout.py), loading a reference-format state_dict, `model.eval(); model.rollout = True; model.reset_initial_state(1)`, the prompt
(a one-letter answer `i` / `d` shows the raw frame / depth image), and the picture.  Frames come from `--frames FILE.npy` (uint8
(T, Hs, Ws, 3), staged by the trunk's resize / crop / normalise path) or from a seeded synthetic episode; `--layer tns` (repeatable)
replaces the prompt and `--out DIR` writes `DIR/<layer>.png` instead of opening a window.

`--saliency position|orientation|both` (addition; needs `--frames`) draws the occlusion-sensitivity map of the chosen frame over it
(util.model_utils.occlusion_sensitivity): `DIR/saliency_position.png` / `DIR/saliency_orientation.png`, and one line per map with its
range and its hottest rectangle.  With `--saliency` and no `--layer` there is no prompt.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rgb_proprioceptive_pose_estimator_amd.scripts.train_model import DTYPES, build_model, build_parser  # noqa: E402


def build_vis_parser():
    p = build_parser()
    p.add_argument("--model_path", type=str, default=None, help="state_dict .pth to load (reference key names)")
    p.add_argument("--frames", type=str, default=None, help=".npy of uint8 camera frames (T, Hs, Ws, 3); default: a seeded synthetic episode")
    p.add_argument("--depth", type=str, default=None, help=".npy of depth images for --use_depth: (T, H, W) or (T, 1, H, W) at the network's input size, or RAW float32 "
                   "(T, Hs, Ws) or (T, Hs, Ws, 1) with the geometry of --frames (resized and cropped on the device, as Pillow would)")
    p.add_argument("--frame", type=int, default=0, help="which frame of the episode to show")
    p.add_argument("--layer", action="append", default=None, help="layer string 'tns' (f9m, a0s, ..); repeatable; default: prompt")
    p.add_argument("--out", type=str, default=None, help="directory for <layer>.png; default: show with matplotlib")
    p.add_argument("--resnet_layers", type=int, default=50, help="depth of the ResNet trunk (18, 50, 101 or 152)")
    p.add_argument("--saliency", choices=["position", "orientation", "both"], default=None,
                   help="occlusion-sensitivity map of the frame (needs --frames): which pixels move the predicted position / orientation")
    p.add_argument("--patch", nargs="+", type=int, default=[32], help="--saliency: size of the covered rectangle, P or Py Px")
    p.add_argument("--stride", nargs="+", type=int, default=[16], help="--saliency: distance of the rectangles' origins, S or Sy Sx (at most the rectangle)")
    p.add_argument("--saliency_alpha", type=float, default=0.5, help="--saliency: weight of the map's colour over the frame, 0..1")
    p.add_argument("--saliency_fade", action="store_true", help="--saliency: the colour's weight grows with the value (cold regions show the frame)")
    p.add_argument("--measurements", type=str, default=None, help="--saliency: .npy (T, 7) of the robot's measured poses; default: the identity pose")
    p.add_argument("--truth", type=str, default=None, help="--saliency: .npy (T, 7) of true poses; the maps then show the change in ERROR, signed")
    return p


def build_saliency(args):
    """Checks the --saliency flags without touching a device -> None, or the keyword arguments of the maps"""
    if args.saliency is None:
        for flag in ("measurements", "truth"):
            if getattr(args, flag) is not None:
                raise SystemExit("--{} belongs to --saliency".format(flag))
        return None
    if not args.frames:
        raise SystemExit("--saliency needs --frames FILE.npy: the rectangles are defined on raw uint8 frames, and the synthetic episode is float images")
    for name in ("patch", "stride"):
        if len(getattr(args, name)) not in (1, 2):
            raise SystemExit("--{} takes one or two integers".format(name))
    if not 0.0 <= args.saliency_alpha <= 1.0:
        raise SystemExit("--saliency_alpha lies in [0, 1]")
    pair = lambda v: int(v[0]) if len(v) == 1 else (int(v[0]), int(v[1]))
    kinds = ("position", "orientation") if args.saliency == "both" else (args.saliency,)
    return dict(kinds=kinds, patch=pair(args.patch), stride=pair(args.stride), alpha=args.saliency_alpha, fade=args.saliency_fade)


def _pose_row(path, flag, frame, count):
    a = np.load(path)
    if a.ndim != 2 or a.shape[1] != 7 or a.shape[0] != count:
        raise SystemExit("--{}: expected a ({}, 7) array, got {}".format(flag, count, a.shape))
    return torch.from_numpy(np.ascontiguousarray(a[frame], dtype=np.float32))


def run_saliency(model, img, depth, sal, measurement, truth, out):
    """the --saliency maps of one frame: a PNG (or a window) and one line each"""
    from rgb_proprioceptive_pose_estimator_amd.util.model_utils import SALIENCY_KINDS, occlusion_grid, occlusion_sensitivity, visualize_saliency
    try:
        occlusion_grid(img.shape[0], img.shape[1], sal["patch"], sal["stride"])
    except ValueError as e:
        raise SystemExit("--patch / --stride: {}".format(e))
    res = occlusion_sensitivity(model, img, depth, measurement, patch=sal["patch"], stride=sal["stride"], truth=truth)
    for kind in sal["kinds"]:
        i = SALIENCY_KINDS.index(kind)
        visualize_saliency(model, img, which=kind, result=res, alpha=sal["alpha"], fade=sal["fade"],
                           out=None if out is None else os.path.join(out, "saliency_{}.png".format(kind)))
        lo, hi = res.minmax[i].tolist()
        s = torch.nan_to_num(res.scores[i], nan=float("-inf")).flatten()
        k = int(s.argmax())
        gy, gx = divmod(k, res.grid[1])
        top, left = min(gy * res.stride[0], img.shape[0] - res.patch[0]), min(gx * res.stride[1], img.shape[1] - res.patch[1])
        print("saliency {}: range [{:.6g}, {:.6g}] {}; hottest rectangle {} at (top {}, left {}), {}x{}: {:.6g}".format(
            kind, lo, hi, "rad" if i else "(pose units)", k, top, left, res.patch[0], res.patch[1], float(s[k])))
    return res


def _show_raw(image, name, out):
    """the prompt's one-letter answers: the raw frame / depth image, drawn as the reference draws them (row 0 at the bottom)"""
    print("Visualizing raw input {}...".format(name))
    a = np.asarray(image)
    if out is not None:
        from PIL import Image
        if a.dtype != np.uint8:
            lo, hi = float(a.min()), float(a.max())
            a = np.uint8(255 * (a - lo) / (hi - lo if hi > lo else 1.0))
        Image.fromarray(a[::-1].copy()).save(os.path.join(out, name + ".png"), format="PNG")
        return
    import matplotlib.pyplot as plt
    plt.axis("off")
    plt.imshow(a)
    plt.gca().invert_yaxis()
    plt.show()


def main(argv=None):
    args = build_vis_parser().parse_args(argv)
    sal = build_saliency(args)
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import synthetic_batch
    from rgb_proprioceptive_pose_estimator_amd.util.model_utils import visualize_layer

    np.random.seed(3)
    torch.manual_seed(3)
    if not torch.cuda.is_available():
        raise SystemExit("visualize_features.py: no MI355X visible; this path has no CPU fallback")
    model = build_model(args, DTYPES[args.dtype])
    if args.model_path:
        model.load_state_dict(torch.load(args.model_path, map_location=torch.device("cpu")))
    model.cuda().eval()
    model.rollout = True
    model.reset_initial_state(1)

    depth = raw_depth = None
    if args.frames:
        frames = np.load(args.frames)
        if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[-1] != 3:
            raise SystemExit("--frames: expected a uint8 (T, Hs, Ws, 3) array, got {} {}".format(frames.dtype, frames.shape))
        raw_img = frames[args.frame]
        img = torch.from_numpy(np.ascontiguousarray(raw_img)).cuda()
        if args.depth:
            d = np.load(args.depth)[args.frame]
            raw_depth = d[..., 0] if d.ndim == 3 and d.shape[-1] == 1 and d.shape[0] != 1 else d.reshape(d.shape[-2:])
            depth = torch.from_numpy(np.ascontiguousarray(raw_depth, dtype=np.float32)).cuda()
            if raw_depth.shape == tuple(model.trunk.crop_hw):
                depth = depth.view(1, 1, *raw_depth.shape)     # already at the network's input size
            elif raw_depth.shape == raw_img.shape[:2]:
                depth = depth.view(*raw_depth.shape, 1)        # raw, the frames' geometry: resized and cropped on the device like them
            else:
                raise SystemExit("--depth: frames of {}x{} are neither the network's input size nor the {}x{} of --frames".format(
                    *raw_depth.shape, *raw_img.shape[:2]))
    else:
        ep = synthetic_batch((args.horizon, 1), 3, with_depth=args.use_depth, noise_scale=args.noise_scale)
        img = ep["img"][args.frame, 0]
        raw_img = ((img - img.min()) / (img.max() - img.min()) * 255).byte().permute(1, 2, 0).cpu().numpy()
        if ep["depth"] is not None:
            depth = ep["depth"][args.frame]
            raw_depth = depth[0, 0].cpu().numpy()
    if args.use_depth and depth is None:
        raise SystemExit("--use_depth needs --depth FILE.npy beside --frames")
    if args.out:
        os.makedirs(args.out, exist_ok=True)

    def answers():
        if args.layer:
            yield from args.layer
            return
        if sal is not None:   # --saliency without --layer: no prompt
            return
        while True:
            try:
                s = input("Model layer to visualize: ")
            except EOFError:
                return
            if not s:
                return
            yield s

    for layer in answers():
        if len(layer) == 1:
            if layer == "i":
                _show_raw(raw_img, "image", args.out)
            elif raw_depth is None:
                print("no depth image in this episode")
            else:
                _show_raw(raw_depth, "depth", args.out)
            continue
        print("Visualizing Layer {}...".format(layer))
        visualize_layer(model, layer, img, depth, out=None if args.out is None else os.path.join(args.out, layer + ".png"))

    if sal is not None:
        measurement = None if args.measurements is None else _pose_row(args.measurements, "measurements", args.frame, len(frames)).cuda()
        truth = None if args.truth is None else _pose_row(args.truth, "truth", args.frame, len(frames)).cuda()
        run_saliency(model, img, depth, sal, measurement, truth, args.out)


if __name__ == "__main__":
    main()
