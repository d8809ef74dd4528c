#!/usr/bin/env python
"""Layer visualisation entry point (model side) on the MI355X path.

The reference's scripts/visualize_features.py steps a Robosuite simulator and, between steps, asks for a layer string and shows
that layer's output for the current camera frame (visualize_features.py:190-234, util/model_utils.py:10-107).  The simulator is out
of scope, so this script keeps what belongs to the model: the constructor flags (the simulator's are accepted and ignored, as in
rollout.py), loading a reference-format state_dict, `model.eval(); model.rollout = True; model.reset_initial_state(1)`, the prompt
(a one-letter answer `i` / `d` shows the raw frame / depth image), and the picture.  Frames come from `--frames FILE.npy` (uint8
(T, Hs, Ws, 3), staged by the trunk's resize / crop / normalise path) or from a seeded synthetic episode; `--layer tns` (repeatable)
replaces the prompt and `--out DIR` writes `DIR/<layer>.png` instead of opening a window.
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
    return p


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


if __name__ == "__main__":
    main()
