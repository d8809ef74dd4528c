"""Diagnostic (GPU box): what the rollout video costs -- 1000 frames of 256 x 256 x 3 uint8 (10 episodes of 100 steps), two pose sets
(truth and estimate: disc, three axes, a trail of 8) and the two error bars, rows flipped -- on the device and by a host loop.  Timed in
ONE process, the forms alternated block by block after a warm-up of all of them:

  (d)   device: rpe_project_poses once, then rpe_draw_poses_u8 in chunks of 256 frames, frames and pictures resident on the device
        (what util.learn_utils.render_episodes launches)
  (d1)  the draw alone as ONE launch over all 1000 frames
  (c)   a plain device copy of the same buffer (Tensor.copy_), for (d1)'s achieved bytes/s as a fraction of a copy's
  (h)   the host: the same poses projected with numpy in float64 and the same glyphs drawn frame by frame with PIL.ImageDraw on the same
        frames (ellipses, lines, rectangles; PIL's own rasterisation, so the pictures are like, not equal)
  (all) render_episodes from HOST frames with the pictures copied back to the host (host clock: includes both transfers)

(d), (d1), (c): blocks of `iters` back-to-back calls between HIP events; (h), (all): host clock around `iters` calls and a device
synchronise.  Reported per form: the mean time of a call and the range of the block means.  Bytes of (d1) and (c): the buffer read once
and written once.

A record, not a bar.  Writes profiles/overlay_cost.txt (or --out).

usage: python tools/overlay_cost.py [--iters N] [--blocks N] [--out FILE]"""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgb_proprioceptive_pose_estimator_amd import ops  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.util import learn_utils as lu  # noqa: E402

E, T, HS, WS, CHUNK, TRAIL, RADIUS, AXIS_WIDTH, AXIS_LEN = 10, 100, 256, 256, 256, 8, 4.0, 1.5, 0.05
CAMERA = np.array([[220.0, 0, 128, 0], [0, 220.0, 128, 0], [0, 0, 1.0, 0]])


def episodes(rng):
    """smooth random walks in front of the camera, a noisy copy as the estimate -> (truth, estimate) (E, T, 7) float32"""
    start = np.concatenate([rng.uniform(-0.3, 0.3, (E, 1, 2)), rng.uniform(0.9, 1.4, (E, 1, 1))], -1)
    pos = start + np.cumsum(rng.normal(0, 0.004, (E, T, 3)), 1)
    q = np.cumsum(rng.normal(0, 0.05, (E, T, 4)), 1) + np.array([0, 0, 0, 1.0])
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    truth = np.concatenate([pos, q], -1).astype(np.float32)
    est = truth + rng.normal(0, 0.01, truth.shape).astype(np.float32)
    return truth, est


def host_points(poses):
    """poses (n, 7) -> (n, 4, 2) float64 pixel coordinates of the centre and the three axis tips (NaN behind the camera)"""
    p, q = poses[:, :3].astype(np.float64), poses[:, 3:].astype(np.float64)
    a, b, c, d = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    R = np.stack([np.stack([1 - 2 * (b * b + c * c), 2 * (a * b - c * d), 2 * (a * c + b * d)], -1),
                  np.stack([2 * (a * b + c * d), 1 - 2 * (a * a + c * c), 2 * (b * c - a * d)], -1),
                  np.stack([2 * (a * c - b * d), 2 * (b * c + a * d), 1 - 2 * (a * a + b * b)], -1)], 1)      # (n, 3, 3): columns are the axes
    X = np.concatenate([p[:, None], p[:, None] + AXIS_LEN * R.transpose(0, 2, 1)], 1)                              # (n, 4, 3)
    h = X @ CAMERA[:, :3].T + CAMERA[:, 3]
    return np.where(h[..., 2:] > 2.0 ** -10, h[..., :2] / h[..., 2:], np.nan)


def host_render(frames, sets, colours, pos_err, ori_err):
    """the PIL loop: frames (E, T, HS, WS, 3) uint8 on the host -> pictures of the same shape"""
    from PIL import Image, ImageDraw
    pts = [host_points(s.reshape(-1, 7)).reshape(E, T, 4, 2) for s in sets]
    out = np.empty_like(frames)
    bar_px = max(1, HS // 32)
    for e in range(E):
        for t in range(T):
            im = Image.fromarray(frames[e, t])
            dr = ImageDraw.Draw(im)
            for g, colour in enumerate(colours):
                faint = tuple((c + 128) // 2 for c in colour)
                for k in range(min(TRAIL, t), 0, -1):
                    u, v = pts[g][e, t - k, 0]
                    if np.isfinite(u):
                        dr.ellipse([u - RADIUS / 2, v - RADIUS / 2, u + RADIUS / 2, v + RADIUS / 2], fill=faint)
            for g, colour in enumerate(colours):
                u, v = pts[g][e, t, 0]
                if not np.isfinite(u):
                    continue
                for k, axis in enumerate(ops.OVERLAY_AXIS_COLOURS):
                    tu, tv = pts[g][e, t, 1 + k]
                    if np.isfinite(tu):
                        dr.line([u, v, tu, tv], fill=tuple(axis), width=2)
                dr.ellipse([u - RADIUS, v - RADIUS, u + RADIUS, v + RADIUS], fill=tuple(colour))
            pic = np.asarray(im)[::-1].copy()
            band = pic[HS - 2 * bar_px:] >> 1
            band[:bar_px, :int(np.clip(pos_err[e, t] / 0.1 * WS, 0, WS))] = colours[-1]
            band[bar_px:, :int(np.clip(np.nan_to_num(ori_err[e, t]) / 0.5 * WS, 0, WS))] = lu.OVERLAY_ORI_BAR_COLOUR
            pic[HS - 2 * bar_px:] = band
            out[e, t] = pic
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10, help="calls per timed block of the device forms (the host forms: one call per block)")
    ap.add_argument("--blocks", type=int, default=6, help="timed blocks per form, alternated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_cost.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("overlay_cost.py: no GPU visible; a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    truth, est = episodes(rng)
    frames_h = torch.from_numpy(rng.integers(0, 256, (E, T, HS, WS, 3), dtype=np.uint8))
    frames = frames_h.to(dev)
    out = torch.empty_like(frames)
    n = E * T
    pos_err = torch.from_numpy(np.linalg.norm(est[..., :3] - truth[..., :3], axis=-1).astype(np.float32)).to(dev)
    ori_err = torch.from_numpy(rng.uniform(0, 0.4, (E, T)).astype(np.float32)).to(dev)
    ev = types.SimpleNamespace(poses=torch.from_numpy(est).to(dev), truth=torch.from_numpy(truth).to(dev), measurements=None, pos_err=pos_err, ori_err=ori_err,
                               noise_scales=None)
    sets = ("truth", "estimate")
    colours = [lu.OVERLAY_COLOURS[s] for s in sets]
    r_q4 = int(round(RADIUS * 16))
    styles = [ops.overlay_style(c, 256, r_q4, int(round(AXIS_WIDTH * 8)), ops.OVERLAY_AXIS_COLOURS, TRAIL, r_q4 // 2) for c in colours]
    poses = torch.stack([ev.truth.reshape(n, 7), ev.poses.reshape(n, 7)], 1).contiguous()
    cam = torch.from_numpy(CAMERA[None]).to(dev)
    cam_index = torch.zeros(n, dtype=torch.int32, device=dev)
    bar_px = max(1, HS // 32)
    flat, out_flat = frames.view(n, HS, WS, 3), out.view(n, HS, WS, 3)
    bar_colours = (colours[-1], lu.OVERLAY_ORI_BAR_COLOUR)

    def device():
        points, bars = ops.project_poses(poses, cam, cam_index, AXIS_LEN, pos_err.reshape(n), ori_err.reshape(n), 0.1, 0.5, WS)
        for i in range(0, n, CHUNK):
            ops.draw_poses_u8(flat[i:i + CHUNK], points, bars, styles, frames_per_episode=T, first=i, bar_px=bar_px, bar_colours=bar_colours, flip=True,
                              out=out_flat[i:i + CHUNK])

    points, bars = ops.project_poses(poses, cam, cam_index, AXIS_LEN, pos_err.reshape(n), ori_err.reshape(n), 0.1, 0.5, WS)

    def draw_once():
        ops.draw_poses_u8(flat, points, bars, styles, frames_per_episode=T, bar_px=bar_px, bar_colours=bar_colours, flip=True, out=out_flat)

    def copy():
        out.copy_(frames)

    pe_h, oe_h = pos_err.cpu().numpy(), ori_err.cpu().numpy()

    def host():
        return host_render(frames_h.numpy(), (truth, est), colours, pe_h, oe_h)

    def whole():
        return lu.render_episodes(ev, frames_h, CAMERA, draw=sets, chunk=CHUNK).cpu()

    def events(fn, iters):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / iters

    def clock(fn, iters=1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / iters

    # the forms draw the same thing: (d) equals (all) byte for byte; the host's pictures are PIL's rasterisation of the same glyphs
    device()
    same = torch.equal(out.cpu(), whole())
    host_pic = host()
    touched_dev = int((out.cpu().numpy() != frames_h.numpy()[:, :, ::-1]).any(-1).sum())
    touched_host = int((host_pic != frames_h.numpy()[:, :, ::-1]).any(-1).sum())
    forms = [("(d)   project + draw, %d chunks of %d" % (-(-n // CHUNK), CHUNK), lambda: events(device, args.iters)),
             ("(d1)  draw, one launch", lambda: events(draw_once, args.iters)), ("(c)   plain device copy", lambda: events(copy, args.iters)),
             ("(h)   host: numpy + PIL.ImageDraw", lambda: clock(host)), ("(all) render_episodes, host -> host", lambda: clock(whole))]
    for _, run in forms:
        run()
    times = {name: [] for name, _ in forms}
    for _ in range(args.blocks):
        for name, run in forms:
            times[name].append(run())
    nbytes = 2 * frames.numel()
    lines = ["device: %s; %d frames of %dx%dx3 uint8 (%d episodes x %d steps), 2 pose sets (disc r %.1f px, 3 axes of %.2f m, trail %d) + 2 error bars, rows "
             "flipped; %d blocks per form, alternated; %d calls per block (host forms: 1)" % (torch.cuda.get_device_name(0), n, HS, WS, E, T, RADIUS, AXIS_LEN, TRAIL,
                                                                                               args.blocks, args.iters)]
    mean = {}
    for name, _ in forms:
        t = times[name]
        mean[name] = sum(t) / len(t)
        lines.append("%-40s %10.4f ms (%10.4f .. %10.4f)" % (name, mean[name], min(t), max(t)))
    m = [mean[name] for name, _ in forms]
    lines.append("(d1): %.1f MB read + written in %.4f ms = %.3f TB/s; (c): %.3f TB/s; (d1) / (c) in bytes/s = %.3f" % (
        nbytes / 1e6, m[1], nbytes / m[1] / 1e9, nbytes / m[2] / 1e9, m[2] / m[1]))
    lines.append("(d) / (h) = %.5f   (all) / (h) = %.5f   per frame: (d) %.2f us, (h) %.2f us" % (m[0] / m[3], m[4] / m[3], 1e3 * m[0] / n, 1e3 * m[3] / n))
    lines.append("(d) equals (all) byte for byte: %s; pixels changed outside the flip: device %d, host %d of %d" % (same, touched_dev, touched_host, n * HS * WS))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
