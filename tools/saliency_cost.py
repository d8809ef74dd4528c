"""Diagnostic (GPU box): what one occlusion-sensitivity map costs -- a 256 x 256 x 3 uint8 frame, rectangles of 32 x 32 every 16 pixels
(K = 225), NaiveObjectStateEstimator on ResNet-50 in bf16, chunks of B = 64 rows (4 forwards) -- split into its three parts, and the
same work done without the new kernels.  Timed in ONE process, the forms alternated block by block after a warm-up of all of them:

  (1)  occlude: the chunks' rpe_occlude_grid_u8 launches (ops.occlude_grid_u8 into a fixed buffer)
  (1t) the same batches by torch: the frame repeated, then one slice assignment per rectangle
  (2)  forwards: the chunks' eval-mode model calls on a prepared batch
  (3)  score + map + overlay: the chunks' rpe_pose_displacement launches, rpe_saliency_map, two rpe_saliency_overlay_u8
  (3h) the same on the host: the predictions copied back, the displacement in numpy float64, the map and the overlay in numpy
       (host clock around the call, which ends in the copy's synchronise)
  (all) util.model_utils.occlusion_sensitivity + render_saliency of both maps (the pictures copied to the host)

(1), (1t), (2), (3): blocks of `iters` back-to-back calls between HIP events; (3h), (all): host clock around `iters` calls and a device
synchronise.  Reported per form: the mean time of a call and the range of the block means.

A record, not a bar.  Writes profiles/saliency_cost.txt (or --out).

usage: python tools/saliency_cost.py [--iters N] [--blocks N] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rgb_proprioceptive_pose_estimator_amd import models as M, ops  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.util import model_utils as mu  # noqa: E402
from rgb_proprioceptive_pose_estimator_amd.util.data_utils import ERASE_FILL_MEAN  # noqa: E402

HS, PATCH, STRIDE, BATCH = 256, 32, 16, 64


def host_scores(pred, ref):
    p, r = pred.astype(np.float64), ref.astype(np.float64)
    pos = np.sqrt(((p[:, :3] - r[:3]) ** 2).sum(-1))
    a, b = p[:, 3:] / np.linalg.norm(p[:, 3:], axis=1, keepdims=True), r[3:] / np.linalg.norm(r[3:])
    dm, dp = np.linalg.norm(a - b, axis=1), np.linalg.norm(a + b, axis=1)
    return pos.astype(np.float32), (4.0 * np.arctan2(np.minimum(dm, dp), np.maximum(dm, dp))).astype(np.float32)


def host_map(scores, tops, lefts):
    acc, cnt = np.zeros((HS, HS), np.float32), np.zeros((HS, HS), np.float32)
    for gy, t in enumerate(tops):
        for gx, l in enumerate(lefts):
            acc[t:t + PATCH, l:l + PATCH] += scores[gy * len(lefts) + gx]
            cnt[t:t + PATCH, l:l + PATCH] += 1
    return acc / cnt


def host_overlay(frame, smap, table, alpha_q8):
    fin = np.isfinite(smap)
    if not fin.any():
        return frame.copy()
    lo, hi = smap[fin].min(), smap[fin].max()
    k = np.minimum(255, ((np.where(fin, smap, lo) - lo) / (hi - lo) * np.float32(256)).astype(np.int64)) if hi != lo else np.zeros(smap.shape, np.int64)
    out = ((frame.astype(np.int64) * (256 - alpha_q8) + table.astype(np.int64)[k] * alpha_q8 + 128) >> 8).astype(np.uint8)
    return np.where(fin[..., None], out, frame)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5, help="calls per timed block")
    ap.add_argument("--blocks", type=int, default=8, help="timed blocks per form, alternated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "saliency_cost.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("saliency_cost.py: no GPU visible; a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = M.NaiveObjectStateEstimator("cube", [1024, 256, 64], 50, 512, False, (9,), False, False, False, compute_dtype=torch.bfloat16).cuda().eval()
    frame = torch.randint(0, 256, (HS, HS, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8).to(dev)
    gy, gx, tops, lefts = mu.occlusion_grid(HS, HS, PATCH, STRIDE)
    k, b = gy * gx, min(BATCH, 1 + gy * gx)
    per = b - 1
    nchunks = -(-k // per)
    desc = ops.occlusion_desc(HS, HS, PATCH, PATCH, STRIDE, STRIDE, *ERASE_FILL_MEAN)
    batch = torch.empty((b, HS, HS, 3), dtype=torch.uint8, device=dev)
    x0bar = torch.zeros(b, 7, device=dev)
    x0bar[:, 6] = 1.0
    fill = torch.tensor(ERASE_FILL_MEAN, dtype=torch.uint8, device=dev)
    table = torch.from_numpy(np.ascontiguousarray(mu.colour_table())).to(dev)
    table_h, frame_h = table.cpu().numpy(), frame.cpu().numpy()

    def occlude():
        for c in range(nchunks):
            ops.occlude_grid_u8(frame, desc, b, c * per, out=batch)

    def occlude_torch():
        for c in range(nchunks):
            rows = frame.expand(b, HS, HS, 3).contiguous()
            for r in range(1, b):
                kk = c * per + r - 1
                if kk < k:
                    t, l = tops[kk // gx], lefts[kk % gx]
                    rows[r, t:t + PATCH, l:l + PATCH] = fill
        return rows

    with torch.no_grad():
        preds = []
        for c in range(nchunks):
            ops.occlude_grid_u8(frame, desc, b, c * per, out=batch)
            preds.append(model(batch, None, x0bar).reshape(b, 7).clone())
    assert torch.equal(occlude_torch(), batch)      # the forms build the same bytes
    dist = torch.empty((2, nchunks, b), dtype=torch.float32, device=dev)

    def forwards():
        with torch.no_grad():
            for c in range(nchunks):
                model(batch, None, x0bar)

    def score_device():
        for c in range(nchunks):
            ops.pose_displacement(preds[c], preds[0][0], pos=dist[0, c], ori=dist[1, c])
        scores = dist[:, :, 1:].reshape(2, nchunks * per)[:, :k].contiguous()
        maps, mm = ops.saliency_map(scores, desc)
        return [ops.saliency_overlay_u8(frame, maps[i], mm[i], table, 128, False) for i in (0, 1)]

    def score_host():
        p = torch.stack(preds).cpu().numpy()
        d = [host_scores(p[c], p[0, 0]) for c in range(nchunks)]
        out = []
        for i in (0, 1):
            s = np.concatenate([x[i][1:] for x in d])[:k]
            out.append(host_overlay(frame_h, host_map(s, tops, lefts), table_h, 128))
        return out

    def whole():
        res = mu.occlusion_sensitivity(model, frame, patch=PATCH, stride=STRIDE, batch=BATCH)
        return [mu.render_saliency(res, frame, kind) for kind in mu.SALIENCY_KINDS]

    def events(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return start.elapsed_time(stop) / args.iters

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / args.iters

    dev_pics, host_pics = score_device(), score_host()
    differ = [int((dev_pics[i].cpu().numpy() != host_pics[i]).sum()) for i in (0, 1)]
    forms = [("(1)  occlude, %d launches" % nchunks, lambda: events(occlude)), ("(1t) torch slice assignment", lambda: events(occlude_torch)),
             ("(2)  forwards, %d x batch %d" % (nchunks, b), lambda: events(forwards)), ("(3)  score + map + overlay", lambda: events(score_device)),
             ("(3h) the same on the host", lambda: clock(score_host)), ("(all) occlusion_sensitivity + 2 pictures", lambda: clock(whole))]
    for _ in range(2):
        for _, run in forms:
            run()
    times = {name: [] for name, _ in forms}
    for _ in range(args.blocks):
        for name, run in forms:
            times[name].append(run())
    lines = ["device: %s; one %dx%dx3 uint8 frame, rectangles %dx%d every %d pixels (K = %d), ResNet-50 bf16 (latent 512, hidden 1024-256-64), %d chunks of "
             "batch %d; %d blocks per form, alternated; %d calls per block" % (torch.cuda.get_device_name(0), HS, HS, PATCH, PATCH, STRIDE, k, nchunks, b,
                                                                               args.blocks, args.iters)]
    mean = {}
    for name, _ in forms:
        t = times[name]
        mean[name] = sum(t) / len(t)
        lines.append("%-42s %9.4f ms (%9.4f .. %9.4f)" % (name, mean[name], min(t), max(t)))
    m = [mean[name] for name, _ in forms]
    lines.append("(1) + (2) + (3) = %.4f ms: occlude %.2f %%, forwards %.2f %%, score + map + overlay %.2f %%" % (
        m[0] + m[2] + m[3], 100 * m[0] / (m[0] + m[2] + m[3]), 100 * m[2] / (m[0] + m[2] + m[3]), 100 * m[3] / (m[0] + m[2] + m[3])))
    lines.append("(1) / (1t) = %.4f   (3) / (3h) = %.4f   pixels where the host's fp32-accumulated pictures differ from the device's: %d, %d of %d" % (
        m[0] / m[1], m[3] / m[4], differ[0], differ[1], HS * HS * 3))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
