"""Training loop of the pose estimators on the MI355X path.

Same signature, phases, criterion dict, statistics and checkpoint naming as train() of the reference
(util/learn_utils.py:21-255); what changes is underneath:
  * batches are time-major slices of data already resident in HBM when the dataset offers `chunk()`; a dataset with only
    the reference's `__getitem__` contract is stacked the way its DataLoader would and staged through pinned, double-buffered
    asynchronous copies (no per-tensor pageable .cuda(), util/learn_utils.py:75-76,130-138);
  * the per-step "val" metric is reduced on the device and only read back once per phase (the reference
    synchronises twice per step: models/losses.py:99-113 and util/learn_utils.py:182);
  * with torch.distributed initialised, episodes are sharded over ranks and the flat gradient buffer is
    SUM-all-reduced (RCCL) between backward and the optimizer step.
rollout() of the reference needs the simulator and is out of scope; its model side -- every episode
walked step by step, per-step position / orientation errors, their per-episode and overall statistics (util/learn_utils.py:
446-538) -- is `evaluate_episodes`: all episodes advance together as lanes of one batch and the errors stay on the device; its
recorded video (util/learn_utils.py:401-403, 462-504) is `render_episodes` / `write_video`: the poses drawn on the recorded frames.
"""
import contextlib
import copy
import os
import time
from datetime import datetime

import numpy as np
import torch
import torch.distributed as dist

from ..dist import GradSync, broadcast_parameters, shard_bounds
from .data_utils import FramePrefetcher, TrainInputs, model_batch, noisy_measurement, ragged_window_counts, window_counts


def _writer(logging):
    if not logging:
        return None
    try:
        from torch.utils.tensorboard import SummaryWriter
        return SummaryWriter()
    except Exception:  # tensorboard is optional here
        return None


def _host_chunks(dataset, horizon, seq, use_depth):
    """What `DataLoader(dataset, batch_size=S, shuffle=False)` yields for a reference-shaped dataset (util/learn_utils.py:75-76,
    util/data_utils.py:62-73): `dataset[t]` is the 6-tuple of all episodes at timestep t; S consecutive timesteps are stacked
    time-major (S, N, ...).  Fields the model never reads (the reference fills them with torch.empty garbage) are dropped here
    instead of being copied to the device."""
    for t0 in range(0, horizon, seq):
        items = [dataset[t] for t in range(t0, min(t0 + seq, horizon))]
        cols = list(zip(*items))
        stack = lambda c: torch.stack([torch.as_tensor(x) for x in c], 0)
        img, depth, x0bar, x0, x1, obj = cols
        yield (stack(img), stack(depth) if use_depth else None, stack(x0bar), stack(x0), stack(x1), stack(obj))


def _chunks(dataset, horizon, seq, use_depth):
    """Time-major device batches of one phase.  Datasets that keep their episodes in HBM offer `chunk(t0, S)` (the synthetic one
    does); any other dataset with the reference's contract -- `__len__`, `__getitem__(t)` -> 6-tuple of host tensors -- goes
    through pinned, double-buffered asynchronous staging (FramePrefetcher), replacing the reference's per-tensor synchronous
    pageable `.cuda()` (util/learn_utils.py:130-138)."""
    if hasattr(dataset, "chunk"):
        for t0 in range(0, horizon, seq):
            yield dataset.chunk(t0, min(seq, horizon - t0))
        return
    first = dataset[0][0]
    if torch.as_tensor(first).is_cuda:   # device-resident tensors behind a plain __getitem__: just stack
        yield from _host_chunks(dataset, horizon, seq, use_depth)
        return
    yield from FramePrefetcher(_host_chunks(dataset, horizon, seq, use_depth), torch.device("cuda", torch.cuda.current_device()))


def sampled_steps_per_epoch(num_episodes, world, horizon, sequence_length, stride, batch_size):
    """optimizer steps of one sampled `train` phase (train(batch_size=...)): every rank draws from its own shard of the episodes
    (dist.shard_bounds), and all take the step count of the SMALLEST shard -- its windows // batch_size -- so the collectives stay
    matched.  A function of the arguments alone: every rank computes the same number without communication."""
    steps = []
    for r in range(int(world)):
        lo, hi = shard_bounds(num_episodes, r, world)
        steps.append(window_counts(hi - lo, horizon, sequence_length, stride)[1] // int(batch_size))
    return min(steps)


def train_step(model, batch, criterion, optimizer, train_obj_pose, phase="train", grad_sync=None, valid=None):
    """One iteration of the reference's hot loop (util/learn_utils.py:152-184).  Returns device scalars
    (loss, pos_err, ori_err) -- nothing is synchronised to the host.
    valid (dataset.valid(t0, S) of episodes of unequal length; None: every sample counts): the mask of the samples that exist, of
    the outputs' leading shape; every criterion sums over those only."""
    img, depth, x0bar, x0, x1, obj = batch
    masked = {} if valid is None else {"valid": valid}   # (None: the criteria are called exactly as before)
    optimizer.zero_grad()
    with torch.set_grad_enabled(phase == "train"):
        if train_obj_pose:
            obj_out = model(img, depth, x0bar)
            loss = criterion["obj_loss"](obj_out, obj, **masked)
            pos_err, ori_err = criterion["val_loss"].forward_device(obj_out, obj, **masked)
        else:
            x0_out, x1_out = model(img, depth, x0bar)
            loss = criterion["x0_loss"](x0_out, x0, **masked) + criterion["x1_loss"](x1_out, x1, **masked)
            pos_err, ori_err = criterion["val_loss"].forward_device(x1_out, x1, **masked)
        if phase == "train":
            loss.backward()
            if grad_sync is not None:
                if grad_sync.staged:   # slices were launched under the backward (dist.GradSync.attach): just wait
                    grad_sync.finish()
                else:
                    grad_sync.all_reduce()
            optimizer.step()
    return loss.detach(), pos_err, ori_err


def _graph_keepalive(model):
    """What a captured graph has baked addresses of, beyond its own tensors: the trunk plans (native engine + workspace) that exist
    at capture time and the per-device weight-gradient scratch.  A later eager call may evict a plan from the trunk's LRU table or
    replace the scratch by a larger buffer; holding these references keeps the captured addresses alive for as long as the graph
    object lives (the eager path simply continues on its new buffers)."""
    from .. import ops
    return (list(model.trunk._plans.values()), list(ops._SCRATCH.values()))


class GraphedTrainStep:
    """One train step (forward -> loss -> on-device val metrics -> backward -> Adam) captured ONCE into a hipGraph and replayed.

    The step is ~330 kernel launches issued from Python + C++ through ctypes; replaying one graph removes the launch gaps on the
    device and the host work between them (HIP streams and graphs instead of a tracing compiler).  Everything a replay touches
    lives at a fixed address: the inputs are copied into static tensors, the trunk plan's workspace and the weight-gradient
    scratch are allocated before the capture, temporaries come from the graph's private pool, and the optimizer's step count is
    kept on the device (FusedAdam(capturable=True)).  Single-process only: with a process group the step stays eager (RCCL
    collectives inside a captured graph are not exercised here).

        step = GraphedTrainStep(model, criterion, optimizer, train_obj_pose=True, example_batch=batch)
        loss, pos_err, ori_err = step(batch)          # device scalars, valid until the next call
        step = GraphedTrainStep(model, criterion, optimizer, True, None, sampler=dataset.sampler(256))
        loss, pos_err, ori_err = step()               # every replay draws the next shuffled batch on the device
        step = GraphedTrainStep(..., sampler=dataset.sampler(256), measurement_noise=MeasurementNoise([0.001, 0.01]))
        loss, pos_err, ori_err = step()               # ... and fresh measurement noise on its true poses
    """

    def __init__(self, model, criterion, optimizer, train_obj_pose, example_batch, warmup=3, augment=None, sampler=None, measurement_noise=None,
                 depth_augment=None):
        if dist.is_initialized() and dist.get_world_size() > 1:
            raise RuntimeError("GraphedTrainStep is single-process; data-parallel steps run eagerly")
        if not getattr(optimizer, "capturable", False):
            raise RuntimeError("GraphedTrainStep needs FusedAdam(..., capturable=True): the step count must live on the device")
        self.model, self.criterion, self.optimizer, self.train_obj_pose = model, criterion, optimizer, train_obj_pose
        # The input stages (util.data_utils.TrainInputs) are part of the captured step, in front of the model: they read the static
        # inputs and write buffers of their own, `fed`, which is what the model is given.  Their step counters live on the device and
        # the captured launches advance them, so every replay draws afresh (the warm-up steps advance them too, the capture does not).
        # With a sampler the step BEGINS with its two launches, which write the sampler's own buffers: these are the static inputs,
        # `example_batch` may be None and __call__ takes no batch.
        inputs = TrainInputs(model, sampler=sampler, measurement_noise=measurement_noise, augment=augment, depth_augment=depth_augment)
        self.sampler, self.measurement_noise, self.augment, self.depth_augment = sampler, measurement_noise, augment, depth_augment
        if sampler is not None:   # (buffers(): no launch, the counter stays; views keep the buffers' addresses)
            self.static = model_batch(sampler.buffers(), model.requires_sequence)
        else:
            self.static = tuple(None if t is None else t.clone() for t in example_batch)
        self.fed = inputs.fed_like(self.static)

        def step():
            return train_step(model, inputs(self.static, out=self.fed), criterion, optimizer, train_obj_pose, "train", None)

        model.train()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):   # warm-up on a side stream: plans, workspaces and scratch buffers exist before the capture
            for _ in range(warmup):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = step()
        self.warmup_steps = warmup   # optimizer steps taken while building (the capture itself does not execute anything)
        self._keep = _graph_keepalive(model)

    def __call__(self, batch=None):
        if self.sampler is not None:
            if batch is not None:
                raise ValueError("a GraphedTrainStep with a sampler draws its own batches: call it without one")
        else:
            for dst, src in zip(self.static, batch):
                if dst is not None and dst is not src:   # (fill `self.static` in place to skip the copy)
                    dst.copy_(src, non_blocking=True)
        self.graph.replay()
        # The replay re-ran the captured weight-packing launch, the optimizer and the BN running-statistics updates behind the
        # host's back: every plan's cached weight copies (the BN-folded inference copies above all) are stale now, exactly as
        # after an eager step.  Bumping the trunk's weight version makes the next eval forward -- on this plan or any other --
        # re-fold before it runs.
        self.model.trunk.weights_changed()
        return self.out


class GraphedRolloutFrame:
    """One eval-mode rollout frame (BN folded into the convs, LSTM state carried in place on the device) as a hipGraph:
    the per-frame path of rollout() (util/learn_utils.py:322-323,342,446 of the reference) is launch-bound at batch 1."""

    def __init__(self, model, img, depth, x0bar, warmup=2, calibrate=8):
        self.model = model
        model.eval()
        self.img, self.x0bar = img.clone(), x0bar.clone()
        self.depth = None if depth is None else depth.clone()
        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calibrate):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / calibrate * 1e3

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        self.replay_ms = self.eager_ms = None
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(warmup):
                model(self.img, self.depth, self.x0bar)
            # A replay is worth it only where the runtime launches the graph cheaply: both forms are timed over `calibrate` frames and the
            # slower one is dropped (see below).  The eager frames come BEFORE the capture: the captured frame bakes in the addresses of
            # the carried LSTM state as the last eager frame left them.  (Like the warm-up frames they advance that state: the caller
            # starts its episode with reset_initial_state afterwards.)
            if calibrate > 0:
                self.eager_ms = timed(lambda: model(self.img, self.depth, self.x0bar))
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self.out = model(self.img, self.depth, self.x0bar)
        self._keep = _graph_keepalive(model)
        # On the round-3 boxes a captured frame that forks to the engine's second stream replayed in 0.56 ms in one process and in
        # 3.2 ms in the next (hipGraphLaunch itself 2.6 ms of host time; round 2's tree behaves the same there:
        # profiles/r03_rollout_latency.txt); the engine now keeps a captured inference frame on ONE stream (0.45 ms, reliably), and
        # this check stays as the guard: replay slower than the eager frame -> the eager frame serves.
        if calibrate > 0:
            self.graph.replay()
            self.replay_ms = timed(self.graph.replay)
            if self.replay_ms > self.eager_ms:
                self.graph = None
                self._keep = None

    @property
    def replaying(self):
        return self.graph is not None

    def __call__(self, img, depth, x0bar):
        if self.graph is None:   # (the eager frame measured faster than the replay on this box)
            dev = self.img.device
            with torch.no_grad():
                return self.model(img.to(dev, non_blocking=True), None if depth is None else depth.to(dev, non_blocking=True), x0bar.to(dev, non_blocking=True))
        self.img.copy_(img, non_blocking=True)
        self.x0bar.copy_(x0bar, non_blocking=True)
        if self.depth is not None:
            self.depth.copy_(depth, non_blocking=True)
        self.graph.replay()
        return self.out


def eval_chunk_length(max_frames, num_episodes):
    """timesteps per evaluator call: as many as keep one trunk batch within `max_frames` frames, at least one"""
    return max(1, int(max_frames) // int(num_episodes))


def sweep_measurements(x0, noise_scales, z):
    """x0 (..., 7) true poses, z a standard-normal draw of that shape -> (K, ..., 7): x0 + sqrt(s_k) z with the quaternion part
    renormalised, as RecordedEpisodeDataset.refresh_data makes a measurement (util/data_utils.py:162-167 of the reference).  The ONE
    draw serves every scale, so the scales differ in nothing but the scale; s = 0 gives the true pose back."""
    return torch.stack([noisy_measurement(x0, float(s), z) for s in noise_scales], 0)


def sweep_draw(num_episodes, horizon, noise_seed):
    """the (E, T, 7) standard-normal draw of a noise sweep (host generator, so a seed means the same numbers on every box)"""
    return torch.randn((int(num_episodes), int(horizon), 7), generator=torch.Generator().manual_seed(int(noise_seed)))


class EpisodeEvaluation:
    """What `evaluate_episodes` returns.  Device tensors, episode-major, with a leading K dimension when noise scales were swept:
        outputs (E, T, 7) raw model outputs        poses (E, T, 7) the same with a unit quaternion
        pos_err (E, T) metres                      ori_err (E, T) radians
        measurements (E, T, 7) what the heads were given as the own end-effector pose; truth (E, T, 7) the scored poses (no K)
    and host numbers (numpy float64; scalars, or (K,) in a sweep) read back in one transfer:
        pos_mean pos_std pos_max ori_mean ori_std ori_max, and per episode (E,) / (K, E): pos_episode_sum pos_episode_mean
        ori_episode_sum ori_episode_mean.
    `stats` is the raw table they are views of: (K, 2, 3 + 2 E) = [scale][pos | ori][rpe_error_stats layout].
    lengths: None, or for episodes of unequal length the numpy (E,) numbers of timesteps; every per-step entry at t >= lengths[e] is
    NaN and the host numbers run over the timesteps that exist (rpe_error_stats_ragged)."""

    def __init__(self, outputs, poses, pos_err, ori_err, stats, noise_scales=None, truth=None, measurements=None, lengths=None):
        stats = np.asarray(stats, dtype=np.float64)
        self.noise_scales = None if noise_scales is None else [float(s) for s in noise_scales]
        k = 1 if noise_scales is None else len(self.noise_scales)
        e = (stats.shape[-1] - 3) // 2
        if stats.shape != (k, 2, 3 + 2 * e):
            raise ValueError("stats must be (K, 2, 3 + 2 E); got %r for K = %d" % (stats.shape, k))
        self.outputs, self.poses, self.pos_err, self.ori_err, self.stats = outputs, poses, pos_err, ori_err, stats
        self.truth, self.measurements = truth, measurements
        self.lengths = None if lengths is None else np.asarray(lengths)
        pick = (lambda a: a[0]) if noise_scales is None else (lambda a: a)
        for i, name in enumerate(("pos", "ori")):
            setattr(self, name + "_mean", pick(stats[:, i, 0]))
            setattr(self, name + "_std", pick(stats[:, i, 1]))
            setattr(self, name + "_max", pick(stats[:, i, 2]))
            setattr(self, name + "_episode_sum", pick(stats[:, i, 3:3 + e]))
            setattr(self, name + "_episode_mean", pick(stats[:, i, 3 + e:]))

    def summary(self):
        """The lines rollout() of the reference prints (util/learn_utils.py:527-538): one per episode, then the evaluation totals; in a
        sweep, that block once per noise scale under a line naming the scale."""
        lines = []
        for k in range(self.stats.shape[0]):
            if self.noise_scales is not None:
                lines.append("noise scale {:g}:".format(self.noise_scales[k]))
            (pm, ps, _), (om, os_, _) = self.stats[k, 0, :3], self.stats[k, 1, :3]
            e = (self.stats.shape[-1] - 3) // 2
            for ep in range(e):
                lines.append("EPISODE COMPLETED -- Total Pos/Ori err: {:.3f} m / {:.3f} rad, Per-Step Err: {:.3f} m / {:.3f} rad".format(
                    self.stats[k, 0, 3 + ep], self.stats[k, 1, 3 + ep], self.stats[k, 0, 3 + e + ep], self.stats[k, 1, 3 + e + ep]))
            lines += ["", "*" * 90,
                      "EVALUATION COMPLETED -- Per-Step Pos Mean/Std Err: {:.5f} / {:.5f} m || Ori Mean/Std Err: {:.5f} / {:.5f} rad".format(pm, ps, om, os_),
                      "*" * 90]
        return "\n".join(lines)


def _repeat_rows(rows, lead, k):
    """feature rows of one trunk pass -> the rows of k copies of every lane: (S, N) lanes become (S, k N), scale-major within a
    timestep; a flat batch (B,) becomes (k B,), scale-major.  Same padded row layout as headops.new_rows."""
    cols, pad = rows.shape[1], rows.stride(0)
    if len(lead) == 2:
        buf = torch.zeros((lead[0], k, lead[1], pad), dtype=torch.float32, device=rows.device)
        buf[..., :cols].copy_(rows.unflatten(0, tuple(lead)).unsqueeze(1).expand(lead[0], k, lead[1], cols))
    else:
        buf = torch.zeros((k, lead[0], pad), dtype=torch.float32, device=rows.device)
        buf[..., :cols].copy_(rows.unsqueeze(0).expand(k, lead[0], cols))
    return buf.view(-1, pad)[:, :cols]


def evaluate_episodes(model, dataset, num_episodes, params, *, max_frames=256, noise_scales=None, noise_seed=0):
    """Score `num_episodes` episodes of `dataset` in one batched pass: the model side of the reference's rollout()
    (util/learn_utils.py:322-323,342,446-538) without its frame-at-a-time walk.  The E episodes advance together as E lanes,
    S = max(1, max_frames // E) timesteps per call (one trunk batch of S E frames; BN is folded in eval mode, so frames are
    independent, and in rollout mode the LSTM state is carried per lane between calls); models without a sequence take the S E
    frames as one flat batch.  The truth is `obj` for a model with `object_name`, otherwise `x1` against the last output, as in
    train().  Outputs go episode-major into one (E, T, 7) device buffer; after the last chunk ONE rpe_pose_errors launch gives the
    per-step errors, two rpe_error_stats launches their statistics, and one device -> host copy reads the scalars.
    noise_scales=[s_0 .. s_{K-1}]: the same frames scored under K measurement-noise scales -- the trunk runs ONCE per chunk, the heads
    run with K E lanes on the feature rows repeated K times and measurements `sweep_measurements(x0, scales, z)` with
    z = sweep_draw(E, T, noise_seed); every field of the result gains a leading K dimension.
    Episodes of unequal length (a dataset with `lengths`): all E lanes still advance over the padded horizon together -- a lane's output
    depends on its own frames only, and on earlier ones through the LSTM, so what a finished lane computes from padding reaches nothing
    that exists.  After the last chunk the per-step entries at t >= len_e are set to NaN (outputs, poses, pos_err, ori_err,
    measurements, truth), the statistics come from rpe_error_stats_ragged over the timesteps that exist, and the result has `lengths`.
    Single process, device only (no CPU fallback).  model.training / model.rollout are restored and the carried state is reset."""
    from .. import ops
    if dist.is_initialized() and dist.get_world_size() > 1:
        raise RuntimeError("evaluate_episodes is single-process")
    p0 = next(model.parameters())
    if not torch.cuda.is_available() or not p0.is_cuda:
        raise RuntimeError("evaluate_episodes(): the pose models run on the MI355X HIP path only (call model.cuda() first); there is no CPU fallback")
    E = int(num_episodes)
    scales = None if noise_scales is None else [float(s) for s in noise_scales]
    if scales is not None and (not scales or min(scales) < 0):
        raise ValueError("noise_scales must be a non-empty list of non-negative variances; got %r" % (noise_scales,))
    K = 1 if scales is None else len(scales)
    scores_obj = hasattr(model, "object_name")
    use_depth = model.use_depth if hasattr(model, "use_depth") else False
    if (scores_obj and getattr(dataset, "obj_name", "") is None) or (not scores_obj and not getattr(dataset, "is_two_arm", True)):
        raise ValueError("the dataset has no {} poses to score this model against".format("object" if scores_obj else "second-arm"))
    was_training, was_rollout = model.training, model.rollout
    dataset.refresh_data(E, params["camera_name"], params["noise_scale"])
    T = len(dataset)
    S = eval_chunk_length(max_frames, E)
    dev = p0.device
    outputs = torch.empty((K, E, T, 7), dtype=torch.float32, device=dev)
    truth = torch.empty((E, T, 7), dtype=torch.float32, device=dev)
    meas = torch.empty((K, E, T, 7), dtype=torch.float32, device=dev)
    z = None if scales is None else sweep_draw(E, T, noise_seed).to(dev)
    # The K E lanes get state tensors of their own: the module's carried (h, c) stay where they are -- a frame captured earlier
    # (GraphedRolloutFrame) has their addresses baked in -- and come back, zeroed, afterwards.
    carried = getattr(model, "_carried", None)
    if carried is not None:
        model._carried = {}
    model.eval()
    model.rollout = True
    model.reset_initial_state(K * E)
    try:
        with torch.no_grad():
            t0 = 0
            for img, depth, x0bar, x0, x1, obj in _chunks(dataset, T, S, use_depth):
                s = img.shape[0]
                target = obj if scores_obj else x1
                if target is None:
                    raise ValueError("the dataset has no {} poses for this model".format("object" if scores_obj else "second-arm"))
                truth[:, t0:t0 + s].copy_(target.transpose(0, 1))
                seq = model.requires_sequence
                if not seq:   # S E independent frames: one flat batch
                    img = img.reshape(s * E, *img.shape[2:])
                    depth = None if depth is None else depth.reshape(s * E, *depth.shape[2:])
                # measurements of this chunk, (K, s, E, 7): the dataset's, or the sweep's own
                xk = x0bar.unsqueeze(0) if scales is None else sweep_measurements(x0, scales, z[:, t0:t0 + s].transpose(0, 1))
                meas[:, :, t0:t0 + s].copy_(xk.transpose(1, 2))
                if scales is None:
                    out = model(img, depth, x0bar if seq else x0bar.reshape(s * E, 7))
                    out = out[-1] if isinstance(out, tuple) else out
                    outputs[0, :, t0:t0 + s].copy_(out.reshape(s, E, 7).transpose(0, 1))
                else:
                    lead, rows = model.features_only(img, depth)
                    if seq:   # lanes of a timestep: scale-major (k, e)
                        out = model.heads_only(_repeat_rows(rows, lead, K), (s, K * E), xk.permute(1, 0, 2, 3))
                        out = (out[-1] if isinstance(out, tuple) else out).reshape(s, K, E, 7).permute(1, 2, 0, 3)
                    else:
                        out = model.heads_only(_repeat_rows(rows, lead, K), (K * s * E,), xk)
                        out = (out[-1] if isinstance(out, tuple) else out).reshape(K, s, E, 7).permute(0, 2, 1, 3)
                    outputs[:, :, t0:t0 + s].copy_(out)
                t0 += s
            pos, ori, poses = ops.pose_errors(outputs, truth.unsqueeze(0).expand(K, E, T, 7).contiguous(), 1e-4, want_pose=True)
            lengths, n = getattr(dataset, "selected_lengths", None), None
            if lengths is not None:   # episodes of unequal length: padding becomes NaN, and the statistics never read it
                n = torch.from_numpy(lengths.astype(np.int32)).to(dev)
                pad = torch.arange(T, dtype=torch.int32, device=dev)[None, :] >= n[:, None]   # (E, T)
                for a in (pos, ori):
                    a.masked_fill_(pad, float("nan"))
                for a in (outputs, poses, meas):
                    a.masked_fill_(pad[None, :, :, None], float("nan"))
                truth.masked_fill_(pad[:, :, None], float("nan"))
            stats = torch.stack([torch.stack([ops.error_stats(pos[k], n), ops.error_stats(ori[k], n)]) for k in range(K)])
            stats = stats.cpu().numpy()   # the one device -> host read of the evaluation
    finally:
        model.train(was_training)
        model.rollout = was_rollout
        if carried is not None:
            model._carried = carried
        model.reset_initial_state(E)
    if scales is None:
        outputs, poses, pos, ori, meas = outputs[0], poses[0], pos[0], ori[0], meas[0]
    return EpisodeEvaluation(outputs, poses, pos, ori, stats, scales, truth=truth, measurements=meas, lengths=lengths)


# ---- rollout video: the estimate and the truth drawn on the recorded frames ------------------------------------------------------
# The reference records its videos inside the simulator (util/learn_utils.py:401-403, 462-504: an indicator object is moved to each
# estimated position and the camera is rendered again).  Here the poses of an EpisodeEvaluation are projected through the camera's
# matrix and drawn on the recorded uint8 frames, both on the device (rpe_project_poses, rpe_draw_poses_u8; DESIGN.md "Pose overlay").
OVERLAY_SETS = ("truth", "estimate", "measurement")
OVERLAY_COLOURS = {"truth": (40, 220, 40), "estimate": (255, 60, 200), "measurement": (90, 160, 255)}
OVERLAY_ORI_BAR_COLOUR = (255, 150, 0)     # the orientation-error bar; the position-error bar has the estimate's colour


def flip_camera_rows(P, Hs):
    """A camera matrix (..., 3 or 4, 4) given for the UPRIGHT picture of Hs rows -> the matrix for the picture as stored upside down
    (robosuite's frames; the reference writes img[::-1]): the row coordinate v becomes Hs - 1 - v, that is row 1 of the matrix
    becomes (Hs - 1) row 2 - row 1.  float64 numpy; the input is not changed."""
    P = np.array(P, dtype=np.float64)
    if P.ndim < 2 or P.shape[-1] != 4 or P.shape[-2] not in (3, 4):
        raise ValueError("a camera matrix is (3, 4) or (4, 4); got {}".format(P.shape))
    P[..., 1, :] = (int(Hs) - 1) * P[..., 2, :] - P[..., 1, :]
    return P


def _camera_matrices(camera, num_episodes, device):
    """camera (3|4, 4) or (E, 3|4, 4) -> (fp64 (C, 3, 4) on the device, whether there is one per episode)"""
    cam = camera if isinstance(camera, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(camera, dtype=np.float64)))
    if cam.dim() not in (2, 3) or cam.shape[-1] != 4 or cam.shape[-2] not in (3, 4) or not (cam.is_floating_point()):
        raise ValueError("camera must be a (3, 4) or (4, 4) matrix, or one per episode (E, ., 4); got {} {}".format(cam.dtype, tuple(cam.shape)))
    if cam.dim() == 3 and cam.shape[0] != num_episodes:
        raise ValueError("camera holds {} matrices for {} episodes".format(cam.shape[0], num_episodes))
    per_episode = cam.dim() == 3
    cam = cam.reshape(-1, cam.shape[-2], 4)[:, :3].to(device=device, dtype=torch.float64).contiguous()
    return cam, per_episode


def render_episodes(evaluation, frames, camera, *, draw=("truth", "estimate"), axis_len=0.05, radius=4.0, axis_width=1.5, trail=8, bars=True,
                    pos_full=0.1, ori_full=0.5, alpha=1.0, flip=True, colours=None, scale=0, chunk=256, out=None):
    """The rollout video: the poses of `evaluation` (an EpisodeEvaluation of E episodes of T steps) drawn on the recorded frames
    -> uint8 (E, T, Hs, Ws, 3) on the device.

    frames: the RAW uint8 frames (E, T, Hs, Ws, 3) the episodes were scored on, host or device; `chunk` frames at a time are moved and
    drawn, so a host array need not fit the device twice.  camera: the 3 x 4 matrix P with [u w, v w, w] = P [x, y, z, 1], u the column
    and v the row of the frame AS STORED (`flip_camera_rows` converts a matrix of the upright picture), as (3, 4) or (4, 4) -- the
    first three rows are used -- or one per episode (E, ., 4); numpy or tensor, used in fp64.
    draw: which of "truth", "estimate" (evaluation.poses), "measurement" to draw, in drawing order.  Each is a disc of `radius` pixels
    at the projected position, three axes of `axis_len` metres and `axis_width` pixels showing the orientation, and the positions of
    the `trail` steps before in the same episode, fainter.  bars: two bars along the bottom edge show the step's position error (full
    width at `pos_full` metres) and orientation error (`ori_full` radians).  alpha: opacity in [0, 1].  flip: write the rows bottom
    up, so that frames stored upside down come out upright.  colours: {set name: (r, g, b)} replacing OVERLAY_COLOURS.  scale: which
    noise scale of a sweep.  out: destination, uint8 (E, T, Hs, Ws, 3) on the device, not overlapping `frames`.
    One rpe_project_poses launch for all steps, then one rpe_draw_poses_u8 launch per chunk, on the current stream; nothing is
    synchronised and nothing of the evaluation is changed.  Device only (no CPU fallback)."""
    from .. import ops
    sets = tuple(draw)
    if not sets or len(sets) != len(set(sets)) or any(s not in OVERLAY_SETS for s in sets):
        raise ValueError("draw lists one or more of {}, each once; got {!r}".format(", ".join(OVERLAY_SETS), draw))
    swept = evaluation.noise_scales is not None
    k = int(scale)
    if not 0 <= k < (len(evaluation.noise_scales) if swept else 1):
        raise ValueError("scale {!r}: the evaluation holds {} noise scale(s)".format(scale, len(evaluation.noise_scales) if swept else 1))
    pick = (lambda t: t[k]) if swept else (lambda t: t)
    source = {"truth": evaluation.truth, "estimate": pick(evaluation.poses),
              "measurement": None if evaluation.measurements is None else pick(evaluation.measurements)}
    for s in sets:
        if source[s] is None:
            raise ValueError("the evaluation holds no {} poses".format(s))
    dev = evaluation.poses.device
    E, T = source[sets[0]].shape[:2]
    if isinstance(frames, np.ndarray):
        frames = torch.from_numpy(frames)
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[-1] != 3:
        raise ValueError("render_episodes draws on RAW uint8 frames (E, T, Hs, Ws, 3), not on resized or normalised images; got {} {}".format(
            getattr(frames, "dtype", type(frames)), tuple(getattr(frames, "shape", ()))))
    if tuple(frames.shape[:2]) != (E, T):
        raise ValueError("frames of {} episodes x {} steps for an evaluation of {} x {}".format(frames.shape[0], frames.shape[1], E, T))
    if frames.is_cuda and frames.device != dev:
        raise ValueError("frames on {} and the evaluation on {}".format(frames.device, dev))
    Hs, Ws = frames.shape[2:4]
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError("alpha lies in [0, 1]; got {!r}".format(alpha))
    if not (float(radius) >= 0 and float(axis_width) >= 0):
        raise ValueError("radius and axis_width are not negative; got {!r}, {!r}".format(radius, axis_width))
    if int(chunk) < 1:
        raise ValueError("chunk must be at least 1; got {!r}".format(chunk))
    colour = dict(OVERLAY_COLOURS)
    for name, c in (colours or {}).items():
        if name not in OVERLAY_SETS:
            raise ValueError("colours: {!r} is none of {}".format(name, ", ".join(OVERLAY_SETS)))
        colour[name] = c
    r_q4 = int(round(float(radius) * 16))
    styles = [ops.overlay_style(colour[s], int(round(float(alpha) * 256)), r_q4, int(round(float(axis_width) * 8)), ops.OVERLAY_AXIS_COLOURS, int(trail),
                                r_q4 // 2) for s in sets]
    cam, per_episode = _camera_matrices(camera, E, None)
    if dev.type != "cuda":
        raise RuntimeError("render_episodes(): the overlay runs on the MI355X HIP path only; there is no CPU fallback")
    cam = cam.to(dev)
    n = E * T
    cam_index = (torch.arange(n, dtype=torch.int32, device=dev) // T) if per_episode else torch.zeros(n, dtype=torch.int32, device=dev)
    poses = torch.stack([source[s].reshape(n, 7) for s in sets], dim=1).to(torch.float32).contiguous()
    bar_px = max(1, Hs // 32) if bars and Hs >= 2 else 0
    errs = (pick(evaluation.pos_err).reshape(n).contiguous(), pick(evaluation.ori_err).reshape(n).contiguous()) if bar_px else (None, None)
    points, bar_len = ops.project_poses(poses, cam, cam_index, axis_len, errs[0], errs[1], pos_full, ori_full, Ws if bar_px else 0)
    shape = (E, T, Hs, Ws, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != dev or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 {} tensor on {}".format(shape, dev))
    if frames.is_cuda:
        lo, hi = frames.data_ptr(), frames.data_ptr() + frames.numel()
        if out.data_ptr() < hi and lo < out.data_ptr() + out.numel():
            raise ValueError("out overlaps frames: the frames are read while the output is written")
    flat, out_flat = frames.reshape(n, Hs, Ws, 3), out.view(n, Hs, Ws, 3)
    bar_colours = (colour["estimate"] if "estimate" in sets else colour[sets[0]], OVERLAY_ORI_BAR_COLOUR)
    for i in range(0, n, int(chunk)):
        src = flat[i:i + int(chunk)]
        src = (src if src.is_cuda else src.to(dev, non_blocking=True)).contiguous()
        ops.draw_poses_u8(src, points, bar_len, styles, frames_per_episode=T, first=i, bar_px=bar_px, bar_colours=bar_colours, flip=flip,
                          out=out_flat[i:i + src.shape[0]])
    return out


def write_video(frames, path, fps=10, lengths=None):
    """Write uint8 frames (..., Hs, Ws, 3) -- all leading dimensions are the frames in order, as render_episodes returns them -- to
    `path`: `.npy` holds the raw (N, Hs, Ws, 3) array, `.gif` an animation at `fps` frames a second (Pillow).
    lengths (E,): the frames are (E, T, Hs, Ws, 3) and episode e has lengths[e] of them; frames [lengths[e], T) are padding and are
    dropped before writing."""
    ext = os.path.splitext(str(path))[1].lower()
    if ext not in (".npy", ".gif"):
        raise ValueError("write_video writes .npy (the raw array) or .gif; got {!r}".format(path))
    if not float(fps) > 0:
        raise ValueError("fps must be positive; got {!r}".format(fps))
    arr = frames.detach().cpu().numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
    if arr.dtype != np.uint8 or arr.ndim < 4 or arr.shape[-1] != 3 or arr.size == 0:
        raise ValueError("frames must be uint8 (..., Hs, Ws, 3); got {} {}".format(arr.dtype, arr.shape))
    if lengths is not None:
        n = np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths)
        if arr.ndim != 5 or n.shape != arr.shape[:1] or n.dtype.kind not in "iu" or (n < 0).any() or (n > arr.shape[1]).any() or n.sum() == 0:
            raise ValueError("write_video(lengths=...) takes frames (E, T, Hs, Ws, 3) and E integers in [0, T], not all 0; got frames {} and lengths {}".format(
                arr.shape, n.tolist() if n.ndim == 1 and n.size <= 16 else n.shape))
        arr = np.concatenate([arr[e, :int(k)] for e, k in enumerate(n)], 0)
    arr = np.ascontiguousarray(arr.reshape((-1,) + arr.shape[-3:]))
    if ext == ".npy":
        with open(path, "wb") as f:
            np.save(f, arr)
        return path
    from PIL import Image
    pics = [Image.fromarray(a, "RGB") for a in arr]
    pics[0].save(path, format="GIF", save_all=True, append_images=pics[1:], duration=max(1, int(round(1000.0 / float(fps)))), loop=0)
    return path


def _telemetry_host(optimizer):
    """param_stats (row-major) followed by the schedule's factor (1 without a schedule), as one fp64 device vector"""
    stats = optimizer.param_stats
    if stats is None:
        raise RuntimeError("telemetry: the optimizer has not measured yet (FusedAdam(telemetry=K), after the first step)")
    f = optimizer.lr_factor
    return torch.cat([stats.reshape(-1), torch.ones(1, dtype=torch.float64, device=stats.device) if f is None else f.double().reshape(1)])


def telemetry_report(optimizer, model, host=None):
    """The last measured step of FusedAdam(telemetry=K) per parameter name -> {name: {grad_norm, weight_norm, grad_max, weight_max,
    zero_frac, nonfinite, first_nonfinite_step, update_ratio, step}}, in the order of optimizer.param_stats_names(model).  ONE
    device-to-host copy (which synchronises); `host`: that copy when the caller already made it (train() folds it into the phase's
    one read), a sequence of T * COLS + 1 numbers.
    grad_norm / weight_norm: l2 norms over the tensor's finite elements; zero_frac: the share of gradient elements that are +-0 (a
    dead tensor: 1); nonfinite: inf / NaN elements of the gradient plus those of the weights; first_nonfinite_step: the first
    measured step that saw any (0: never; sticky until optimizer.reset_param_stats()); step: the optimizer step measured.
    update_ratio = lr_eff ||d|| / ||p||, lr_eff the param group's lr times the schedule's factor of that step and d = m_hat / (sqrt(v_hat)
    + eps) the Adam direction of the update just applied.  It is the ADAM TERM ONLY: with weight decay the step also shrinks p by
    lr_eff weight_decay p, which is not included; a clipped step is (d is formed from the moments the clipped gradient went into).
    A skipped fp16 step reports 0; a tensor of norm 0 reports inf (or NaN when nothing moved either)."""
    from .._lib import PARAM_STATS_COLS
    names = optimizer.param_stats_names(model)
    if host is None:
        host = _telemetry_host(optimizer).cpu()
    host = np.asarray(host, dtype=np.float64)
    table, factor = host[:-1].reshape(len(names), PARAM_STATS_COLS), float(host[-1])
    numel = {n: p.numel() for n, p in model.named_parameters()}
    report = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for name, row, k in zip(names, table, optimizer.param_stats_groups()):
            lr_eff = optimizer.param_groups[k]["lr"] * factor
            report[name] = dict(grad_norm=float(np.sqrt(row[0])), weight_norm=float(np.sqrt(row[1])), grad_max=float(row[3]), weight_max=float(row[4]),
                                zero_frac=float(row[6] / max(1, numel[name])), nonfinite=int(row[5] + row[7]), first_nonfinite_step=int(row[9]),
                                update_ratio=float(lr_eff * np.sqrt(row[2]) / np.sqrt(row[1])), step=int(row[8]))
    return report


def train(model, dataset, criterion, optimizer, num_epochs, num_train_episodes_per_epoch, num_val_episodes_per_epoch, params, device,
          save_path='default', save_model=True, logging=True, *, save_optimizer=False, augment=None, batch_size=None, window_stride=None,
          shuffle_seed=0, measurement_noise=None, telemetry=None, telemetry_log=None, depth_augment=None):
    """See the module docstring.  Returns (model with the best validation weights, best validation loss).
    save_optimizer (addition; the reference saves weights only): also write `<save_path>.optim` with the optimizer state of the
    best-validation epoch so that a run can be resumed (`optimizer.load_state_dict(torch.load(path))`).
    An optimizer with a weight average (FusedAdam(ema_decay=...)): the `val` phase runs on the AVERAGED weights, so the best
    validation loss is theirs, and beside `<save_path>` (the raw weights, unchanged: a resume with `.optim` continues exactly)
    `<save_path>.ema` holds model.state_dict() with the averaged weights -- reference-shaped, so scripts/rollout.py
    --checkpoint_model_path X.ema loads it as it is.  BatchNorm's running statistics are not averaged: `.ema` carries those of the
    raw run.  With a schedule (lr_schedule=...) the per-epoch train line shows the current rate of the first param group.
    augment (util.data_utils.FrameAugment): applied on the device to the raw uint8 frames of the `train` phase, between their staging
    copy and the model; the `val` phase sees the recorded pixels.  Needs a dataset of raw frames (RecordedEpisodeDataset): with
    preprocessed float images it is a ValueError.
    batch_size (default None: the lockstep walk, one chunk of every selected episode per step): the `train` phase draws shuffled
    minibatches of `batch_size` windows of S = model.sequence_length (or 1) timesteps from the selected episodes instead
    (dataset.sampler: util.data_utils.ResidentEpisodeDataset / WindowSampler), window starts `window_stride` apart (default S), under
    seed `shuffle_seed` + rank; an epoch takes sampled_steps_per_epoch(...) optimizer steps and its averages divide by
    steps * batch_size * S frames per rank.  The `val` phase is unchanged.  A dataset without `sampler` is a ValueError.
    measurement_noise (util.data_utils.MeasurementNoise): in the `train` phase the model is fed measurement_noise(x0), drawn on the
    device afresh at every step, in place of the dataset's x0bar (drawn on the host once per refresh); it needs the batch's x0 rows
    only, so every dataset takes it.  The `val` phase keeps the dataset's measurements, and the dataset's own pool is not written.
    depth_augment (util.data_utils.DepthAugment): applied on the device to the depth frames of the `train` phase; the `val` phase sees
    the recorded depth and the dataset's own depth is not written.  A ValueError for a model without use_depth, or when its
    share_erase names a FrameAugment that is not the `augment` of this call.
    These stages and the sampler run as one util.data_utils.TrainInputs, which validates them and fixes their order.
    telemetry (None or K >= 1; needs FusedAdam(telemetry=K) with the same K): at the end of every `train` phase the optimizer's
    per-tensor table of the last measured step is read WITH the phase's one host read (no synchronisation per step is added) and
    written as Telemetry/grad_norm/<name>, Telemetry/update_ratio/<name>, Telemetry/zero_frac/<name>; when a tensor has seen
    non-finite values, one line names the first one and its step.  telemetry_log: a list that receives every epoch's
    telemetry_report(...).  The `val` phase is untouched.
    A dataset of episodes of unequal length (a file with `lengths`): the `val` phase walks the padded horizon in lockstep as ever, gives
    every criterion dataset.valid(t0, S) and divides the epoch sums by the number of timesteps that exist; the `train` phase needs
    batch_size, the device sampler, which never draws padding (the lockstep walk would feed padded frames into the batch statistics of
    train-mode BatchNorm: a ValueError), and takes num_windows // batch_size steps of the current selection.  Under a process group
    such a dataset is a ValueError: the shards' window counts can no longer be computed without communication."""
    if telemetry is not None and getattr(optimizer, "telemetry", None) != telemetry:
        raise ValueError("train(telemetry={!r}) needs an optimizer built with the same option (optim.FusedAdam(..., telemetry={!r})); got {} with telemetry={!r}".format(
            telemetry, telemetry, type(optimizer).__name__, getattr(optimizer, "telemetry", None)))
    if telemetry is None and telemetry_log is not None:
        raise ValueError("train(telemetry_log=...) belongs to telemetry=K")
    # the device stages of the `train` phase, validated here: before the model, the optimizer or the device are touched
    inputs = TrainInputs(model, dataset, measurement_noise=measurement_noise, augment=augment, depth_augment=depth_augment)
    if batch_size is not None and not hasattr(dataset, "sampler"):
        raise ValueError("train(batch_size=...) draws minibatches on the device and needs a dataset with sampler() (ResidentEpisodeDataset); "
                         "{} has none".format(type(dataset).__name__))
    if batch_size is None and (window_stride is not None or shuffle_seed != 0):
        raise ValueError("train(window_stride=..., shuffle_seed=...) belong to batch_size=...; without it the episodes are walked in lockstep")
    ragged = getattr(dataset, "lengths", None) is not None
    if ragged and batch_size is None:
        raise ValueError("episodes of unequal length train from shuffled minibatches only: give train(batch_size=...) with a ResidentEpisodeDataset "
                         "(scripts/train_model.py --resident --batch_size B); the lockstep walk would feed padded frames into BatchNorm's batch statistics")
    if ragged and dist.is_initialized() and dist.get_world_size() > 1:
        raise ValueError("episodes of unequal length under a process group are not built: the ranks' shards hold different numbers of windows, "
                         "so the common step count cannot be computed without communication")
    if ragged:   # the first `train` selection is known already: refuse a batch it cannot fill here, before the device is touched
        s0 = model.sequence_length if model.requires_sequence else 1
        m0 = ragged_window_counts(dataset.peek_lengths(num_train_episodes_per_epoch), s0, s0 if window_stride is None else window_stride)[1]
        if m0 < int(batch_size):
            raise ValueError("a batch of {} windows needs at least as many windows; the {} episodes of the first train phase hold {} "
                             "(sequence_length {}, stride {})".format(batch_size, num_train_episodes_per_epoch, m0, s0, s0 if window_stride is None else window_stride))
    train_obj_pose = hasattr(model, "object_name")
    dt_string = datetime.now().strftime("%d-%m-%Y_%H-%M-%S")
    since = time.time()
    best_model = copy.deepcopy(model.state_dict())
    best_err = np.inf
    has_ema = getattr(optimizer, "ema_decay", None) is not None
    scheduled = getattr(optimizer, "lr_schedule", None) is not None
    rank = dist.get_rank() if dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_initialized() else 1
    writer = _writer(logging and rank == 0)
    if device == "cpu":
        raise RuntimeError("train(): the pose train step runs on the MI355X HIP path only (device='cuda:N'); there is no CPU fallback")
    model.cuda()
    # Build the flat parameter arena now, so replicas can be made identical and the gradient reduction attached BEFORE the
    # first optimizer step (Adam moments would otherwise diverge between ranks).
    model._materialize(torch.device("cuda", torch.cuda.current_device()))
    grad_sync = None
    if world > 1:
        broadcast_parameters(model._arena.flat, list(model.buffers()))
        grad_sync = GradSync(model._arena.grad).attach(model)
    seq = model.sequence_length if model.requires_sequence else 1
    fname = "{}_{}_{}hzn_{}ep_{}.pth".format(type(model).__name__, type(dataset.env).__name__, dataset.env.horizon,
                                             num_epochs * num_train_episodes_per_epoch, dt_string)
    if save_model and rank == 0:
        print("\nFile name saved:\n{}\n".format(fname))
    for epoch in range(num_epochs):
        if logging and rank == 0:
            print("\n" + "-" * 10 + "\nEpoch {}/{}\n".format(epoch, num_epochs - 1) + "-" * 10)
        for phase in ["train", "val"]:
            num_episodes = num_train_episodes_per_epoch if phase == "train" else num_val_episodes_per_epoch
            model.train() if phase == "train" else model.eval()
            lo, hi = shard_bounds(num_episodes, rank, world)
            dataset.refresh_data(hi - lo, params["camera_name"], params["noise_scale"])
            model.reset_initial_state(hi - lo)
            sums = torch.zeros(3, dtype=torch.float64, device="cuda")
            # gradient clipping on (FusedAdam(max_grad_norm=...)): the norm of every step and the count of clipped ones, on the device
            clip_sums = torch.zeros(2, dtype=torch.float64, device="cuda") if phase == "train" and getattr(optimizer, "max_grad_norm", None) is not None else None
            clip_steps = 0
            horizon = len(dataset)
            ema_sd = None
            sampled = batch_size is not None and phase == "train"
            if sampled:
                if inputs.sampler is None:   # made after the first `train` refresh: it reads the number of selected episodes
                    inputs.draw_from(dataset.sampler(batch_size, sequence_length=seq, stride=window_stride, shuffle=True, seed=shuffle_seed + rank))
                if ragged:   # (single process) the windows of THIS selection; fewer than a batch is the sampler's ValueError
                    inputs.sampler.check_windows()
                    steps = inputs.sampler.steps_per_epoch
                else:
                    steps = sampled_steps_per_epoch(num_episodes, world, horizon, seq, inputs.sampler.stride, batch_size)
                if steps < 1:
                    raise ValueError("the smallest shard of {} episodes over {} ranks has fewer than batch_size = {} windows".format(num_episodes, world, batch_size))
                model.reset_initial_state(batch_size)
                batches = (None for _ in range(steps))   # `inputs` draws them
            else:
                batches = (model_batch(b, model.requires_sequence) for b in _chunks(dataset, horizon, seq, getattr(model, "use_depth", False)))
            masks = None   # episodes of unequal length, walked in lockstep (`val`): which samples of every chunk exist
            if ragged and not sampled:
                masks = (model_batch((dataset.valid(t0, min(seq, horizon - t0)),), model.requires_sequence)[0] for t0 in range(0, horizon, seq))
            with optimizer.averaged_weights(model) if phase == "val" and has_ema else contextlib.nullcontext():   # validate the average
                for batch in batches:
                    if phase == "train":   # new tensors: what the dataset handed out is not written
                        batch = inputs(batch)
                    loss, pe, oe = train_step(model, batch, criterion, optimizer, train_obj_pose, phase, grad_sync,
                                              valid=None if masks is None else next(masks))
                    sums += torch.stack([loss.double(), pe.double(), oe.double()])
                    if clip_sums is not None:
                        clip_sums += torch.stack([optimizer.grad_norm.double(), (optimizer.clip_coef < 1.0).double()])
                        clip_steps += 1
                if world > 1:
                    dist.all_reduce(sums)
                stats = [sums] + ([] if clip_sums is None else [clip_sums])
                if phase == "train" and scheduled and optimizer.lr_factor is not None:
                    stats.append(optimizer.lr_factor.double().reshape(1))
                measured = phase == "train" and telemetry is not None and optimizer.param_stats is not None
                if measured:
                    n_head = sum(s.numel() for s in stats)
                    stats.append(_telemetry_host(optimizer))
                tot = (sums if len(stats) == 1 else torch.cat(stats)).tolist()  # the one host synchronisation of the phase
                tele = None
                if measured:
                    tot, tele = tot[:n_head], telemetry_report(optimizer, model, tot[n_head:])
                denom = steps * batch_size * seq * world if sampled else horizon * num_episodes
                if masks is not None:   # the timesteps that exist
                    denom = int(dataset.selected_lengths.sum())
                epoch_loss, epoch_pos_err, epoch_ori_err = tot[0] / denom, tot[1] / denom, tot[2] / denom
                if phase == "val" and has_ema and epoch_loss < best_err and save_model and rank == 0:
                    ema_sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}   # taken under the swap
            cur_lr = optimizer.param_groups[0]["lr"] * tot[-1] if phase == "train" and scheduled and optimizer.lr_factor is not None else None
            time_elapsed = time.time() - since
            if writer is not None:
                tag = "train" if phase == "train" else "val"
                writer.add_scalar("Loss/" + tag, epoch_loss, epoch)
                writer.add_scalar("Err_pos/" + tag, epoch_pos_err, epoch)
                writer.add_scalar("Err_ori/" + tag, epoch_ori_err, epoch)
                if clip_sums is not None and clip_steps:   # every rank clips the same reduced gradient: rank 0's figures are everyone's
                    writer.add_scalar("GradNorm/" + tag, tot[3] / clip_steps, epoch)
                    writer.add_scalar("GradClipped/" + tag, tot[4] / clip_steps, epoch)
                if cur_lr is not None:
                    writer.add_scalar("LR/" + tag, cur_lr, epoch)
                for name, r in (tele or {}).items():
                    for key in ("grad_norm", "update_ratio", "zero_frac"):
                        writer.add_scalar("Telemetry/{}/{}".format(key, name), r[key], epoch)
            if tele is not None:
                if telemetry_log is not None:
                    telemetry_log.append(tele)
                bad = [(r["first_nonfinite_step"], name) for name, r in tele.items() if r["first_nonfinite_step"]]
                if bad and logging and rank == 0:
                    step, name = min(bad, key=lambda b: b[0])
                    print("telemetry: non-finite values first seen in {} at optimizer step {} ({} tensors affected so far)".format(name, step, len(bad)))
            if logging and rank == 0:
                print('{} Loss: {:.4f}, PosErr: {:.4f}, OriErr: {:.4f}. Time elapsed = {:.0f}m {:.0f}s'.format(
                    phase, epoch_loss, epoch_pos_err, epoch_ori_err, time_elapsed // 60, time_elapsed % 60)
                    + ("" if cur_lr is None else " lr = {:.3e}".format(cur_lr)))
            if phase == "val" and epoch_loss < best_err:
                best_err = epoch_loss
                best_model = copy.deepcopy(model.state_dict())
                if save_model and rank == 0:
                    if save_path == 'default':
                        save_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "log", "runs", fname)
                    os.makedirs(os.path.dirname(os.path.abspath(save_path)), exist_ok=True)
                    torch.save(model.state_dict(), save_path)
                    if ema_sd is not None:
                        torch.save(ema_sd, save_path + ".ema")
                    if save_optimizer:
                        torch.save(optimizer.state_dict(), save_path + ".optim")
    if logging and rank == 0:
        time_elapsed = time.time() - since
        print('-' * 10)
        print('Training completed in {:.0f}m {:.0f}s'.format(time_elapsed // 60, time_elapsed % 60))
        print('Best val Err: {:.4f}'.format(best_err))
    model.load_state_dict(best_model)
    return model, best_err
