"""Adam over the flat parameter arena: one HIP kernel per trainable segment instead of ~170 per-tensor
update chains.  Same hyper-parameter defaults and update rule as torch.optim.Adam, which the reference
constructs at scripts/train_model.py:228 (no weight decay, no amsgrad); parameters whose gradient is
identically zero (e.g. the unused depth head) do not move, matching torch's `grad is None` skip.

Two options the reference does not have, both off by default and both on the device (no host synchronisation, capturable by
util.learn_utils.GraphedTrainStep): `max_grad_norm` clips the global gradient norm as torch.nn.utils.clip_grad_norm_ does, and
`weight_decay` (FusedAdamW) is torch.optim.AdamW's decoupled decay.  The loss is SUMMED over episodes x sequence steps
(DESIGN.md section 2), so the gradient grows with the batch; the clip bounds the update whatever the batch.

Three more, off by default and on the device as well: `lr_schedule` (LRSchedule: linear warm-up, then constant / cosine / step decay,
evaluated by rpe_lr_schedule from the device's step count), per-group hyper-parameters (every param group is updated with its own lr,
betas, eps and weight_decay over its own arena segments) and `ema_decay` (an exponential moving average of the weights, written by the
update kernel itself).  lr_factor() below is the one statement of the schedule rule.

One instrument, off by default and on the device too: `telemetry=K` measures, every K-th optimizer step and after the update, per-tensor
gradient / weight / update norms, maxima, non-finite and zero counts of every param group (rpe_param_stats: two launches per group).
"""
import contextlib
import math

import torch

from . import ops
from ._lib import PARAM_STATS_COLS, PARAM_STATS_PART_COLS, lib
from .params import arena_of


def _check_options(weight_decay, max_grad_norm):
    if not 0.0 <= weight_decay < math.inf:      # negative, NaN or inf
        raise ValueError("invalid weight_decay %r: a finite value >= 0" % (weight_decay,))
    if max_grad_norm is not None and not max_grad_norm > 0.0:      # <= 0 or NaN
        raise ValueError("invalid max_grad_norm %r: None (off) or a value > 0" % (max_grad_norm,))


SCHEDULE_KINDS = ("constant", "cosine", "step")     # the `kind` argument of rpe_lr_schedule is the index


def _is_int(x):
    return isinstance(x, int) and not isinstance(x, bool)


class LRSchedule:
    """Linear warm-up over `warmup_steps` optimizer steps from `warmup_start_factor`, then `kind`:
    constant: 1;  cosine: half a cosine from 1 down to `min_factor` at `total_steps`, held there afterwards;  step: times `gamma` every
    `step_size` steps after the warm-up.  A validated value object: the position is the optimizer's step count, not kept here."""
    FIELDS = ("kind", "warmup_steps", "warmup_start_factor", "total_steps", "min_factor", "step_size", "gamma")

    def __init__(self, kind="constant", warmup_steps=0, warmup_start_factor=0.1, total_steps=None, min_factor=0.0, step_size=None, gamma=0.1):
        if kind not in SCHEDULE_KINDS:
            raise ValueError("invalid schedule kind %r: one of %s" % (kind, ", ".join(SCHEDULE_KINDS)))
        if not _is_int(warmup_steps) or warmup_steps < 0:
            raise ValueError("invalid warmup_steps %r: an integer >= 0" % (warmup_steps,))
        if not 0.0 <= warmup_start_factor <= 1.0:
            raise ValueError("invalid warmup_start_factor %r: a value in [0, 1]" % (warmup_start_factor,))
        if not 0.0 <= min_factor <= 1.0:
            raise ValueError("invalid min_factor %r: a value in [0, 1]" % (min_factor,))
        if total_steps is not None and not _is_int(total_steps):
            raise ValueError("invalid total_steps %r: an integer" % (total_steps,))
        if kind == "cosine" and (total_steps is None or total_steps <= warmup_steps):
            raise ValueError("invalid total_steps %r: the cosine schedule needs total_steps > warmup_steps" % (total_steps,))
        if (step_size is not None or kind == "step") and (not _is_int(step_size) or step_size < 1):
            raise ValueError("invalid step_size %r: an integer >= 1" % (step_size,))
        if not 0.0 < gamma <= 1.0:
            raise ValueError("invalid gamma %r: a value in (0, 1]" % (gamma,))
        self.kind, self.warmup_steps, self.warmup_start_factor = kind, warmup_steps, float(warmup_start_factor)
        self.total_steps, self.min_factor, self.step_size, self.gamma = total_steps, float(min_factor), step_size, float(gamma)

    def state_dict(self):
        return {k: getattr(self, k) for k in self.FIELDS}

    def load_state_dict(self, sd):
        self.__init__(**{k: sd[k] for k in self.FIELDS})

    def __eq__(self, other):
        return isinstance(other, LRSchedule) and self.state_dict() == other.state_dict()

    def __repr__(self):
        return "LRSchedule(%s)" % ", ".join("%s=%r" % kv for kv in self.state_dict().items())

    def c_args(self):
        """the scalar arguments of rpe_lr_schedule (an unused total_steps / step_size as 0 / 1)"""
        return (SCHEDULE_KINDS.index(self.kind), self.warmup_steps, self.warmup_start_factor, self.total_steps or 0, self.min_factor,
                self.step_size or 1, self.gamma)


def lr_factor(schedule, e):
    """The factor that multiplies every group's lr at the optimizer step that follows `e` completed ones (e = 0: the first step), in
    fp64 -- the closed form rpe_lr_schedule evaluates on the device.  With W = warmup_steps, s = warmup_start_factor, T = total_steps,
    fmin = min_factor:
        e < W:     s + (1 - s) e / W                      torch's LinearLR(start_factor=s, total_iters=W)
        constant:  1
        cosine:    fmin + (1 - fmin)(1 + cos(pi (min(e, T) - W) / (T - W))) / 2
                                                          CosineAnnealingLR(T_max=T - W, eta_min=fmin lr) after the warm-up; beyond T
                                                          it HOLDS fmin (torch's recursion climbs again)
        step:      gamma ** ((e - W) // step_size)        StepLR after the warm-up"""
    e = int(e)
    if e < 0:
        raise ValueError("lr_factor: e >= 0")
    W, s = schedule.warmup_steps, schedule.warmup_start_factor
    if e < W:
        return s + (1.0 - s) * e / W
    if schedule.kind == "cosine":
        T, fmin = schedule.total_steps, schedule.min_factor
        return fmin + (1.0 - fmin) * (1.0 + math.cos(math.pi * (min(e, T) - W) / (T - W))) / 2.0
    if schedule.kind == "step":
        return schedule.gamma ** ((e - W) // schedule.step_size)
    return 1.0


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, capturable=False, *, weight_decay=0.0, max_grad_norm=None,
                 lr_schedule=None, ema_decay=None, telemetry=None):
        """capturable: keep the step count (for the bias corrections) on the DEVICE, so that a captured hipGraph of the whole
        train step (util.learn_utils.GraphedTrainStep) advances it at every replay; a host-side count would be frozen at its
        capture-time value.  Same update rule either way.

        max_grad_norm: clip the global l2 norm of all trainable gradients to this value before the update: every gradient is
        multiplied by min(1, max_grad_norm / (norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s rule, with the norm summed in fp64
        on the device.  UNLIKE torch's in-place clip, `.grad` / `arena.grad` are not written: they keep the true (unscaled,
        unclipped) gradient, and the coefficient is applied inside the update kernel.  `grad_norm` and `clip_coef` expose the
        last step's values as 0-d device tensors.  inf: measure the norm only.
        weight_decay: decoupled decay, p *= 1 - lr weight_decay before the update (torch.optim.AdamW; see FusedAdamW).  It
        applies to every trainable parameter, BatchNorm weights and biases included, as AdamW(model.parameters()) does.
        With either option set the step count lives on the device whatever `capturable` says.

        lr_schedule: an LRSchedule.  Every group's rate is group["lr"] * lr_factor(lr_schedule, e), e the optimizer steps taken so
        far, evaluated on the device from the device's step count (a skipped fp16 step does not advance it).  Under
        GraphedTrainStep a host scheduler (torch.optim.lr_scheduler) that writes group["lr"] is NOT seen by the replays -- the rate
        is a launch argument the capture froze -- while lr_schedule= is.  In eager mode both compose: the factor multiplies whatever
        group["lr"] holds.  `lr_factor` and `steps_scheduled` expose the last step's factor and e as 0-d device tensors.
        ema_decay: in [0, 1): keep ema = decay ema + (1 - decay) p over all trainable parameters, updated from the new p inside the
        update kernel (torch.optim.swa_utils.get_ema_multi_avg_fn's rule).  It starts as a copy of the arena, so frozen parameters
        equal themselves; BatchNorm buffers are not averaged (AveragedModel's default does not either).  ema_parameters() is the
        flat average, averaged_weights(model) swaps it into the model for validation / rollout.
        Neither is a param-group key: they are attributes, and top-level keys ("lr_schedule", "ema") of state_dict().  With either set
        the step count lives on the device as well.
        Param groups: every group is updated with its own lr, betas, eps and weight_decay over its own parameters' segments;
        max_grad_norm is one global norm and must be the same in all groups.

        telemetry: None (off) or a positive int K: after the update kernels of every param group, two more launches (rpe_param_stats,
        rpe_param_stats_finalize) reduce that group's trainable tensors of p, g, m, v to one fp64 row each -- sum g^2, sum p^2, sum d^2
        (d the Adam direction of the update just applied, with the group's betas and eps), max|g|, max|p|, non-finite g, zero g,
        non-finite p, the step measured, the first step with a non-finite value (ops.PARAM_STATS_COLUMNS).  The device decides from its
        own step count whether a step is measured (count % K == 0), so the launches are the same at every step and a captured train
        step replays them; nothing is read by the host and nothing is allocated after the first step.  It sits after the update because
        on the fp16 path the arena gradient carries the loss scale until this step's unscale pass, and because d needs the new moments.
        A skipped fp16 step does not advance the count: it is measured again if the count is still a multiple of K, shows its non-finite
        gradients, and reports sum d^2 = 0.  `param_stats` is the (T, COLS) device tensor (None before the first step), rows in the
        order of param_stats_names(); reset_param_stats() clears the sticky column.  Not a state_dict key.  Like the other options it
        keeps a step count on the device: the one the other options or `capturable` already keep, and without any of them a count of
        its own, bumped by one extra launch behind update launches that stay exactly those of telemetry=None (the host-count and the
        device-count update kernels round differently in the last bit; telemetry must not choose between them)."""
        if telemetry is not None and not (_is_int(telemetry) and telemetry >= 1):
            raise ValueError("invalid telemetry %r: None (off) or an integer >= 1 (measure every K-th step)" % (telemetry,))
        self.telemetry = telemetry
        self._tele = None           # (arena, per-group plans, out, the param group of every row): built at the first measured step
        if lr < 0.0 or eps < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameters")
        _check_options(weight_decay, max_grad_norm)
        if lr_schedule is not None and not isinstance(lr_schedule, LRSchedule):
            raise ValueError("invalid lr_schedule %r: None (off) or an LRSchedule" % (lr_schedule,))
        if ema_decay is not None and not 0.0 <= ema_decay < 1.0:      # < 0, >= 1 or NaN
            raise ValueError("invalid ema_decay %r: None (off) or a value in [0, 1)" % (ema_decay,))
        self.lr_schedule, self.ema_decay = lr_schedule, ema_decay
        self._ema = None            # the fp32 average in arena order (allocated with the moments)
        self._sched = None          # 4 device floats: factor, steps taken before the last step, -, -
        self._sched_state = None    # the block the last scheduled step wrote factor and step count to
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm))
        self.capturable = capturable
        self._dev_state = None
        self._clip_state = None     # the state block the last clipped step wrote its norm and coefficient to
        self._partials = None       # (segments, per-segment row offsets, fp64 partial rows of rpe_grad_sumsq)
        self._step = 0
        self._m = self._v = None
        self._arena = None

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        g = self.param_groups[-1]
        try:
            if g["lr"] < 0.0 or g["eps"] < 0.0 or not (0.0 <= g["betas"][0] < 1.0 and 0.0 <= g["betas"][1] < 1.0):
                raise ValueError("invalid Adam hyper-parameters in a param group")
            _check_options(g["weight_decay"], g["max_grad_norm"])
            norms = {x["max_grad_norm"] for x in self.param_groups}
            if len(norms) > 1:
                raise ValueError("max_grad_norm is ONE global norm: every param group must carry the same value, got %s" % sorted(map(repr, norms)))
        except ValueError:
            del self.param_groups[-1]
            raise

    def _ensure(self):
        params = [p for g in self.param_groups for p in g["params"]]
        arena = arena_of(params)
        if arena is None:
            raise RuntimeError("FusedAdam needs the model's flat parameter arena: run one forward on the device "
                               "(or call model._materialize) before the first step")
        if arena is not self._arena:
            self._arena = arena
            if self._dev_state is not None:
                self._dev_state = self._dev_state.to(arena.flat.device)
            amp_sd = getattr(self, "_amp_restore", None)
            if amp_sd is not None and getattr(arena, "loss_scaler", None) is not None:
                arena.loss_scaler.load_state_dict(amp_sd)
                self._amp_restore = None
            loaded = self._m is not None and self._m.numel() == arena.flat.numel()   # moments restored by load_state_dict
            self._m = self._m.to(arena.flat.device) if loaded else torch.zeros_like(arena.flat)
            self._v = self._v.to(arena.flat.device) if loaded else torch.zeros_like(arena.flat)
            if self.ema_decay is not None:
                loaded = self._ema is not None and self._ema.numel() == arena.flat.numel()   # average restored by load_state_dict
                self._ema = self._ema.to(arena.flat.device) if loaded else arena.flat.clone()  # a copy: frozen parameters equal themselves
            self._sched = self._sched_state = None
        return arena

    def zero_grad(self, set_to_none=True):
        """The HIP backward overwrites every gradient view, so there is nothing to clear on the device; this only tells the arena
        that the next backward starts fresh instead of accumulating (reference loop: util/learn_utils.py:152)."""
        arena = self._arena
        if arena is None:
            params = [p for g in self.param_groups for p in g["params"]]
            arena = arena_of(params)
        if arena is not None:
            arena.zero_grad()
        return None

    @property
    def max_grad_norm(self):
        return self.param_groups[0].get("max_grad_norm")

    @property
    def grad_norm(self):
        """0-d device view of the last clipped step's global gradient norm (None before the first one); reading it synchronises"""
        return None if self._clip_state is None else self._clip_state[6]

    @property
    def clip_coef(self):
        """0-d device view of the coefficient the last clipped step multiplied the gradients by (None before the first one)"""
        return None if self._clip_state is None else self._clip_state[7]

    @property
    def lr_factor(self):
        """0-d device view of the factor the last scheduled step multiplied every group's lr by (None before the first one)"""
        return None if self._sched_state is None else self._sched_state[0]

    @property
    def steps_scheduled(self):
        """0-d device view of e, the optimizer steps taken before the last scheduled step (None before the first one)"""
        return None if self._sched_state is None else self._sched_state[1]

    def ema_parameters(self):
        """The flat fp32 average in arena order (None without ema_decay, or before the arena exists)"""
        return self._ema

    def _swap_ema(self, arena):
        s = ops._stream()
        for lo, hi in arena.trainable_segments():
            lib.rpe_swap_f32(ops._p(arena.flat[lo:hi]), ops._p(self._ema[lo:hi]), hi - lo, s)

    @contextlib.contextmanager
    def averaged_weights(self, model=None):
        """Inside the block the trainable parameters hold the average (and ema_parameters() the raw weights): an in-place exchange
        over the trainable segments, undone by the same call on exit, exceptions included.  No address changes, so a captured train
        step replays correctly afterwards; use it OUTSIDE any capture.  `model`: its trunk is told that the weights changed (the
        cached compute-dtype / BN-folded copies are stale), on entry and on exit."""
        if self.ema_decay is None:
            raise RuntimeError("averaged_weights() needs FusedAdam(..., ema_decay=...)")
        arena = self._ensure()
        trunk = getattr(model, "trunk", None)
        self._swap_ema(arena)
        if trunk is not None:
            trunk.weights_changed()
        try:
            yield self
        finally:
            self._swap_ema(arena)
            if trunk is not None:
                trunk.weights_changed()

    def _groups(self, arena):
        """[(param group, its trainable segments)]; with one group the segments are the arena's, as they always were"""
        if len(self.param_groups) == 1:
            return [(self.param_groups[0], arena.trainable_segments())]
        return [(g, arena.trainable_segments(g["params"])) for g in self.param_groups]

    def _step_device(self, arena, groups, scaler, max_norm):
        """The device-state route with the norm pass, the decay, the schedule and / or the average: [unscale,] step bump, [sum of
        squares per segment, norm and coefficient,] [schedule,] update per segment.  No host synchronisation; nothing is allocated
        after the first step."""
        scheduled = self.lr_schedule is not None or self.ema_decay is not None
        s = ops._stream()
        if scaler is not None:
            st = scaler.unscale_and_update(arena.grad)                           # fp16: rpe_amp_unscale, rpe_amp_update
        else:
            st = self._device_state(arena)
            lib.rpe_amp_update(ops._p(st), 1.0, 1.0, 1 << 30, s)                 # steps += 1 (found_inf is never set)
        segs = [seg for _, gs in groups for seg in gs]
        rows = 0
        if max_norm is not None:
            if self._partials is None or self._partials[0] != segs or self._partials[2].device != arena.grad.device:
                offs = [0]
                for lo, hi in segs:
                    offs.append(offs[-1] + lib.rpe_grad_sumsq_rows(hi - lo))
                self._partials = (segs, offs, torch.empty(max(1, offs[-1]), dtype=torch.float64, device=arena.grad.device))
            _, offs, part = self._partials
            for (lo, hi), off in zip(segs, offs):
                lib.rpe_grad_sumsq(ops._p(arena.grad[lo:hi]), hi - lo, ops._p(part[off:]), s)
            rows = offs[-1]
        if max_norm is not None or not scheduled:
            lib.rpe_clip_coef(ops._p(self._partials[2] if rows else None), rows, 0.0 if max_norm is None else max_norm, ops._p(st), s)   # st[6], st[7]
        use_clip = int(max_norm is not None and math.isfinite(max_norm))
        if scheduled:
            if self._sched is None or self._sched.device != arena.flat.device:
                self._sched = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float32).to(arena.flat.device)   # factor 1 without a schedule
            if self.lr_schedule is not None:
                lib.rpe_lr_schedule(ops._p(st), *self.lr_schedule.c_args(), ops._p(self._sched), s)            # sched[0], sched[1]
                self._sched_state = self._sched
        ema, ema_decay = self._ema, 0.0 if self.ema_decay is None else self.ema_decay
        for g, gs in groups:
            (b1, b2), wd = g["betas"], g.get("weight_decay", 0.0)
            for lo, hi in gs:
                if scheduled:
                    lib.rpe_adamw_step_sched(ops._p(arena.flat[lo:hi]), ops._p(arena.grad[lo:hi]), ops._p(self._m[lo:hi]), ops._p(self._v[lo:hi]),
                                             ops._p(None if ema is None else ema[lo:hi]), hi - lo, g["lr"], b1, b2, g["eps"], wd, ema_decay,
                                             ops._p(st), ops._p(self._sched), use_clip, s)
                else:
                    lib.rpe_adamw_step_clip(ops._p(arena.flat[lo:hi]), ops._p(arena.grad[lo:hi]), ops._p(self._m[lo:hi]), ops._p(self._v[lo:hi]), hi - lo,
                                            g["lr"], b1, b2, g["eps"], wd, ops._p(st), use_clip, s)
        if max_norm is not None:
            self._clip_state = st
        self._measure(arena, groups, st)
        return None

    def _measure(self, arena, groups, st):
        """telemetry: after the update kernels, two launches per param group over that group's tensors, with its betas and eps"""
        if self.telemetry is None:
            return
        for (g, _), plan in zip(groups, self._telemetry_plans(arena, groups)):
            if plan is not None:
                table, table_host, partials, out = plan
                ops.param_stats(arena.flat, arena.grad, self._m, self._v, table, table_host, partials, out, g["betas"][0], g["betas"][1], g["eps"],
                                st, self.telemetry)

    def _telemetry_tensors(self, arena, group):
        """the (parameter, arena offset) pairs a group's telemetry rows stand for: its trainable parameters in arena order"""
        only = {id(p) for p in group["params"]}
        return [(p, off) for p, off in zip(arena.params, arena.offsets) if p.requires_grad and id(p) in only]

    def _telemetry_plans(self, arena, groups):
        """per param group (table on the device, its host copy, partial rows, rows of `param_stats`), or None for a group without
        trainable parameters; built once per arena"""
        if self._tele is None or self._tele[0] is not arena:
            dev = arena.flat.device
            hosts = [[(off, p.numel()) for p, off in self._telemetry_tensors(arena, g)] for g, _ in groups]
            hosts = [ops.param_stats_table(h) if h else None for h in hosts]
            out = torch.zeros(sum(h.shape[0] for h in hosts if h is not None), PARAM_STATS_COLS, dtype=torch.float64, device=dev)
            plans, row_group, t0 = [], [], 0
            for k, h in enumerate(hosts):
                if h is None:
                    plans.append(None)
                    continue
                partials = torch.zeros(ops.param_stats_total_rows(h), PARAM_STATS_PART_COLS, dtype=torch.float64, device=dev)
                plans.append((h.to(dev), h, partials, out[t0:t0 + h.shape[0]]))
                row_group += [k] * h.shape[0]
                t0 += h.shape[0]
            self._tele = (arena, plans, out, row_group)
        return self._tele[1]

    @property
    def param_stats(self):
        """(T, PARAM_STATS_COLS) fp64 device tensor of the last measured step, columns ops.PARAM_STATS_COLUMNS, one row per trainable
        tensor: param group by param group, arena order within a group (arena order overall when the groups do not interleave).  None
        before the first step; reading it synchronises."""
        return None if self._tele is None else self._tele[2]

    def param_stats_names(self, model):
        """the parameter names of `model` in the order of the rows of `param_stats`"""
        params = [p for g in self.param_groups for p in g["params"]]
        arena = self._arena if self._arena is not None else arena_of(params)
        if arena is None:
            raise RuntimeError("param_stats_names needs the model's flat parameter arena (run one forward on the device first)")
        name_of = {id(p): n for n, p in model.named_parameters()}
        return [name_of[id(p)] for g in self.param_groups for p, _ in self._telemetry_tensors(arena, g)]

    def param_stats_groups(self):
        """the index of the param group of every row of `param_stats` (None before the first step)"""
        return None if self._tele is None else list(self._tele[3])

    def reset_param_stats(self):
        """zero the sticky column (the first step with a non-finite value) of every row"""
        if self._tele is not None:
            self._tele[2][:, 9].zero_()

    def _device_state(self, arena):
        # device-side step count: the same state block the loss scaler uses (amp.py), with scale 1 and no unscale pass
        if self._dev_state is None or self._dev_state.device != arena.flat.device:
            st = torch.zeros(8, dtype=torch.float32)
            st[0] = st[1] = 1.0
            st[5] = float(self._step - 1)
            self._dev_state = st.to(arena.flat.device)
        return self._dev_state

    @torch.no_grad()
    def step(self, closure=None):
        arena = self._ensure()
        self._step += 1
        groups = self._groups(arena)
        scaler = getattr(arena, "loss_scaler", None)
        max_norm = self.param_groups[0].get("max_grad_norm")
        if max_norm is not None or self.lr_schedule is not None or self.ema_decay is not None or any(g.get("weight_decay", 0.0) for g, _ in groups):
            return self._step_device(arena, groups, scaler, max_norm)
        if scaler is not None:
            # fp16 compute (amp.py): unscale + finite check, scale update and the skip decision all stay on the device; the
            # bias-correction step count is the device's count of steps actually taken (self._step counts calls)
            st = scaler.unscale_and_update(arena.grad)
            s = ops._stream()
            for g, segs in groups:
                b1, b2 = g["betas"]
                for lo, hi in segs:
                    lib.rpe_adam_step_amp(ops._p(arena.flat[lo:hi]), ops._p(arena.grad[lo:hi]), ops._p(self._m[lo:hi]), ops._p(self._v[lo:hi]), hi - lo,
                                          g["lr"], b1, b2, g["eps"], ops._p(st), s)
            self._measure(arena, groups, st)
            return None
        if self.capturable:
            st = self._device_state(arena)
            s = ops._stream()
            lib.rpe_amp_update(ops._p(st), 1.0, 1.0, 1 << 30, s)   # steps += 1 (found_inf is never set)
            for g, segs in groups:
                b1, b2 = g["betas"]
                for lo, hi in segs:
                    lib.rpe_adam_step_amp(ops._p(arena.flat[lo:hi]), ops._p(arena.grad[lo:hi]), ops._p(self._m[lo:hi]), ops._p(self._v[lo:hi]), hi - lo,
                                          g["lr"], b1, b2, g["eps"], ops._p(st), s)
            self._measure(arena, groups, st)
            return None
        for g, segs in groups:
            b1, b2 = g["betas"]
            for lo, hi in segs:
                ops.adam_step(arena.flat[lo:hi], arena.grad[lo:hi], self._m[lo:hi], self._v[lo:hi], g["lr"], b1, b2, g["eps"], self._step)
        if self.telemetry is not None:
            # telemetry alone: the update launches above are today's, bit for bit; the gate and d's bias corrections read a device-side
            # count, bumped by one launch here (it starts at the host's count, and equals it from then on: no step is ever skipped)
            st = self._device_state(arena)
            lib.rpe_amp_update(ops._p(st), 1.0, 1.0, 1 << 30, ops._stream())
            self._measure(arena, groups, st)
        return None

    def state_dict(self):
        """Flat first / second moments in arena order (= model.parameters() order, 16-byte padded segments) + the step count.
        The reference saves no optimizer state (util/learn_utils.py:211-241); this is what a resumable checkpoint adds."""
        sd = {"step": self._step, "m": self._m, "v": self._v, "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]}
        # device-side step count (capturable / fp16 steps) and the loss scaler's state, so that a resumed run continues both
        if self._dev_state is not None:
            sd["dev_state"] = self._dev_state.detach().cpu().clone()
        scaler = getattr(self._arena, "loss_scaler", None) if self._arena is not None else None
        if scaler is not None:
            sd["amp"] = scaler.state_dict()
        # the schedule's position is the device-side step count above; the average is saved like the moments
        if self.lr_schedule is not None:
            sd["lr_schedule"] = self.lr_schedule.state_dict()
        if self.ema_decay is not None:
            sd["ema"] = self._ema
        return sd

    def load_state_dict(self, sd):
        self._step = int(sd["step"])
        self._m = None if sd["m"] is None else sd["m"].clone()
        self._v = None if sd["v"] is None else sd["v"].clone()
        # a checkpoint without these keys keeps the constructor's schedule, and the average starts from the weights
        if sd.get("lr_schedule") is not None:
            self.lr_schedule = LRSchedule(**sd["lr_schedule"])
        self._ema = sd["ema"].clone() if self.ema_decay is not None and sd.get("ema") is not None else None
        self._arena = None   # re-attached (and the moments moved to its device) at the next step
        self._dev_state = sd["dev_state"].clone() if sd.get("dev_state") is not None else None
        # fp16: the loss scaler must hold the checkpointed scale BEFORE the first backward after the resume multiplies the output
        # gradients by it (round 2 handed it over inside the first step(), i.e. after that backward had used a fresh 2^12: the first
        # step's gradients were off by the ratio of the two scales and went into Adam's moments).  The scaler object belongs to the
        # model: load it now if the arena exists, else leave it on the parameters for the model's _materialize to install.
        amp_sd = sd.get("amp")
        self._amp_restore = None
        if amp_sd is not None:
            params = [p for g in self.param_groups for p in g["params"]]
            arena = arena_of(params)
            scaler = getattr(arena, "loss_scaler", None) if arena is not None else None
            if scaler is not None:
                scaler.load_state_dict(amp_sd)
            else:
                self._amp_restore = amp_sd
                for p in params:
                    p._rpe_pending_amp = amp_sd
        for g, sg in zip(self.param_groups, sd.get("param_groups", [])):
            g.update({k: v for k, v in sg.items() if k != "params"})


class FusedAdamW(FusedAdam):
    """FusedAdam with torch.optim.AdamW's default decoupled weight decay of 1e-2 (what fine-tuning a pretrained trunk expects)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, capturable=False, *, weight_decay=1e-2, max_grad_norm=None,
                 lr_schedule=None, ema_decay=None, telemetry=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, capturable=capturable, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                         lr_schedule=lr_schedule, ema_decay=ema_decay, telemetry=telemetry)
