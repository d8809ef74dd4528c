"""GPU tests of the training telemetry: rpe_param_stats + rpe_param_stats_finalize on synthetic arenas one call at a time, FusedAdam /
FusedAdamW(telemetry=K) over a small arena step by step, a graph-replayed train step of the toy model and one fp16 step -- the three
sums within the bounds of tests/_telemetry_oracle.py (fp64 references from the same fp32 operands), every other column bit-equal."""
import ctypes

import numpy as np
import pytest
import torch

import _telemetry_oracle as TO

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from rgb_proprioceptive_pose_estimator_amd import ops
    from rgb_proprioceptive_pose_estimator_amd._lib import PARAM_STATS_PART_COLS, lib, raw

DEV = "cuda"
GUARD = 7.0
HP = (0.9, 0.999, 1e-8)
NAN = float("nan")


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _state(step, skip=0.0):
    return torch.tensor([1.0, 1.0, 0.0, skip, 0.0, float(step), -3.0, 1.0], dtype=torch.float32).to(DEV)


def _chunk():
    """C: the largest numel that takes one row"""
    lo, hi = 1, 1 << 30
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if lib.rpe_param_stats_rows(mid) == 1 else (lo, mid - 1)
    return lo


class Arena:
    """four fp32 arenas of one layout on the host: tensors at 16-byte boundaries, a gap of 4 floats behind every second one, and every
    padding lane, gap and the tail filled with NaN"""

    def __init__(self, numels, seed=0, data=None):
        gen = torch.Generator().manual_seed(seed)
        self.entries, at = [], 0
        for k, n in enumerate(numels):
            self.entries.append((at, n))
            at += (n + 3) // 4 * 4 + (4 if k % 2 else 0)
        self.total = at + 4
        self.p, self.g, self.m, self.v = (torch.full((self.total,), NAN) for _ in range(4))
        for k, (off, n) in enumerate(self.entries):
            src = data[k] if data is not None else (torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 3.0,
                                                    torch.randn(n, generator=gen) * 0.3, torch.rand(n, generator=gen) * 0.09)
            for buf, s in zip(self.bufs(), src):
                buf[off:off + n] = s
        self.table = ops.param_stats_table(self.entries)

    def bufs(self):
        return (self.p, self.g, self.m, self.v)

    def tensor(self, k):
        off, n = self.entries[k]
        return tuple(b[off:off + n].clone() for b in self.bufs())

    def ref(self, step, hp=HP, skip=False, prev=None):
        return TO.table_ref(*(b.numpy() for b in self.bufs()), self.entries, step, *hp, skip=skip, prev=prev)


class Run:
    """device copies of an Arena, partials and out with one guard row behind each; launch() is the two raw launches"""

    def __init__(self, arena):
        self.arena = arena
        self.dev = [b.to(DEV) for b in arena.bufs()]
        self.table = arena.table.to(DEV)
        self.T, self.rows = arena.table.shape[0], ops.param_stats_total_rows(arena.table)
        self.part = torch.full((self.rows + 1, PARAM_STATS_PART_COLS), GUARD, dtype=torch.float64, device=DEV)
        self.out = torch.zeros(self.T + 1, TO.COLS, dtype=torch.float64, device=DEV)
        self.out[self.T:] = GUARD

    def upload(self):
        for d, b in zip(self.dev, self.arena.bufs()):
            d.copy_(b)

    def launch(self, step, every=1, hp=HP, skip=0.0):
        st = _state(step, skip)
        lib.rpe_param_stats(*(_P(d) for d in self.dev), _P(self.table), ctypes.c_void_p(self.arena.table.data_ptr()), self.T, _P(self.part), *hp, _P(st),
                            every, _S())
        lib.rpe_param_stats_finalize(_P(self.part), _P(self.table), self.T, _P(self.out), _P(st), every, _S())
        torch.cuda.synchronize()
        assert (self.part[self.rows:] == GUARD).all(), "rpe_param_stats wrote behind its partial rows"
        assert (self.out[self.T:] == GUARD).all(), "rpe_param_stats_finalize wrote behind out"
        assert st.cpu().tolist() == [1.0, 1.0, 0.0, skip, 0.0, float(step), -3.0, 1.0], "the state block was written"
        for d, b in zip(self.dev, self.arena.bufs()):
            assert torch.equal(_bits(d), _bits(b)), "an input arena was written"
        return self.out[:self.T].cpu().numpy()


# ------------------------------------------------------------------ 1. shapes
def test_shapes_padding_and_guards():
    """tensors of numel 1, 3, 4, 5, 63, 64, 65, C - 1, C, C + 1 and 2 C + 3 in one table (C the chunk: one, one, two and three rows),
    NaN in every padding lane and gap of all four arenas: a single NaN read into a result would show in a sum, a maximum or a count.
    Sums within their bound, everything else bit-equal, the guard rows behind partials and out intact, the inputs unchanged."""
    C = _chunk()
    numels = [1, 3, 4, 5, 63, 64, 65, C - 1, C, C + 1, 2 * C + 3]
    a = Arena(numels, seed=1)
    assert a.table[:, 2].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11]
    run = Run(a)
    for step in (1, 5, 1000):
        got = run.launch(step)
        TO.check_table(got, *a.ref(step), "shapes step=%d" % step)
        assert not got[:, 5].any() and not got[:, 7].any() and not got[:, 9].any(), "a padding NaN was read"


# ------------------------------------------------------------------ 2. values
def test_planted_values():
    """+inf, -inf, NaN, +0, -0, a denormal, 1e20 and 1e-20 in g; inf in p; v = 0 with m = 0; a non-finite m; a negative v: counts exact,
    and the finite sums are those of the oracle on the same data -- one inf does not hide the rest of the tensor.  eps = 0 as well,
    where v = 0 with m = 0 is 0 / 0 and leaves sum d^2."""
    C = _chunk()
    a = Arena([37, C + 9], seed=2)
    for k, (off, n) in enumerate(a.entries):
        at = off + (0 if k == 0 else C - 3)          # the second tensor's plants straddle its two rows
        plants = [float("inf"), float("-inf"), NAN, 0.0, -0.0, 1e-42, 1e20, 1e-20]
        plants = plants if k == 0 else plants[:6]     # (1e20 squared hides every other term of its sum: the second tensor goes without)
        a.g[at:at + len(plants)] = torch.tensor(plants)
        a.p[off + n - 1] = float("inf")
        a.m[off + 10], a.v[off + 10] = 0.0, 0.0
        a.m[off + 11] = float("inf")
        a.m[off + 12] = NAN
        a.v[off + 13] = -1.0
    assert a.g[a.entries[0][0] + 5] != 0.0, "the denormal survived"
    run = Run(a)
    for hp in (HP, (0.8, 0.99, 0.0)):
        run.out[:run.T] = 0.0
        got = run.launch(3, hp=hp)
        ref, bnd = a.ref(3, hp)
        TO.check_table(got, ref, bnd, "values eps=%g" % hp[2])
        assert got[:, 5].tolist() == [3.0, 3.0] and got[:, 6].tolist() == [2.0, 2.0] and got[:, 7].tolist() == [1.0, 1.0]
        assert got[0, 3] == float(np.float32(1e20)) and got[0, 0] >= 1e40 and got[1, 0] < 1e6 and np.isfinite(got).all()
        assert got[:, 9].tolist() == [3.0, 3.0]


# ------------------------------------------------------------------ 3. determinism
def test_two_runs_and_two_placements_give_the_same_bits():
    C = _chunk()
    a = Arena([5, 2 * C + 3, 64, 1, 2 * C + 3], seed=3)
    big = Arena([2 * C + 3], seed=30).tensor(0)
    data = [a.tensor(k) for k in range(5)]
    data[1] = data[4] = big
    a = Arena([5, 2 * C + 3, 64, 1, 2 * C + 3], data=data)
    assert a.entries[1][0] != a.entries[4][0] and a.table[1, 2] != a.table[4, 2]
    r1, r2 = Run(a), Run(a)
    o1, o2 = r1.launch(7), r2.launch(7)
    assert np.array_equal(o1.view(np.int64), o2.view(np.int64)) and torch.equal(_bits(r1.part), _bits(r2.part)), "two runs differ"
    assert np.array_equal(o1[1, :8].view(np.int64), o1[4, :8].view(np.int64)), "the same tensor at two offsets and row positions differs"
    TO.check_table(o1, *a.ref(7), "determinism")


# ------------------------------------------------------------------ 4. gate and stickiness
def test_gate_stamp_and_sticky_step():
    """every = 3, state[5] = 1 .. 7: out is rewritten at 3 and 6 only (stamped), bit-unchanged otherwise, partials likewise; a NaN planted
    at step 3 only stays in column 9 at step 6 and after, until it is zeroed; state[3] = 1 gives sum d^2 = 0 and nothing else changes"""
    C = _chunk()
    a = Arena([9, C + 1], seed=4)
    run = Run(a)
    run.out[:run.T] = -1.0
    run.out[:run.T, 9] = 0.0
    clean_g = a.g.clone()
    prev, prev_part = run.out.clone(), run.part.clone()
    table = None
    for step in range(1, 8):
        a.g.copy_(clean_g)
        if step == 3:
            a.g[a.entries[1][0] + C] = NAN          # the second tensor's second row
        run.upload()
        got = run.launch(step, every=3)
        if step in (3, 6):
            table = a.ref(step, prev=table[0] if table else None)
            TO.check_table(got, *table, "gate step=%d" % step)
            assert got[:, 8].tolist() == [float(step)] * 2 and got[:, 9].tolist() == [0.0, 3.0]
            assert got[1, 5] == (1.0 if step == 3 else 0.0)
        else:
            assert torch.equal(_bits(run.out), _bits(prev)) and torch.equal(_bits(run.part), _bits(prev_part)), "step %d was measured" % step
        prev, prev_part = run.out.clone(), run.part.clone()
    assert run.out[:run.T, 8].tolist() == [6.0, 6.0] and run.out[:run.T, 9].tolist() == [0.0, 3.0]
    run.out[:run.T, 9] = 0.0                        # what optimizer.reset_param_stats() does
    got = run.launch(9, every=3)
    assert got[:, 8].tolist() == [9.0, 9.0] and got[:, 9].tolist() == [0.0, 0.0]
    skipped = run.launch(9, every=3, skip=1.0)
    assert skipped[:, 2].tolist() == [0.0, 0.0] and got[:, 2].all()
    keep = [c for c in range(TO.COLS) if c != 2]
    assert np.array_equal(skipped[:, keep].view(np.int64), got[:, keep].view(np.int64))
    TO.check_table(skipped, *a.ref(9, skip=True), "skipped step")


# ------------------------------------------------------------------ 5. refusals
def test_refusals_launch_nothing():
    a = Arena([5, 70], seed=5)
    run = Run(a)
    run.out[:] = GUARD
    st = _state(3)
    host = lambda t: ctypes.c_void_p(t.data_ptr())
    bufs = [_P(d) for d in run.dev]

    def stats(bufs=bufs, table=_P(run.table), table_host=host(a.table), T=run.T, part=_P(run.part), state=_P(st), every=1):
        return raw.rpe_param_stats(*bufs, table, table_host, T, part, *HP, state, every, _S())

    def fin(part=_P(run.part), table=_P(run.table), T=run.T, out=_P(run.out), state=_P(st), every=1):
        return raw.rpe_param_stats_finalize(part, table, T, out, state, every, _S())

    assert stats(T=0) == 1 and stats(T=-2) == 1 and stats(every=0) == 1 and stats(every=-1) == 1
    for k in range(4):
        assert stats(bufs=[None if i == k else b for i, b in enumerate(bufs)]) == 1
        assert stats(bufs=[ctypes.c_void_p(run.dev[i].data_ptr() + 4) if i == k else b for i, b in enumerate(bufs)]) == 3
    assert stats(table=None) == 1 and stats(table_host=None) == 1 and stats(part=None) == 1 and stats(state=None) == 1
    bad = a.table.clone()
    bad[1, 0] += 2
    assert stats(table_host=host(bad)) == 3 and b"multiple of 4" in raw.rpe_last_error()
    bad = a.table.clone()
    bad[1, 2] += 1
    assert stats(table_host=host(bad)) == 1
    assert fin(T=0) == 1 and fin(every=0) == 1 and fin(part=None) == 1 and fin(table=None) == 1 and fin(out=None) == 1 and fin(state=None) == 1
    torch.cuda.synchronize()
    assert (run.out == GUARD).all() and (run.part == GUARD).all(), "a refused call wrote"
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.param_stats_table([(0, 3), (3, 5)])
    z = torch.zeros(16, device=DEV)
    with pytest.raises(ValueError, match="behind the arena"):
        ops.param_stats(z, z, z, z, run.table, a.table, run.part, run.out[:run.T], *HP, st)
    # the dispatcher entry is the same two launches
    import rgb_proprioceptive_pose_estimator_amd.torch_ops  # noqa: F401
    run.out[:run.T] = 0.0
    torch.ops.rpe.param_stats(*run.dev, run.table, a.table, run.part, run.out[:run.T], *HP, st, 1)
    torch.cuda.synchronize()
    TO.check_table(run.out[:run.T].cpu().numpy(), *a.ref(3), "torch.ops.rpe.param_stats")
    assert (run.out[run.T:] == GUARD).all()


# ------------------------------------------------------------------ 6. optimizer
def _tiny_module(seed=3):
    """parameter sizes 1, 7, 10 and 33; the third frozen (the module of tests/test_gpu_clip.py)"""
    torch.manual_seed(seed)
    mod = torch.nn.Module()
    for name, n in (("a", 1), ("b", 7), ("c", 10), ("d", 33)):
        mod.register_parameter(name, torch.nn.Parameter(torch.randn(n, device=DEV)))
    mod.c.requires_grad_(False)
    return mod


GROUP_HP = (dict(betas=(0.9, 0.999), eps=1e-8, lr=1e-3), dict(betas=(0.8, 0.99), eps=1e-6, lr=3e-3))


def _make(variant, telemetry, capturable=False):
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam, FusedAdamW, LRSchedule
    from rgb_proprioceptive_pose_estimator_amd.params import ParamArena
    mod = _tiny_module()
    arena = ParamArena(mod)
    groups = [dict(params=[mod.a, mod.b], **GROUP_HP[0]), dict(params=[mod.c, mod.d], **GROUP_HP[1])]
    if variant == "alone":
        opt = FusedAdam(groups, capturable=capturable, telemetry=telemetry)
    else:
        opt = FusedAdamW(groups, weight_decay=1e-2, max_grad_norm=1.0, lr_schedule=LRSchedule("cosine", warmup_steps=2, total_steps=10), ema_decay=0.9,
                         telemetry=telemetry)
    return mod, arena, opt


@pytest.mark.parametrize("variant", ["alone", "clip+schedule+ema"])
def test_optimizer_measures_after_the_update_and_changes_nothing(variant):
    """two param groups with their own betas and eps over the tiny arena, three steps with telemetry=1: after every step param_stats
    equals the oracle on the arena's tensors as the step left them (each group's rows with that group's betas and eps), and p, m, v
    (and the average) are bit-identical to the same run with telemetry=None (`alone`: the plain run with the step count on the host,
    whose update launches it keeps).  The buffers are built at the first step and nothing is allocated afterwards."""
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import telemetry_report
    mod, arena, opt = _make(variant, 1)
    others = [_make(variant, None)]
    assert opt.param_stats is None
    entries = [(0, 1), (4, 7), (24, 33)]
    gen = torch.Generator().manual_seed(13)
    ptrs = None
    allocations = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]      # device allocations made so far, a counter
    for k, scale in enumerate((1.0, 30.0, 1e-3), start=1):
        grad = torch.randn(arena.numel, generator=gen) * scale
        for _, a_, o_ in [(mod, arena, opt)] + others:
            a_.grad.copy_(grad)
            before = allocations()
            o_.step()
            assert k == 1 or o_ is not opt or allocations() == before, "step %d allocated on the device" % k
        torch.cuda.synchronize()
        assert opt._dev_state[5].item() == float(k)
        host = [t.cpu().numpy() for t in (arena.flat, arena.grad, opt._m, opt._v)]
        ref0, bnd0 = TO.table_ref(*host, entries[:2], k, *GROUP_HP[0]["betas"], GROUP_HP[0]["eps"])
        ref1, bnd1 = TO.table_ref(*host, entries[2:], k, *GROUP_HP[1]["betas"], GROUP_HP[1]["eps"])
        got = opt.param_stats.cpu().numpy()
        TO.check_table(got, np.concatenate([ref0, ref1]), np.concatenate([bnd0, bnd1]), "optimizer %s step %d" % (variant, k))
        for _, a_, o_ in others:
            pairs = [(arena.flat, a_.flat), (opt._m, o_._m), (opt._v, o_._v)] + ([(opt._ema, o_._ema)] if variant != "alone" else [])
            for mine, theirs in pairs:
                assert torch.equal(_bits(mine), _bits(theirs)), "telemetry changed the update (%s, step %d)" % (variant, k)
            assert o_.param_stats is None
        here = (opt.param_stats.data_ptr(),) + tuple(pl[2].data_ptr() for pl in opt._tele[1])
        assert ptrs in (None, here), "the telemetry buffers were rebuilt"
        ptrs = here
    assert opt.param_stats_names(mod) == ["a", "b", "d"] and opt.param_stats_groups() == [0, 0, 1]
    rep = telemetry_report(opt, mod)
    factor = 1.0 if opt.lr_factor is None else opt.lr_factor.item()
    assert list(rep) == ["a", "b", "d"]
    for name, row, hp in zip(rep, got, (GROUP_HP[0], GROUP_HP[0], GROUP_HP[1])):
        r = rep[name]
        assert r["grad_norm"] == np.sqrt(row[0]) and r["weight_norm"] == np.sqrt(row[1]) and r["grad_max"] == row[3] and r["step"] == 3
        assert r["nonfinite"] == 0 and r["first_nonfinite_step"] == 0 and r["zero_frac"] == 0.0
        want = hp["lr"] * factor * np.sqrt(row[2]) / np.sqrt(row[1])
        assert abs(r["update_ratio"] - want) <= 1e-12 * want and 0.0 < want < float("inf")
    arena.grad[24:28] = 0.0
    arena.grad[5] = float("inf")
    opt.step()
    rep = telemetry_report(opt, mod)
    # (the inf gradient went through the update before the measurement: that weight is NaN now, and counted too)
    assert rep["d"]["zero_frac"] == 4 / 33 and rep["b"]["nonfinite"] == 2 and rep["b"]["first_nonfinite_step"] == 4 and rep["a"]["nonfinite"] == 0
    opt.reset_param_stats()
    assert not opt.param_stats[:, 9].any()


# ------------------------------------------------------------------ 7. captured step, 8. f16
def _toy(dtype):
    from rgb_proprioceptive_pose_estimator_amd import models as M
    torch.manual_seed(4)
    return M.NaiveObjectStateEstimator("cube", [32], 50, 32, False, (9,), False, False, False, compute_dtype=dtype).cuda().train()


def _toy_batches():
    from rgb_proprioceptive_pose_estimator_amd import models as M
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import synthetic_batch
    batches = []
    for i in range(2):
        b = synthetic_batch((4,), 20 + i)
        batches.append((b["img"], None, b["x0bar"], b["x0"], None, b["obj"]))
    criterion = {"obj_loss": M.PoseDistanceLoss("combined", 1.0, 0.5, 1e-4, "pose"), "val_loss": M.PoseDistanceLoss(mode="val")}
    return batches, criterion


def _entries(opt, arena):
    return [(off, p.numel()) for g in opt.param_groups for p, off in opt._telemetry_tensors(arena, g)]


def test_captured_step_replays_the_gate():
    """GraphedTrainStep takes no new argument: the optimizer step, telemetry included, is inside the capture.  telemetry=2, the device's
    step count set back to 0 after the build, four replays: the table is bit-unchanged after replays 1 and 3 and stamped 2, then 4,
    after replays 2 and 4.  `Equal to the same steps run eagerly, bit for bit` is asserted where it is well posed: the toy model's aux
    head accumulates its gradients with atomics and the network is chaotic (tests/test_gpu_train.py), so two runs of the MODEL differ
    whatever the optimizer does; after every measured replay the same two launches issued eagerly over the replay's own arenas and
    state block must reproduce the replayed table bit for bit, and both must equal the oracle on those arenas."""
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import GraphedTrainStep
    batches, criterion = _toy_batches()
    m = _toy(torch.float32)
    opt = FusedAdam(m.parameters(), lr=1e-3, capturable=True, telemetry=2)
    g = GraphedTrainStep(m, criterion, opt, True, batches[0], warmup=2)
    torch.cuda.synchronize()
    arena = m._arena
    entries = _entries(opt, arena)
    assert opt.param_stats[:, 8].tolist() == [2.0] * len(entries), "the warm-up's second step was measured"
    opt._dev_state[5] = 0.0
    opt.param_stats.zero_()
    table, table_host, partials, _ = opt._tele[1][0]
    stamps = []
    for k in range(1, 5):
        before = opt.param_stats.clone()
        g(batches[k % 2])
        torch.cuda.synchronize()
        assert opt._dev_state[5].item() == float(k)
        stamps.append(opt.param_stats[0, 8].item())
        if k % 2:
            assert torch.equal(_bits(opt.param_stats), _bits(before)), "replay %d was measured" % k
            continue
        assert (opt.param_stats[:, 8] == float(k)).all()
        eager = torch.zeros_like(opt.param_stats)
        ops.param_stats(arena.flat, arena.grad, opt._m, opt._v, table, table_host, torch.zeros_like(partials), eager, *HP, opt._dev_state, 2)
        torch.cuda.synchronize()
        assert torch.equal(_bits(eager), _bits(opt.param_stats)), "replayed and eager tables differ at step %d" % k
        if k == 4:      # (one oracle pass: the model is a ResNet-50)
            host = [t.cpu().numpy() for t in (arena.flat, arena.grad, opt._m, opt._v)]
            TO.check_table(opt.param_stats.cpu().numpy(), *TO.table_ref(*host, entries, k, *HP), "captured step %d" % k)
    assert stamps == [0.0, 2.0, 2.0, 4.0]
    assert opt.param_stats[:, 0].sum().item() > 0.0 and opt.param_stats_names(m)[0] == next(n for n, p in m.named_parameters() if p.requires_grad)


def test_f16_step_measures_the_unscaled_gradient():
    """one eager step of the fp16 toy model: the loss scaler's unscale pass runs inside FusedAdam.step, and the measured gradient norms
    are those of the UNSCALED gradient that the step leaves in arena.grad -- the pass sits after the unscale.  A step the scaler skips
    (an overflow at its initial scale) reports its non-finite gradients and sum d^2 = 0."""
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import train_step
    batches, criterion = _toy_batches()
    m = _toy(torch.float16)
    opt = FusedAdam(m.parameters(), lr=1e-3, telemetry=1)
    m._materialize(torch.device("cuda", torch.cuda.current_device()))
    arena = m._arena
    opt._ensure()
    for _ in range(4):
        train_step(m, batches[1], criterion, opt, True, "train", None)
        st = arena.loss_scaler.state
        stats = opt.param_stats.cpu().numpy()
        if st[3].item() == 0.0:
            break
        assert stats[:, 5].sum() > 0 and not stats[:, 2].any() and (stats[:, 8] == 0.0).all(), "a skipped step: non-finite gradients, no update"
        opt.reset_param_stats()
    assert st[3].item() == 0.0 and st[5].item() == 1.0 and st[0].item() > 1.0, "no fp16 step was taken: %s" % (st.tolist(),)
    entries = _entries(opt, arena)
    host = [t.cpu().numpy() for t in (arena.flat, arena.grad, opt._m, opt._v)]
    ref, bnd = TO.table_ref(*host, entries, 1, *HP)
    TO.check_table(stats, ref, bnd, "f16 step")
    scaled = sum(float((arena.grad[o:o + n].double() * st[0].item()).pow(2).sum()) for o, n in entries)
    assert stats[:, 0].sum() < 0.5 * scaled, "the norms are those of the scaled gradient"
    assert stats[:, 0].sum() > 0.0 and not stats[:, 5].any()
