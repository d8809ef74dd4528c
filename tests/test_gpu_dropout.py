"""Head dropout on the device: the two entry points bit for bit against tests/_dropout_oracle.py, the five model classes against the
same models with `_drop` replaced by a torch formulation of the oracle's mask, the states in which nothing may be dropped, and a
captured train step that draws a fresh mask at every replay.

The comparison rule of the model tests.  The substituted model runs the same kernels on the same numbers everywhere except at the
dropout sites, where torch.where(keep, x * scale, 0) produces the same bits as the kernel; so outputs, loss and gradients can only
differ by what two runs of ONE model differ by.  `_baseline` measures that on the dropout-off model, per tensor, over 16 steps on the
same input.  Measured on an MI355X: every output, the loss and every parameter gradient of `no`, `n`, `td` and `tdo_v2` is
bit-reproducible (172 to 179 tensors each); so is `tdo` (175 tensors) except the two gradients of its depth head's InstanceNorm
affine, depth_nets.0.module.2.weight and .bias, which the parent sums over workgroups with float atomics (depth_head_bwd): three bit
patterns up to 8 units in the last place apart for the weight (1.2e-7 at a value of -0.17) and two patterns 1 unit apart for the bias
(6e-8 at 0.84).  With dropout on, 16 runs of the kernel's model and of the torch-substituted one at ONE step number each show the
same two neighbouring patterns for those two tensors (3e-8 apart at 0.41 and at -0.33).
Every tensor the parent reproduces is compared bit for bit.  For the two it does not, the parent's absolute spread is no bound at
another step: under the mask of step 1 the bias gradient lies in [2, 4), where ONE unit in the last place is 2.4e-7, four times the
6e-8 measured on the dropout-off step (seen on the GPU: the two sides one unit apart there).  They are compared as `_assert_same`
describes instead: either side is run 8 times at the same step number, and the two sets of bit patterns must overlap."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _dropout_oracle as do
from oracle import pose_oracle as po
from rgb_proprioceptive_pose_estimator_amd import models as M
from rgb_proprioceptive_pose_estimator_amd import ops

from _helpers import CASES, build, load_values

DEV = "cuda"
SEED = 7


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def _i32(v):
    """a 32-bit counter value as the int32 the state tensor stores"""
    return int(np.array(int(v) & 0xFFFFFFFF, dtype=np.uint32).view(np.int32))


def _state(step=0):
    return torch.tensor([_i32(step)], dtype=torch.int32, device=DEV), torch.full((1,), -5, dtype=torch.int32, device=DEV)


# -- the entry points ------------------------------------------------------------------------------------------------------------

def test_dropout_begin_takes_and_advances_the_counter():
    state, picks = _state(41)
    ops.dropout_begin(state, picks)
    assert picks.item() == 41 and state.item() == 42
    ops.dropout_begin(state, picks)
    assert picks.item() == 42 and state.item() == 43
    state, picks = _state(2 ** 32 - 1)
    ops.dropout_begin(state, picks)
    assert picks.item() == -1 and state.item() == 0      # 2^32 - 1 as the int32 holds it; the counter wrapped


def _input(n, ld, gen):
    x = torch.randn(n, ld, generator=gen)
    # every third element is NaN, +inf, -inf or -0 in turn: with p = 0.5 and 0.1 they fall into dropped and into kept positions (asserted)
    at = torch.arange(0, x.numel(), 3)
    x.view(-1)[at] = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0])[(at // 3) % 4]
    return x


@pytest.mark.parametrize("p", [2.0 ** -32, 0.1, 0.5])
@pytest.mark.parametrize("ld, c0, c1", [(64, 0, 64), (64, 0, 50), (64, 3, 61), (8, 5, 6), (3204, 0, 3200)])
def test_dropout_rows_matches_the_oracle_bit_for_bit(ld, c0, c1, p):
    gen = torch.Generator().manual_seed(ld * 1000 + c0 * 10 + c1)
    desc = ops.dropout_desc(p, SEED)
    for n in (1, 5, 257):
        for site, step in ((0, 3), (2, 2 ** 32 - 2)):
            x = _input(n, ld, gen)
            xn = x.numpy().copy()
            _, picks = _state()
            picks.fill_(_i32(step))
            want = do.dropout_rows(xn, SEED, step, site, p, c0, c1)
            keep = do.keep_mask(SEED, step, site, n, c0, c1, p)
            if p >= 0.1 and n * (c1 - c0) >= 250:      # the special values met both fates
                special = ~np.isfinite(xn[:, c0:c1]) | (do.bits(xn[:, c0:c1]) == 0x80000000)
                assert (special & keep).any() and (special & ~keep).any()
            # in place
            xd = x.to(DEV)
            got = ops.dropout_rows(xd, desc, picks, site=site, c0=c0, c1=c1)
            assert got is xd
            np.testing.assert_array_equal(_bits(xd), do.bits(want), err_msg="in place n=%d site=%d" % (n, site))
            # out of place, from a sentinel: the columns outside [c0, c1) keep it, the input is not written
            xd = x.to(DEV)
            out = torch.full((n, ld), -7.5, device=DEV)
            got = ops.dropout_rows(xd, desc, picks, site=site, c0=c0, c1=c1, out=out)
            assert got is out
            want_out = do.dropout_rows(xn, SEED, step, site, p, c0, c1, out=np.full((n, ld), -7.5, dtype=np.float32))
            np.testing.assert_array_equal(_bits(out), do.bits(want_out), err_msg="out of place n=%d site=%d" % (n, site))
            np.testing.assert_array_equal(_bits(xd), do.bits(xn))
            # a second launch on the same picks: the forward / backward agreement
            again = ops.dropout_rows(x.to(DEV), desc, picks, site=site, c0=c0, c1=c1, out=torch.full((n, ld), -7.5, device=DEV))
            np.testing.assert_array_equal(_bits(again), _bits(out))


def test_dropout_rows_on_row_views_and_unaligned_buffers():
    """a [n, cols] view of a padded row buffer (what headops.new_rows hands out), and a buffer 4 bytes off 16-byte alignment: the
    4-byte path gives the same bits"""
    gen = torch.Generator().manual_seed(5)
    desc, step = ops.dropout_desc(0.5, SEED), 9
    _, picks = _state()
    picks.fill_(step)
    buf = torch.randn(6, 12, generator=gen)
    want = do.dropout_rows(buf.numpy(), SEED, step, 1, 0.5, 0, 10)
    bd = buf.to(DEV)
    ops.dropout_rows(bd[:, :10], desc, picks, site=1)       # columns 10, 11 are the padding: outside the range
    np.testing.assert_array_equal(_bits(bd), do.bits(want))
    flat = torch.zeros(6 * 12 + 1, device=DEV)
    off = flat[1:].view(6, 12)
    off.copy_(buf)
    assert off.data_ptr() % 16 == 4
    ops.dropout_rows(off, desc, picks, site=1, c1=10)
    np.testing.assert_array_equal(_bits(off), do.bits(want))
    for bad in (dict(c0=-1), dict(c1=13), dict(c0=4, c1=4), dict(site=4), dict(site=-1), dict(out=torch.zeros(6, 11, device=DEV)),
                dict(out=torch.zeros(6, 12, device=DEV, dtype=torch.float64))):
        with pytest.raises(ValueError):
            ops.dropout_rows(bd, desc, picks, **bad)
    from rgb_proprioceptive_pose_estimator_amd._lib import RpeError
    with pytest.raises(RpeError, match="overlap"):
        ops.dropout_rows(bd[:5], desc, picks, out=bd[1:])
    import rgb_proprioceptive_pose_estimator_amd.torch_ops  # noqa: F401  (registers torch.ops.rpe.*)
    y = torch.ops.rpe.dropout_rows(buf.to(DEV), [float(SEED), 0.0, 0.5], picks, 1, 0, 10)      # the dispatcher's form: a copy
    np.testing.assert_array_equal(_bits(y), do.bits(want))
    st, pk = _state(4)
    torch.ops.rpe.dropout_begin(st, pk)
    assert (pk.item(), st.item()) == (4, 5)


# -- the models ------------------------------------------------------------------------------------------------------------------

def _batch(kind, seed_offset=1):
    cfg, lead, wseed, dseed = CASES[kind]
    b = po.synth_batch(lead, dseed + seed_offset, with_depth=cfg.get("use_depth", False))
    return {k: (None if v is None else v.to(DEV)) for k, v in b.items()}


def _model(kind):
    cfg, lead, wseed, dseed = CASES[kind]
    model = build(kind, cfg, torch.float32)
    load_values(model, kind, po.make_state(kind, cfg, wseed))
    return model.to(DEV).train()


def _crit():
    return M.PoseDistanceLoss(distance_metric="combined", scale_factor=1.0, alpha=0.5, mode="pose")


def _step(model, kind, b, backward=True):
    """one forward (+ backward) -> {name: tensor}: outputs, loss, every parameter gradient"""
    for p in model.parameters():
        p.grad = None
    out = model(b["img"], b["depth"], b["x0bar"])
    crit = _crit()
    if kind in ("n", "td"):
        outs, loss = tuple(out), crit(out[0], b["x0"]) + crit(out[1], b["x1"])
    else:
        outs, loss = (out,), crit(out, b["obj"])
    res = {"out%d" % i: o.detach().clone() for i, o in enumerate(outs)}
    res["loss"] = loss.detach().clone()
    if backward:
        loss.backward()
        for name, p in model.named_parameters():
            if p.grad is not None:
                res["grad:" + name] = p.grad.detach().clone()
    torch.cuda.synchronize()
    return res


RUNS = 16        # dropout-off steps that measure the parent's run-to-run spread
RERUNS = 8       # steps per side where a tensor the parent cannot reproduce is compared (see _assert_same)
_BASE = {}


def _steps(model, kind, b, runs, at=None):
    """`runs` steps on one input; at: the step number every one of them is taken at (the counter is set back before each)"""
    out = []
    for _ in range(runs):
        if at is not None:
            model._drop_state.fill_(at)
        out.append(_step(model, kind, b))
    return out


def _baseline(kind):
    """-> (the dropout-off model, RUNS of its steps on _batch(kind), {tensor: spread} of the tensors whose bits moved between them: the
    largest |difference| of any two runs).  The first run is kept whole, of the others only the tensors that moved.  Computed once per
    class and shared; nothing in it is written afterwards."""
    if kind not in _BASE:
        plain, b = _model(kind), _batch(kind)
        runs = _steps(plain, kind, b, RUNS)
        loose = {}
        for k in runs[0]:
            if not all(torch.equal(r[k].view(torch.int32), runs[0][k].view(torch.int32)) for r in runs[1:]):
                stack = torch.stack([r[k].double() for r in runs])
                loose[k] = float((stack.max(0).values - stack.min(0).values).max())
        print("run-to-run spread of the dropout-off %s step over %d runs: %d of %d tensors not bit-identical %r" % (kind, RUNS, len(loose), len(runs[0]), loose))
        _BASE[kind] = (plain, [runs[0]] + [{k: r[k] for k in loose} for r in runs[1:]], loose)
    return _BASE[kind]


def _patterns(runs, k):
    return {r[k].cpu().numpy().tobytes() for r in runs if k in r}


def _assert_same(got, want, loose, label):
    """got, want: lists of steps of the two sides (one each where `loose` is empty).  A tensor the parent reproduces bit for bit is
    compared bit for bit, in every run.  A tensor in `loose` -- one the PARENT's step does not reproduce run to run, because it is
    summed with float atomics in an order that varies -- takes one of a few neighbouring bit patterns per run on either side; the
    parent's absolute spread was measured at other gradient values and does not carry over to a step under another mask, so the two
    sides are run RERUNS times each and must have a bit pattern in common: the same sum, in one of its orders."""
    assert sorted(got[0]) == sorted(want[0]) and set(loose) <= set(want[0]), label
    for k in want[0]:
        assert torch.isfinite(want[0][k]).all(), (label, k)
        if k in loose:
            assert len(got) >= RERUNS and len(want) >= RERUNS, (label, k)
            assert _patterns(got, k) & _patterns(want, k), "%s: %s has no bit pattern in common over %d and %d runs" % (label, k, len(got), len(want))
            continue
        for g in got:
            if k in g:
                assert torch.equal(g[k].view(torch.int32), want[0][k].view(torch.int32)), \
                    "%s: %s differs (max |d| = %.3g)" % (label, k, float((g[k].double() - want[0][k].double()).abs().max()))


def _torch_drop(model, seed, log=None):
    """replace model._drop by a torch formulation at the same sites: the oracle's mask for the step read from the device"""
    def _drop(site, x, out=None, c0=0, c1=None):
        step = int(model._drop_picks.item()) & 0xFFFFFFFF
        n, cols = x.shape
        c1 = cols if c1 is None else c1
        p = model._drop_p[0 if site == 0 else 1]
        keep = torch.from_numpy(do.keep_mask(seed, step, site, n, c0, c1, p)).to(x.device)
        scale = float(do.thresh_scale(p)[1])
        res = torch.where(keep, x[:, c0:c1] * scale, torch.zeros((), device=x.device))
        dst = x if out is None else out
        dst[:, c0:c1] = res
        if log is not None:
            log.append((site, step, n, c0, c1, out is not None))
        return dst
    model._drop = _drop
    return model


SITES = {"no": [0], "n": [0], "td": [0, 1, 2], "tdo": [0, 1], "tdo_v2": [0, 1, 2]}


def _set(model, kind, **kw):
    return model.set_dropout(feature=0.5, seed=SEED, **kw) if kind in ("n", "no") else model.set_dropout(feature=0.5, hidden=0.5, seed=SEED, **kw)


@pytest.mark.parametrize("kind", list(CASES))
def test_train_step_matches_the_torch_formulation(kind):
    b = _batch(kind)
    plain, base, loose = _baseline(kind)
    reruns = RERUNS if loose else 1
    model = _set(_model(kind), kind)
    assert model._drop_state.item() == 0
    got = _steps(model, kind, b, reruns, at=0)
    assert model._drop_state.item() == 1 and model._drop_picks.item() == 0      # one begin per training forward
    log = []
    twin = _torch_drop(_set(_model(kind), kind), SEED, log)
    want = _steps(twin, kind, b, reruns, at=0)
    assert twin._drop_state.item() == 1
    log = log[:2 * len(SITES[kind])]      # (the first of those steps)
    # every site was visited once forward and once backward, all at step 0; the hidden sites forward out of place
    assert sorted((s, oop) for s, _, _, _, _, oop in log) == sorted([(s, s != 0) for s in SITES[kind]] + [(s, False) for s in SITES[kind]]), log
    assert {step for _, step, _, _, _, _ in log} == {0}
    L = CASES[kind][0]["latent_dim"] + (0 if kind == "n" else 3136)
    assert all((c0, c1) == (0, L) for s, _, _, c0, c1, _ in log if s == 0)      # the proprioceptive columns lie behind c1
    _assert_same(got, want, loose, kind)
    # ... and dropout did something: the step differs from the dropout-off one, and the next step from this one
    assert not torch.equal(got[0]["out0"], base[0]["out0"]) and not torch.equal(got[0]["loss"], base[0]["loss"])
    nxt = _steps(model, kind, b, reruns, at=1)
    assert model._drop_state.item() == 2 and not torch.equal(nxt[0]["loss"], got[0]["loss"])
    _assert_same(nxt, _steps(twin, kind, b, reruns, at=1), loose, kind + " step 1")


def _engine_census(model, fn):
    """the engine's per-launch profile (the facility of tests/test_gpu_launch_census.py) around fn(): {kernel symbol: launches}"""
    from rgb_proprioceptive_pose_estimator_amd._lib import lib
    plan = model._plan
    lib.rpe_resnet50_profile(plan.handle, 1)
    fn()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    nbytes = lib.rpe_resnet50_profile_kernels(plan.handle, buf, len(buf))
    lib.rpe_resnet50_profile(plan.handle, 0)
    assert nbytes > 0
    launches = {}
    for line in buf.raw[:nbytes].decode().splitlines():
        name, cnt = line.split(";")[:2]
        launches[name] = launches.get(name, 0) + int(cnt)
    return launches


def _count_calls(monkeypatch):
    """count the calls of the two dropout entry points: every dropout launch of the package goes through them"""
    from rgb_proprioceptive_pose_estimator_amd import _lib
    calls = {"rpe_dropout_begin": 0, "rpe_dropout_rows_f32": 0}
    for name in calls:
        real = getattr(_lib.lib, name)

        def counted(*a, _real=real, _name=name):
            calls[_name] += 1
            return _real(*a)
        monkeypatch.setattr(_lib.lib, name, counted)
    return calls


@pytest.mark.parametrize("kind", list(CASES))
def test_dropout_off_changes_nothing(kind, monkeypatch):
    """set_dropout() with zeros == a model that never called it: bits, launches, counter.  And with dropout ON, every forward that keeps
    no state for a backward is the dropout-off forward, and the counter stays."""
    b = _batch(kind)
    plain, base, loose = _baseline(kind)
    reruns = RERUNS if loose else 1
    census_plain = _engine_census(plain, lambda: _step(plain, kind, b))
    calls = _count_calls(monkeypatch)
    zero = _model(kind).set_dropout(0.0, 0.0, seed=SEED)
    assert zero._drop_desc == {} and zero._drop_state.item() == 0
    _assert_same(_steps(zero, kind, b, reruns), base, loose, kind + " zeros")
    census_zero = _engine_census(zero, lambda: _step(zero, kind, b))
    assert census_zero == census_plain and sum(census_zero.values()) > 100
    assert calls == {"rpe_dropout_begin": 0, "rpe_dropout_rows_f32": 0} and zero._drop_state.item() == 0
    # dropout on: +1 begin and +1 per active site forward and backward, the engine's own launches unchanged
    model = _set(_model(kind), kind)
    _steps(model, kind, b, reruns)
    census_on = _engine_census(model, lambda: _step(model, kind, b))
    assert census_on == census_plain
    steps = reruns + 1
    assert calls == {"rpe_dropout_begin": steps, "rpe_dropout_rows_f32": steps * 2 * len(SITES[kind])} and model._drop_state.item() == steps
    # forwards that keep no state: eval, features_only + heads_only, no_grad in train mode
    # (the reference is `zero`: bit-identical to the plain model, and with the same history of training forwards -- `reruns` steps and the
    # census step, then the no_grad one -- as `model`, so the BatchNorm running statistics the eval forward reads are the same)
    with torch.no_grad():
        want_train = _step(zero, kind, b, backward=False)
        zero.eval()
        zero.reset_initial_state(CASES[kind][1][-1])
        want_eval = _step(zero, kind, b, backward=False)
    for k in calls:
        calls[k] = 0
    with torch.no_grad():
        got_train = _step(model, kind, b, backward=False)
    model.eval()
    model.reset_initial_state(CASES[kind][1][-1])
    got_eval = _step(model, kind, b, backward=False)      # grad enabled, eval mode
    lead, rows = model.features_only(b["img"], b["depth"])
    halves = model.heads_only(rows, lead, b["x0bar"])
    halves = halves if isinstance(halves, tuple) else (halves,)
    torch.cuda.synchronize()
    for k in ("loss",) + tuple(k for k in want_eval if k.startswith("out")):
        assert torch.equal(got_train[k].view(torch.int32), want_train[k].view(torch.int32)), (kind, "no_grad", k)
        assert torch.equal(got_eval[k].view(torch.int32), want_eval[k].view(torch.int32)), (kind, "eval", k)
    for i, h in enumerate(halves):
        assert torch.equal(h.reshape(-1).view(torch.int32), want_eval["out%d" % i].reshape(-1).view(torch.int32)), (kind, "heads_only", i)
    assert calls == {"rpe_dropout_begin": 0, "rpe_dropout_rows_f32": 0} and model._drop_state.item() == steps


def test_naive_classes_refuse_hidden_and_state_stays_put():
    model = _model("no")
    with pytest.raises(ValueError, match="feature"):
        model.set_dropout(feature=0.1, hidden=0.1)
    model.set_dropout(feature=0.1)
    state, picks = model._drop_state, model._drop_picks
    assert state.is_cuda and state.dtype == torch.int32 and "_drop_state" not in dict(model.named_buffers())
    _step(model, "no", _batch("no"))
    model.set_dropout(feature=0.3, seed=3)
    assert model._drop_state is state and model._drop_picks is picks and state.item() == 1      # never reallocated, never reset
    cpu = build("no", CASES["no"][0], torch.float32).set_dropout(feature=0.5)
    assert cpu._drop_state is None
    load_values(cpu, "no", po.make_state("no", CASES["no"][0], CASES["no"][2]))
    cpu.to(DEV).train()
    _step(cpu, "no", _batch("no"))      # allocated when the model first meets the device
    assert cpu._drop_state.is_cuda and cpu._drop_state.item() == 1


# -- the captured step (kept single, small and last) -----------------------------------------------------------------------------

def test_graphed_train_step_draws_a_fresh_mask_at_every_replay():
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import GraphedTrainStep
    kind = "tdo"
    b = _batch(kind)
    batch = (b["img"], b["depth"], b["x0bar"], b["x0"], None, b["obj"])
    criterion = {"obj_loss": _crit(), "val_loss": M.PoseDistanceLoss(mode="val")}
    model = _set(_model(kind), kind)
    opt = FusedAdam(model.parameters(), lr=1e-3, capturable=True)
    warmup = 2
    g = GraphedTrainStep(model, criterion, opt, True, batch, warmup=warmup)
    torch.cuda.synchronize()
    state = model._drop_state
    assert state.item() == warmup      # the warm-up steps advanced the counter, the capture executed nothing
    bufs = list(model.buffers())
    snap = (model._arena.flat.clone(), opt._m.clone(), opt._v.clone(), opt._dev_state.clone(), [t.clone() for t in bufs])

    def restore():
        model._arena.flat.copy_(snap[0]); opt._m.copy_(snap[1]); opt._v.copy_(snap[2]); opt._dev_state.copy_(snap[3])
        for t, s in zip(bufs, snap[4]):
            t.copy_(s)
        model.trunk.weights_changed()

    # the yardstick: the eager loss of this model at one step number, twice (dropout through the kernels)
    def eager_loss(step):
        restore()
        state.fill_(step)
        model.train()
        out = model(b["img"], b["depth"], b["x0bar"])
        return _crit()(out, b["obj"]).detach().clone()

    l0, l1 = eager_loss(warmup), eager_loss(warmup)
    spread = 0.0 if torch.equal(l0, l1) else abs(l0.item() - l1.item())
    print("run-to-run spread of the eager tdo loss: %.3g" % spread)
    # what each replay must give: the eager loss of the `_drop`-substituted model at that replay's step number
    _torch_drop(model, SEED)
    want = [eager_loss(warmup + k) for k in range(2)]
    del model._drop      # back to the class's method (the graph holds the kernels' launches either way)
    state.fill_(warmup)
    got = []
    for k in range(2):
        restore()      # identical input, freshly reloaded identical weights
        torch.cuda.synchronize()
        loss, _, _ = g(batch)
        got.append(loss.detach().clone())
        torch.cuda.synchronize()
        assert state.item() == warmup + k + 1
    assert state.item() == warmup + 2      # advanced by exactly two
    for k in range(2):
        assert torch.isfinite(got[k]).item()
        if spread == 0.0:
            assert torch.equal(got[k], want[k]), (k, got[k].item(), want[k].item())
        else:
            assert abs(got[k].item() - want[k].item()) <= spread, (k, got[k].item(), want[k].item(), spread)
    assert got[0].item() != got[1].item()      # same input, same weights: only the mask moved
