"""GPU tests of the on-device gradient-norm clip and the AdamW update: rpe_grad_sumsq + rpe_clip_coef and rpe_adamw_step_clip one
call at a time, FusedAdam / FusedAdamW over a small arena step by step, and one eager + one graph-replayed train step of the toy
model -- every stored value within its bound of tests/_clip_bounds.py (fp64 references built on the device from the same fp32
operands; the bounds as tests/test_clip_cpu.py holds them on the inputs of tests/_clip_cases.py)."""
import ctypes

import pytest
import torch

import _bounds as B
import _clip_bounds as CB
import _clip_cases as C

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from rgb_proprioceptive_pose_estimator_amd import ops
    from rgb_proprioceptive_pose_estimator_amd._lib import lib, raw

DEV = "cuda"
GUARD = 7.0
HP_ARGS = (C.HP["lr"], C.HP["b1"], C.HP["b2"], C.HP["eps"])


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _state(step=0.0, skip=0.0, coef=1.0):
    return torch.tensor([1.0, 1.0, 0.0, skip, 0.0, float(step), -3.0, float(coef)], dtype=torch.float32).to(DEV)


def _pad4(n):
    return (n + 3) // 4 * 4


# ------------------------------------------------------------------ operator level: norm and coefficient
def _norm_and_coef(segs, max_norm):
    """rpe_grad_sumsq per segment (16-byte aligned starts in one buffer, as in the arena; its own row offset in one partials buffer)
    + rpe_clip_coef -> (state block, partial rows) on the host.  One guard row behind the partials stays as it was."""
    offs, at = [], 0
    for s in segs:
        offs.append(at)
        at += _pad4(s.numel())
    buf = torch.full((at + 4,), GUARD)
    for s, o in zip(segs, offs):
        buf[o:o + s.numel()] = s
    buf = buf.to(DEV)
    rows = [lib.rpe_grad_sumsq_rows(s.numel()) for s in segs]
    part = torch.full((sum(rows) + 1,), GUARD, dtype=torch.float64, device=DEV)
    st = _state(step=5.0)
    r0 = 0
    for s, o, r in zip(segs, offs, rows):
        lib.rpe_grad_sumsq(_P(buf[o:]), s.numel(), _P(part[r0:]), _S())
        r0 += r
    lib.rpe_clip_coef(_P(part), r0, max_norm, _P(st), _S())
    st, part, after = st.cpu(), part.cpu(), buf.cpu()
    assert float(part[-1]) == GUARD, "rpe_grad_sumsq wrote behind its partial rows"
    for s, o in zip(segs, offs):
        assert torch.equal(_bits(after[o:o + s.numel()]), _bits(s)), "rpe_grad_sumsq changed the gradient"
    assert st[:6].tolist() == [1.0, 1.0, 0.0, 0.0, 0.0, 5.0], "rpe_clip_coef touched the loss scaler's part of the state block"
    return st, part[:-1]


def _segments(n, kind):
    if n == "split":
        return [C.grad_case(k, kind, seed=i) for i, k in enumerate(C.SPLIT)]
    return [C.grad_case(n, kind)]


@pytest.mark.parametrize("n", C.GPU_NS + ["full", "split"])
def test_norm_and_coefficient(n):
    """norm and coefficient within their bound for unit, tiny, 1e-20 and 1e20 gradients (fp32 squares would underflow / overflow),
    exact for zero gradients (0 and 1), the reference's non-finite pattern for one inf (inf, 0) and one NaN (NaN, NaN); a second
    run gives the same bits (partial rows included); max_norm 0 or inf only measures.  `full`: 5 elements more than one full pass of
    the capped grid (a second trip and a live tail); `split`: three odd-length segments into one partials buffer."""
    if n == "full":
        n = C.full_pass_n(lib.rpe_grad_sumsq_rows)
    for kind in C.KINDS + tuple(C.NONFINITE):
        segs = _segments(n, kind)
        for mx in ((1.0,) if kind in C.NONFINITE else C.max_norms(kind)):
            st, part = _norm_and_coef(segs, mx)
            st2, part2 = _norm_and_coef(segs, mx)
            assert torch.equal(_bits(st), _bits(st2)) and torch.equal(_bits(part), _bits(part2)), "two runs differ (%s, %s)" % (kind, mx)
            rn, rc = CB.clip_ref(segs, mx)
            label = "n=%s %s max_norm=%g" % (n, kind, mx)
            for name, got, fx in (("norm", st[6], rn), ("coef", st[7], rc)):
                got = got.double()
                assert bool(torch.isnan(got)) == bool(torch.isnan(fx.v)) and bool(torch.isinf(got)) == bool(torch.isinf(fx.v)), \
                    "%s %s: got %r, reference %r" % (label, name, float(got), float(fx.v))
                if torch.isfinite(fx.v):
                    B.assert_within(got, *fx.out(), "clip %s %s" % (name, label))
                elif torch.isinf(fx.v):
                    assert float(got) == float(fx.v)
            if kind == "zero":
                assert float(st[6]) == 0.0 and float(st[7]) == 1.0
            if kind == "inf":
                assert float(st[7]) == 0.0
        if kind in ("unit", "nan"):       # measure only: the coefficient is 1 whatever the norm
            for mx in (0.0, float("inf")):
                st, _ = _norm_and_coef(segs, mx)
                assert float(st[7]) == 1.0, (kind, mx, float(st[7]))
                assert torch.equal(_bits(st[6]), _bits(_norm_and_coef(segs, 1.0)[0][6]))


def test_clip_coef_without_rows_and_bad_arguments():
    """rows = 0 (weight decay without clipping): norm 0, coefficient 1, no partials read; bad arguments are refused"""
    st = _state()
    lib.rpe_clip_coef(None, 0, 0.0, _P(st), _S())
    assert st[6:].tolist() == [0.0, 1.0]
    g = torch.zeros(16, device=DEV)
    part = torch.zeros(4, dtype=torch.float64, device=DEV)
    assert raw.rpe_grad_sumsq(_P(g), 0, _P(part), _S()) != 0
    assert raw.rpe_grad_sumsq(ctypes.c_void_p(g.data_ptr() + 4), 8, _P(part), _S()) == 3      # RPE_ERR_ALIGN
    assert raw.rpe_clip_coef(None, 2, 1.0, _P(st), _S()) != 0 and raw.rpe_clip_coef(_P(part), -1, 1.0, _P(st), _S()) != 0
    torch.cuda.synchronize()
    assert not part.any()


# ------------------------------------------------------------------ operator level: the update
def _dev4(ts):
    """each operand with 4 guard elements behind it, on the device"""
    return [torch.cat([t, torch.full((4,), GUARD)]).to(DEV) for t in ts]


@pytest.mark.parametrize("n", C.GPU_NS + ["full"])
def test_adamw_step_clip_elementwise(n):
    """rpe_adamw_step_clip: p, m and v element-wise within the bounds of adamw_clip_ref at steps 1 .. 1000, weight decay 0 / 1e-2 / 0.1,
    with and without the coefficient (the fp32 value of clip_ref at max_norm 1e-3, placed in the state block; 1e20 gradients only
    clipped).  g stays bitwise, as do 4 guard elements behind every buffer; without decay and coefficient the result also meets the
    bounds of _bounds.adam_ref, and zero gradients with zero moments leave p bitwise; a set skip flag leaves everything bitwise; a
    pointer off by 4 bytes is refused and nothing is written."""
    if n == "full":
        n = C.full_pass_n(lib.rpe_grad_sumsq_rows)
    for kind in C.KINDS:
        for step in C.STEPS:
            p, g, m, v = C.clip_case(n, step, kind)
            coef = CB.clip_ref([g], 1e-3)[1].v.to(torch.float32)
            ops_dev = [t.to(DEV) for t in (p, g, m, v)]            # the references are built on the device
            for wd in C.WDS:
                for use_clip in (0, 1):
                    if kind == "huge" and not use_clip:
                        continue
                    pd, gd, md, vd = _dev4((p, g, m, v))
                    st = _state(step, coef=float(coef))
                    lib.rpe_adamw_step_clip(_P(pd), _P(gd), _P(md), _P(vd), n, *HP_ARGS, wd, _P(st), use_clip, _S())
                    label = "n=%d %s step=%d wd=%g clip=%d" % (n, kind, step, wd, use_clip)
                    assert torch.equal(_bits(gd[:n]), _bits(g)), "g was written: " + label
                    for t in (pd, gd, md, vd):
                        assert (t[n:] == GUARD).all(), "wrote behind a buffer: " + label
                    ref = CB.adamw_clip_ref(*ops_dev, step, float(coef) if use_clip else None, wd=wd, **C.HP)
                    for k, t in zip("pmv", (pd, md, vd)):
                        B.assert_within(t[:n], *ref[k], "adamw_step_clip %s %s" % (k, label), "i")
                    if wd == 0.0 and not use_clip:
                        plain = B.adam_ref(*ops_dev, step, **C.HP)
                        for k, t in zip("pmv", (pd, md, vd)):
                            B.assert_within(t[:n], *plain[k], "adamw_step_clip vs adam_ref %s %s" % (k, label), "i")
                    if kind == "zero" and wd == 0.0:
                        assert torch.equal(_bits(pd[:n]), _bits(p)) and not md[:n].any() and not vd[:n].any(), "a zero update moved something"
    # skip flag set (fp16: non-finite gradients): nothing moves
    p, g, m, v = C.clip_case(n, 10, "unit")
    bufs = _dev4((p, g, m, v))
    st = _state(10, skip=1.0, coef=0.5)
    lib.rpe_adamw_step_clip(*(_P(t) for t in bufs), n, *HP_ARGS, 0.1, _P(st), 1, _S())
    for t, t0 in zip(bufs, (p, g, m, v)):
        assert torch.equal(_bits(t[:n]), _bits(t0)), "rpe_adamw_step_clip moved a buffer although skip is set"
    # 16-byte alignment of every buffer
    for bad in range(4):
        ptrs = [ctypes.c_void_p(t.data_ptr() + (4 if i == bad else 0)) for i, t in enumerate(bufs)]
        rc = raw.rpe_adamw_step_clip(*ptrs, max(1, n - 1), *HP_ARGS, 0.1, _P(st), 0, _S())
        assert rc == 3, "rpe_adamw_step_clip took a misaligned pointer (status %d)" % rc
    torch.cuda.synchronize()
    for t, t0 in zip(bufs, (p, g, m, v)):
        assert torch.equal(_bits(t[:n]), _bits(t0)), "rpe_adamw_step_clip wrote although it returned the alignment error"


# ------------------------------------------------------------------ optimizer level
def _check_step(label, segs, before, after, grad, state, step, max_norm, wd, lr=1e-3):
    """One optimizer step against the one-step reference from a snapshot: before / after = (p, m, v) flat buffers, grad the flat
    gradient the step read, state the device state block after it.  Norm and coefficient against clip_ref over the segments, then
    every element of every segment against adamw_clip_ref carrying the coefficient's bound."""
    coef = None
    if max_norm is not None:
        rn, rc = CB.clip_ref([grad[lo:hi] for lo, hi in segs], max_norm)
        B.assert_within(state[6], *rn.out(), label + " norm")
        B.assert_within(state[7], *rc.out(), label + " coef")
        coef = rc if max_norm != float("inf") else None
    hp = dict(C.HP, lr=lr)
    for lo, hi in segs:
        ref = CB.adamw_clip_ref(before[0][lo:hi], grad[lo:hi], before[1][lo:hi], before[2][lo:hi], step, coef, wd=wd, **hp)
        for k, t in zip("pmv", after):
            B.assert_within(t[lo:hi], *ref[k], "%s %s [%d:%d]" % (label, k, lo, hi), "i")


def _tiny_module(seed=3):
    """parameter sizes 1, 7, 10 and 33; the third frozen: two trainable segments, [0, 12) and [24, 60)"""
    torch.manual_seed(seed)
    mod = torch.nn.Module()
    for name, n in (("a", 1), ("b", 7), ("c", 10), ("d", 33)):
        mod.register_parameter(name, torch.nn.Parameter(torch.randn(n, device=DEV)))
    mod.c.requires_grad_(False)
    return mod


@pytest.mark.parametrize("variant", ["clip", "decay", "clip+decay capturable", "measure only"])
def test_optimizer_steps_one_by_one(variant):
    """FusedAdam / FusedAdamW over a two-segment arena, five steps with fresh gradients written into arena.grad (scales from far
    above to far below the threshold), each step checked on its own against the one-step reference from a snapshot of (p, m, v, g):
    no error compounds.  The frozen parameter and the gradients never move; grad_norm / clip_coef are None until a clipped step
    ran and the state block's views afterwards; the step count lives on the device."""
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam, FusedAdamW
    from rgb_proprioceptive_pose_estimator_amd.params import ParamArena
    mod = _tiny_module()
    arena = ParamArena(mod)
    segs = arena.trainable_segments()
    assert segs == [(0, 12), (24, 60)]
    if variant == "clip":
        opt, mx, wd = FusedAdam(mod.parameters(), max_grad_norm=1.0), 1.0, 0.0
    elif variant == "decay":
        opt, mx, wd = FusedAdam(mod.parameters(), weight_decay=0.1), None, 0.1
    elif variant == "clip+decay capturable":
        opt, mx, wd = FusedAdamW(mod.parameters(), capturable=True, max_grad_norm=0.5), 0.5, 1e-2
    else:
        opt, mx, wd = FusedAdam(mod.parameters(), max_grad_norm=float("inf")), float("inf"), 0.0
    assert opt.grad_norm is None and opt.clip_coef is None
    gen = torch.Generator().manual_seed(11)
    clipped = []
    for k, scale in enumerate((1.0, 1e-2, 30.0, 1e-8, 0.2), start=1):
        arena.grad.copy_(torch.randn(arena.numel, generator=gen) * scale)
        if k == 1:
            opt._ensure()
        before = (arena.flat.clone(), opt._m.clone(), opt._v.clone())
        g0 = arena.grad.clone()
        opt.step()
        assert torch.equal(_bits(arena.grad), _bits(g0)), "the step wrote the gradient"
        assert opt._dev_state[5].item() == float(k)
        _check_step("%s step %d" % (variant, k), segs, before, (arena.flat, opt._m, opt._v), g0, opt._dev_state, k, mx, wd)
        for t, t0 in zip((arena.flat, opt._m, opt._v), before):
            assert torch.equal(_bits(t[12:24]), _bits(t0[12:24])), "the frozen parameter moved"
        if mx is None:
            assert opt.grad_norm is None and opt.clip_coef is None
        else:
            assert opt.grad_norm.data_ptr() == opt._dev_state[6].data_ptr() and opt.clip_coef.data_ptr() == opt._dev_state[7].data_ptr()
            assert opt.grad_norm.dim() == 0 and opt.grad_norm.is_cuda
            clipped.append(opt.clip_coef.item() < 1.0)
    if variant in ("clip", "clip+decay capturable"):
        assert clipped == [True, False, True, False, True], clipped      # norms ~ 7 s: 7, 0.07, 200, 7e-8, 1.4
    if variant == "measure only":
        assert clipped == [False] * 5


@pytest.mark.parametrize("capturable", [False, True])
def test_without_options_the_launches_are_todays(capturable):
    """no option set: parameters and moments bit-identical to the launches FusedAdam.step issued before the options existed
    (rpe_adam_step per segment with the host's step count; capturable: the step bump + rpe_adam_step_amp), and nothing of the clip
    path is created"""
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.params import ParamArena
    mod = _tiny_module()
    arena = ParamArena(mod)
    opt = FusedAdam(mod.parameters(), lr=1e-3, capturable=capturable, weight_decay=0.0, max_grad_norm=None)
    flat, m, v = arena.flat.clone(), torch.zeros_like(arena.flat), torch.zeros_like(arena.flat)
    st = _state()
    st[6:] = 0.0
    gen = torch.Generator().manual_seed(12)
    for k in range(1, 4):
        arena.grad.copy_(torch.randn(arena.numel, generator=gen))
        opt.step()
        for lo, hi in arena.trainable_segments():
            if capturable:
                if lo == 0:
                    lib.rpe_amp_update(_P(st), 1.0, 1.0, 1 << 30, _S())
                lib.rpe_adam_step_amp(_P(flat[lo:hi]), _P(arena.grad[lo:hi]), _P(m[lo:hi]), _P(v[lo:hi]), hi - lo, *HP_ARGS, _P(st), _S())
            else:
                ops.adam_step(flat[lo:hi], arena.grad[lo:hi], m[lo:hi], v[lo:hi], *HP_ARGS, k)
    for got, want in ((arena.flat, flat), (opt._m, m), (opt._v, v)):
        assert torch.equal(_bits(got), _bits(want))
    assert opt._partials is None and opt._clip_state is None and opt.grad_norm is None
    assert (opt._dev_state is not None) == capturable
    if capturable:
        assert opt._dev_state[6:].tolist() == [0.0, 0.0]


# ------------------------------------------------------------------ model level
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


MAX_NORM = 1e-3


def test_train_step_clips_eager_and_replayed():
    """the fp32 toy model of test_graphed_train_step_matches_eager with max_grad_norm = 1e-3: one eager train step and one replay of
    the captured step from the same restored state, each checked element by element against the reference computed from ITS OWN
    arena.grad (so the aux head's atomic-order noise needs no tolerance) -- after asserting that the step did clip"""
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import GraphedTrainStep, train_step
    batches, criterion = _toy_batches()
    m = _toy(torch.float32)
    opt = FusedAdam(m.parameters(), lr=1e-3, capturable=True, max_grad_norm=MAX_NORM)
    g = GraphedTrainStep(m, criterion, opt, True, batches[0], warmup=2)
    torch.cuda.synchronize()
    arena, segs = m._arena, m._arena.trainable_segments()
    assert opt.grad_norm.item() > MAX_NORM and opt.clip_coef.item() < 1.0, "the warm-up steps did not clip"
    bufs = list(m.buffers())
    snap = (arena.flat.clone(), opt._m.clone(), opt._v.clone(), opt._dev_state.clone(), [b_.clone() for b_ in bufs])
    train_step(m, batches[1], criterion, opt, True, "train", None)
    assert opt.grad_norm.item() > MAX_NORM and opt.clip_coef.item() < 1.0
    assert opt._dev_state[5].item() == 3.0
    _check_step("eager", segs, snap[:3], (arena.flat, opt._m, opt._v), arena.grad, opt._dev_state, 3, MAX_NORM, 0.0)
    assert (arena.flat - snap[0]).abs().max().item() > 1e-5
    arena.flat.copy_(snap[0]); opt._m.copy_(snap[1]); opt._v.copy_(snap[2]); opt._dev_state.copy_(snap[3])
    for b_, s_ in zip(bufs, snap[4]):
        b_.copy_(s_)
    g(batches[1])
    torch.cuda.synchronize()
    assert opt._dev_state[5].item() == 3.0 and opt.grad_norm.item() > MAX_NORM and opt.clip_coef.item() < 1.0
    _check_step("replay", segs, snap[:3], (arena.flat, opt._m, opt._v), arena.grad, opt._dev_state, 3, MAX_NORM, 0.0)
    assert (arena.flat - snap[0]).abs().max().item() > 1e-5      # the replay did train


def test_train_step_clips_f16():
    """the same single eager step for the fp16 toy model: the loss scaler's unscale pass runs first, the norm is that of the
    UNSCALED gradient left in arena.grad, and norm / coefficient share the scaler's state block"""
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdamW
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import train_step
    batches, criterion = _toy_batches()
    m = _toy(torch.float16)
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-2, max_grad_norm=MAX_NORM)
    m._materialize(torch.device("cuda", torch.cuda.current_device()))
    arena = m._arena
    opt._ensure()
    for _ in range(4):      # a step the loss scaler skips (an overflow at its initial scale) halves the scale: take the first real one
        before = (arena.flat.clone(), opt._m.clone(), opt._v.clone())
        train_step(m, batches[1], criterion, opt, True, "train", None)
        st = arena.loss_scaler.state
        if st[3].item() == 0.0:
            break
        for t, t0 in zip((arena.flat, opt._m, opt._v), before):
            assert torch.equal(_bits(t), _bits(t0)), "a skipped step moved something"
    assert opt._dev_state is None and opt.grad_norm.data_ptr() == st[6].data_ptr()
    assert st[3].item() == 0.0 and st[5].item() == 1.0, "no fp16 step was taken: %s" % (st.tolist(),)
    assert opt.grad_norm.item() > MAX_NORM and opt.clip_coef.item() < 1.0
    _check_step("f16", arena.trainable_segments(), before, (arena.flat, opt._m, opt._v), arena.grad, st, 1, MAX_NORM, 1e-2)
