"""GPU side of the frame augmentation: rpe_augment_frames_u8 against the numpy oracle (tests/_augment_oracle.py).  The arithmetic is
integer, so every comparison is `np.array_equal` -- output, parameter table, grey sums and step counter -- and then the feature
through FrameAugment, a captured graph, train() and GraphedTrainStep."""
import numpy as np
import pytest
import torch

import _augment_oracle as ao

pytestmark = pytest.mark.gpu

Q1 = 65536
FULL = 2 ** 32 - 1

# the kernel walks the batch as one flat array in groups of 16 pixels, the remainder one pixel per thread:
SHAPES = {
    "tail_only": (1, 5, 7),         # 35 pixels: two groups and three single pixels; every pixel single from a pointer off the 16-byte grid
    "sub_group": (1, 3, 5),         # 15 pixels: fewer than one group
    "odd": (3, 33, 47),             # 1551 pixels per frame: frame boundaries inside groups, waves across frames, more than one block, a tail
    "grouped": (3, 2, 16, 24),      # (S, N): whole groups per frame
    "erasing": (2, 64, 64),
}


def _features(hs, ws):
    """desc settings by name: every feature alone (drawn and pinned), and all together"""
    eh, ew = max(1, hs // 2), max(1, ws // 2)
    rect = dict(eh_lo=1, eh_hi=eh, ew_lo=1, ew_hi=ew)
    f = {
        "neutral": {},
        "brightness_drawn": dict(qb_lo=Q1 // 2, qb_hi=2 * Q1),
        "brightness_pinned": dict(qb_lo=2 * Q1, qb_hi=2 * Q1),
        "contrast_drawn": dict(qc_lo=0, qc_hi=3 * Q1),
        "contrast_pinned": dict(qc_lo=0, qc_hi=0),
        "saturation_drawn": dict(qs_lo=0, qs_hi=4 * Q1),
        "saturation_pinned": dict(qs_lo=0, qs_hi=0),
        "noise": dict(noise_q=3000),
        "noise_strong": dict(noise_q=Q1),
        "erase_constant": dict(erase_thresh=FULL, fill_rgb=(1, 2, 3), **rect),
        "erase_random": dict(erase_thresh=FULL, fill_mode=1, **rect),
        "erase_half": dict(erase_thresh=1 << 31, **rect),
        "all": dict(qb_lo=Q1 // 2, qb_hi=2 * Q1, qc_lo=Q1 // 4, qc_hi=3 * Q1, qs_lo=0, qs_hi=3 * Q1, noise_q=5000, erase_thresh=3 << 30, fill_mode=1, **rect),
        "all_no_contrast": dict(qb_lo=Q1 // 2, qb_hi=2 * Q1, qs_lo=0, qs_hi=3 * Q1, noise_q=5000, erase_thresh=3 << 30, **rect),   # the skipped reduction
    }
    return f


_INPUTS = {}


def _input(name):
    """seeded frames of one shape with 0 and 255 in them (made once, shared, never written to)"""
    if name not in _INPUTS:
        rng = np.random.default_rng(len(name) * 131 + sum(SHAPES[name]))
        f = rng.integers(0, 256, SHAPES[name] + (3,), dtype=np.uint8)
        f.reshape(-1)[::11] = 0
        f.reshape(-1)[5::13] = 255
        f.setflags(write=False)
        _INPUTS[name] = f
    return _INPUTS[name]


def _to_desc(d):
    from rgb_proprioceptive_pose_estimator_amd import ops
    d = dict(d)
    r, g, b = d.pop("fill_rgb")
    return ops.augment_desc(fill_r=r, fill_g=g, fill_b=b, **d)


def _device_frames(frames, misaligned=False):
    """the frames on the device; misaligned: at a byte offset of 3 from the allocation (off the 16-byte grid)"""
    t = torch.from_numpy(frames.copy())
    if not misaligned:
        return t.cuda()
    buf = torch.empty(t.numel() + 3, dtype=torch.uint8, device="cuda")
    view = buf[3:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0
    return view


_ORACLE = {}


def _oracle(frames, desc, step):
    """the oracle's (out, params, sums) of one case, computed once (the inputs are shared read-only arrays)"""
    key = (id(frames), tuple(sorted(desc.items())), step)
    if key not in _ORACLE:
        _ORACLE[key] = ao.augment(frames, desc, step)
    return _ORACLE[key]


def _i32(u):
    """a 32-bit word as the int32 tensor element that holds it"""
    return u - (1 << 32) if u >= (1 << 31) else u


def _desc_of(aug, hs, ws, group):
    """the oracle's desc of a FrameAugment for one frame size"""
    f = dict(aug.desc_fields(hs, ws, group))
    f["fill_rgb"] = (f.pop("fill_r"), f.pop("fill_g"), f.pop("fill_b"))
    return ao.neutral_desc(**f)


def _check(frames, desc, step, in_place=False, misaligned=False):
    from rgb_proprioceptive_pose_estimator_amd import ops
    want, want_params, want_sums = _oracle(frames, desc, step)
    b = frames.size // (frames.shape[-3] * frames.shape[-2] * 3)
    g = ao.num_streams(desc, b)
    dev = _device_frames(frames, misaligned)
    state = torch.tensor([_i32(step), -7], dtype=torch.int32, device="cuda")
    params = torch.full((1 + 8 * g + 2,), -5, dtype=torch.int32, device="cuda")
    sums = torch.full((b + 1,), -9, dtype=torch.int64, device="cuda")
    out = ops.augment_frames_u8(dev, _to_desc(desc), state, out=dev if in_place else None, params=params, sums=sums)
    if in_place:
        assert out.data_ptr() == dev.data_ptr()
    else:
        assert np.array_equal(dev.cpu().numpy(), frames), "the input was written"
    assert state.tolist() == [_i32((step + 1) & FULL), -7]
    got_params = params.cpu().numpy()
    assert np.array_equal(got_params[:1 + 8 * g], want_params) and got_params[1 + 8 * g:].tolist() == [-5, -5]
    contrast = not (desc["qc_lo"] == Q1 and desc["qc_hi"] == Q1)
    got_sums = sums.cpu().numpy()
    assert got_sums[b] == -9
    if contrast:
        assert np.array_equal(got_sums[:b].astype(np.uint64), want_sums)
    else:
        assert (got_sums[:b] == -9).all()      # the reduction is skipped
    got = out.cpu().numpy()
    assert got.shape == frames.shape and np.array_equal(got, want), "%d of %d bytes differ" % ((got != want).sum(), got.size)
    return got


@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_equals_the_oracle(shape):
    frames = _input(shape)
    assert frames.min() == 0 and frames.max() == 255
    hs, ws = frames.shape[-3:-1]
    groups = (0, frames.shape[1]) if frames.ndim == 5 else (0,)
    for i, (name, kw) in enumerate(_features(hs, ws).items()):
        for group in groups:
            desc = ao.neutral_desc(seed=0x9E3779B97F4A7C15 + i, group=group, **kw)
            got = _check(frames, desc, step=3 + i)
            if name == "neutral":
                assert np.array_equal(got, frames)
            if name == "brightness_pinned":
                assert (got[frames >= 128] == 255).all() and (frames >= 128).any()          # the upper clamp fires
            if name == "noise_strong" and frames.size >= 3000:
                assert (got[frames == 255] == 255).any() and (got[frames == 0] == 0).any()   # both clamps fire
            _check(frames, desc, step=3 + i, in_place=True)
    # every pixel through the one-pixel path
    for name in ("all", "all_no_contrast"):
        _check(frames, ao.neutral_desc(seed=5, **_features(hs, ws)[name]), step=9, misaligned=True)
        _check(frames, ao.neutral_desc(seed=5, **_features(hs, ws)[name]), step=9, misaligned=True, in_place=True)


def test_erase_fills_and_step_extremes():
    frames = _input("erasing")
    rect = dict(erase_thresh=FULL, eh_lo=8, eh_hi=40, ew_lo=8, ew_hi=40)
    const = _check(frames, ao.neutral_desc(seed=2, fill_rgb=(250, 0, 7), **rect), step=0)
    rnd = _check(frames, ao.neutral_desc(seed=2, fill_mode=1, **rect), step=0)
    assert (const != frames).any() and (rnd != frames).any() and not np.array_equal(const, rnd)
    # the largest seed and step: the counter wraps to 0
    _check(frames, ao.neutral_desc(seed=2 ** 64 - 1, fill_mode=1, noise_q=2000, qc_lo=Q1 // 2, qc_hi=Q1, **rect), step=FULL)


def test_consecutive_calls_and_frame_augment():
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import FrameAugment
    frames = _input("grouped")
    dev = torch.from_numpy(frames.copy()).cuda()
    for per_episode in (True, False):
        aug = FrameAugment(brightness=0.4, contrast=0.5, saturation=0.6, noise_std=4.0, erase_prob=0.5, erase_scale=(0.2, 0.5), erase_fill="noise",
                           per_episode=per_episode, seed=12)
        aug.load_state_dict({"seed": 12, "step": 6})
        group = frames.shape[1] if per_episode else 0
        desc = _desc_of(aug, 16, 24, group)
        assert desc["group"] == group and desc["eh_lo"] == 3 and desc["ew_hi"] == 12
        for step in (6, 7):
            want, want_params, _ = ao.augment(frames, desc, step)
            got = aug(dev)
            assert got.data_ptr() != dev.data_ptr() and np.array_equal(got.cpu().numpy(), want)
            assert np.array_equal(aug.last_params.cpu().numpy(), want_params) and aug.step == step + 1
        assert aug.state_dict() == {"seed": 12, "step": 8}
        flat = aug(dev.reshape(-1, 16, 24, 3))                      # a 4-D batch draws per frame whatever per_episode says
        assert np.array_equal(flat.cpu().numpy().reshape(frames.shape), ao.augment(frames, dict(desc, group=0), 8)[0])
    assert np.array_equal(dev.cpu().numpy(), frames)


def test_torch_op_equals_the_wrapper():
    from rgb_proprioceptive_pose_estimator_amd import ops
    import rgb_proprioceptive_pose_estimator_amd.torch_ops  # noqa: F401  (registers torch.ops.rpe.*)
    frames = _input("odd")
    dev = torch.from_numpy(frames.copy()).cuda()
    fields = dict(seed=77, qb_lo=Q1 // 2, qb_hi=2 * Q1, qc_lo=Q1 // 2, qc_hi=2 * Q1, qs_lo=0, qs_hi=2 * Q1, noise_q=4000, erase_thresh=1 << 31, eh_lo=2, eh_hi=20,
                  ew_lo=2, ew_hi=30, fill_mode=1, fill_r=9, fill_g=8, fill_b=7, group=0)
    s1, s2 = (torch.tensor([41], dtype=torch.int32, device="cuda") for _ in range(2))
    a = ops.augment_frames_u8(dev, ops.augment_desc(**fields), s1)
    b = torch.ops.rpe.augment_frames_u8(dev, [fields[k] for k in ops.AUGMENT_DESC_FIELDS], s2)
    assert torch.equal(a, b) and s1.item() == 42 and s2.item() == 42
    assert not torch.equal(a, dev)


def test_captured_call_draws_fresh_numbers_at_every_replay():
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import FrameAugment
    frames = _input("odd")
    static = torch.from_numpy(frames.copy()).cuda()
    aug = FrameAugment(brightness=0.5, contrast=0.5, saturation=0.5, noise_std=3.0, erase_prob=0.5, seed=4)
    out = torch.empty_like(static)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aug(static, out=out)                                           # step 0: the state and table buffers exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        aug(static, out=out)
    assert aug.step == 1                                               # the capture itself ran nothing
    desc = _desc_of(aug, 33, 47, 0)
    outs = []
    for step in (1, 2):
        g.replay()
        outs.append(out.cpu().numpy())
        assert np.array_equal(outs[-1], ao.augment(frames, desc, step)[0]) and aug.step == step + 1
    assert not np.array_equal(outs[0], outs[1])


# -- through the training loop ----------------------------------------------------------------------------------------------------

def _episode_file(tmp_path, e=4, t=4, hw=64):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset
    rng = np.random.default_rng(0)
    def poses():
        q = rng.normal(size=(e, t, 4))
        return np.concatenate([rng.random((e, t, 3)), q / np.linalg.norm(q, axis=-1, keepdims=True)], -1).astype(np.float32)
    return RecordedEpisodeDataset.save(str(tmp_path / "episodes.npz"), env_name="Lift", imgs=rng.integers(0, 256, (e, t, hw, hw, 3), dtype=np.uint8),
                                       true_self=poses(), true_obj=poses())


def _model(seed=3):
    """ResNet-18 trunk, latent 32, no depth head (its two InstanceNorm scalars are summed with float atomics: runs would not repeat bitwise)"""
    from rgb_proprioceptive_pose_estimator_amd import models as M
    torch.manual_seed(seed)
    return M.NaiveObjectStateEstimator("cube", [32], 18, 32, False, (9,), False, False, False, compute_dtype=torch.float32).cuda()


def _criterion():
    from rgb_proprioceptive_pose_estimator_amd import models as M
    crit = lambda: M.PoseDistanceLoss("combined", 1.0, 0.5, 1e-4, "pose")
    return {"x0_loss": crit(), "x1_loss": crit(), "obj_loss": crit(), "val_loss": M.PoseDistanceLoss(mode="val")}


def _train(tmp_path, **kw):
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import train
    ds = RecordedEpisodeDataset(_episode_file(tmp_path), obj_name="cube")
    model = _model()
    model, best = train(model, ds, _criterion(), FusedAdam(model.parameters(), lr=1e-3), num_epochs=1, num_train_episodes_per_epoch=2,
                        num_val_episodes_per_epoch=2, params={"camera_name": "frontview", "noise_scale": 0.001}, device="cuda:0", save_model=False,
                        logging=False, **kw)
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, best


def test_train_with_augmentation(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import FrameAugment
    plain, best_plain = _train(tmp_path)
    none, best_none = _train(tmp_path, augment=None)
    assert best_plain == best_none and all(torch.equal(plain[k], none[k]) for k in plain)   # augment=None: nothing changes
    aug = FrameAugment(brightness=0.3, contrast=0.3, saturation=0.3, noise_std=2.0, erase_prob=0.5, seed=1)
    sd, best = _train(tmp_path, augment=aug)
    assert np.isfinite(best)
    assert aug.step == 4                     # 4 train chunks (horizon 4, one timestep per chunk); the 4 val chunks drew nothing
    assert tuple(aug.last_params.shape) == (1 + 8 * 2,) and aug.last_params[0].item() == 3
    assert any(not torch.equal(sd[k], plain[k]) for k in plain)     # and the train phase did see other pixels


def test_graphed_train_step_with_augmentation():
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import FrameAugment
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import GraphedTrainStep
    g = torch.Generator().manual_seed(2)
    frames = torch.randint(0, 256, (2, 64, 64, 3), generator=g, dtype=torch.uint8)
    batch = (frames.cuda(), None, torch.randn(2, 7, generator=g).cuda(), torch.randn(2, 7, generator=g).cuda(), None, torch.randn(2, 7, generator=g).cuda())
    model = _model().train()
    aug = FrameAugment(brightness=0.3, contrast=0.3, noise_std=2.0, erase_prob=1.0, seed=8)
    step = GraphedTrainStep(model, _criterion(), FusedAdam(model.parameters(), lr=1e-3, capturable=True), True, batch, warmup=2, augment=aug)
    assert aug.step == 2 and step.fed[0].data_ptr() != step.static[0].data_ptr()
    desc = _desc_of(aug, 64, 64, 0)
    for k in (2, 3):
        loss, _, _ = step(batch)
        assert torch.isfinite(loss).item() and aug.step == k + 1
        assert np.array_equal(step.fed[0].cpu().numpy(), ao.augment(frames.numpy(), desc, k)[0])       # what the model was fed in replay k
        assert torch.equal(step.static[0].cpu(), frames)
    with pytest.raises(ValueError):
        GraphedTrainStep(model, _criterion(), FusedAdam(model.parameters(), lr=1e-3, capturable=True), True,
                         (torch.zeros(2, 3, 224, 224, device="cuda"),) + batch[1:], warmup=1, augment=aug)
