"""GPU side of the frame blur: rpe_blur_frames_u8 against the numpy oracle (tests/_blur_oracle.py).  The arithmetic is integer, so
every comparison is `np.array_equal` -- output, parameter table, guard bytes, step counter -- and then the feature through
FrameAugment (blur in front of the existing augmentation), a captured graph, train() and GraphedTrainStep."""
import numpy as np
import pytest
import torch

import _augment_oracle as ao
import _blur_oracle as bo

pytestmark = pytest.mark.gpu

FULL = 2 ** 32 - 1
GUARD = 64

# the kernel works on tiles of 32 x 32 pixels inside one frame, with a halo of 8 clamped pixels, 4 bytes of a row per thread; rows of
# Ws % 4 == 0 pixels from 4-byte aligned pointers go as dwords, everything else as bytes:
SHAPES = {
    "one_pixel": (1, 1, 1),
    "narrow": (1, 3, 5),            # narrower than every halo: the clamp fires several times over on both sides
    "wide_row": (2, 9, 70),         # three tiles across, the last 6 pixels wide; byte path (70 % 4 != 0)
    "odd": (3, 33, 47),             # a second tile row of one pixel row; byte path
    "grouped": (3, 2, 16, 24),      # (S, N); dword path
    "tiles": (2, 97, 100),          # 3 tiles + 1 row down, 3 tiles + 4 pixels across; dword path (100 % 4 == 0), interior and all edges
    "tiles_odd": (1, 97, 97),       # 3 tiles + 1 pixel in each direction; byte path
}

_INPUTS = {}


def _input(name):
    """seeded frames of one shape with 0 and 255 in them (made once, shared, never written to)"""
    if name not in _INPUTS:
        rng = np.random.default_rng(len(name) * 137 + sum(SHAPES[name]))
        f = rng.integers(0, 256, SHAPES[name] + (3,), dtype=np.uint8)
        if f.size >= 30:
            f.reshape(-1)[::11] = 0
            f.reshape(-1)[5::13] = 255
        f.setflags(write=False)
        _INPUTS[name] = f
    return _INPUTS[name]


def _levels(sigmas):
    t = [bo.gauss_taps(s) for s in sigmas]
    return dict(radius=tuple(r for r, _ in t), taps=tuple(tuple(w) for _, w in t))


def _mixture(**kw):
    """all three kinds drawn: 8 levels over sigma 0.5 .. 2.0, 7 lengths, 16 directions"""
    cx, cy = bo.directions(16)
    d = dict(gauss_thresh=FULL // 3, motion_thresh=FULL // 3, n_lengths=7, dir_cx=tuple(cx), dir_cy=tuple(cy), **_levels([0.5 + 1.5 * s / 7 for s in range(8)]))
    d.update(kw)
    return bo.neutral_desc(**d)


def _freeze(v):
    return tuple(_freeze(x) for x in v) if isinstance(v, (list, tuple)) else v


_ORACLE = {}


def _oracle(frames, desc, step):
    """the oracle's (out, params) of one case, computed once (the inputs are shared read-only arrays)"""
    key = (id(frames), tuple(sorted((k, _freeze(v)) for k, v in desc.items())), step)
    if key not in _ORACLE:
        _ORACLE[key] = bo.blur(frames, desc, step)
    return _ORACLE[key]


def _i32(u):
    return u - (1 << 32) if u >= (1 << 31) else u


def _check(frames, desc, step, offset=0):
    """one launch against the oracle: output, table, guard bytes around `out`, input and counter untouched.  offset: both buffers
    start that many bytes off the 16-byte grid"""
    from rgb_proprioceptive_pose_estimator_amd import ops
    want, want_params = _oracle(frames, desc, step)
    n = frames.size
    b = n // (frames.shape[-3] * frames.shape[-2] * 3)
    g = bo.num_streams(desc, b)
    src = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    dev = src[offset:offset + n].view(frames.shape)
    dev.copy_(torch.from_numpy(frames.copy()))
    buf = torch.full((n + 2 * GUARD + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[GUARD + offset:GUARD + offset + n].view(frames.shape)
    assert dev.data_ptr() % 16 == offset and out.data_ptr() % 16 == offset
    state = torch.tensor([_i32(step), -7], dtype=torch.int32, device="cuda")
    params = torch.full((1 + 4 * g + 2,), -5, dtype=torch.int32, device="cuda")
    got = ops.blur_frames_u8(dev, ops.blur_desc(**desc), state, out=out, params=params)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert state.tolist() == [_i32(step), -7], "the blur launch moved the counter"
    assert np.array_equal(dev.cpu().numpy(), frames), "the input was written"
    got_params = params.cpu().numpy()
    assert np.array_equal(got_params[:1 + 4 * g], want_params) and got_params[1 + 4 * g:].tolist() == [-5, -5]
    whole = buf.cpu().numpy()
    assert (whole[:GUARD + offset] == 0xA5).all() and (whole[GUARD + offset + n:] == 0xA5).all(), "bytes around out were written"
    got = whole[GUARD + offset:GUARD + offset + n].reshape(frames.shape)
    assert np.array_equal(got, want), "%d of %d bytes differ" % ((got != want).sum(), got.size)
    return got, want_params


def _groups(frames):
    return (0, frames.shape[1]) if frames.ndim == 5 else (0,)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_kinds_off_is_a_byte_copy(shape):
    frames = _input(shape)
    for offset in (0, 1):
        got, params = _check(frames, _mixture(seed=11, gauss_thresh=0, motion_thresh=0), step=4, offset=offset)
        assert np.array_equal(got, frames) and (params[1::4] == 0).all()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_radius_pinned(shape):
    frames = _input(shape)
    if frames.size >= 30:
        assert frames.min() == 0 and frames.max() == 255
    for radius, sigma in enumerate((0.0, 0.2, 0.5, 0.9, 1.3, 1.6, 2.0, 2.3, 4.0)):
        lv = _levels([sigma])
        assert lv["radius"] == (radius,)
        for group in _groups(frames):
            got, params = _check(frames, bo.neutral_desc(seed=radius, gauss_thresh=FULL, group=group, **lv), step=2 + radius)
            assert (params[1::4] == 1).all() and (params[2::4] == 0).all()
            if radius == 0:
                assert np.array_equal(got, frames)
    _check(frames, bo.neutral_desc(seed=1, gauss_thresh=FULL, **_levels([4.0])), step=1, offset=1)      # every byte through the byte path


def test_every_length_and_direction_pinned():
    """(L, d): the direction is pinned by a table of one entry, the length by offering 3 .. L and taking the first step at which the
    oracle's table gives frame 0 the length L -- a condition on the inputs, met before the device is asked"""
    frames = _input("odd")
    cx, cy = bo.directions(16)
    for length in range(3, 16, 2):
        nl = (length - 1) // 2
        for d in range(16):
            desc = bo.neutral_desc(seed=100 * length + d, motion_thresh=FULL, n_lengths=nl, dir_cx=(cx[d],), dir_cy=(cy[d],))
            step = next(s for s in range(256) if bo.stream_params(desc, 3, s)["L"][0] == length)
            got, params = _check(frames, desc, step)
            assert (params[1::4] == 2).all() and params[3] == length and (params[4::4] == 0).all()
    # the negative-going components (directions beyond 90 degrees have cx < 0) and the steepest offsets through the byte path
    _check(frames, bo.neutral_desc(seed=3, motion_thresh=FULL, n_lengths=7, dir_cx=(-256, 256), dir_cy=(256, -256)), step=0, offset=1)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_drawn_mixtures(shape):
    frames = _input(shape)
    b = frames.size // (frames.shape[-3] * frames.shape[-2] * 3)
    for group in _groups(frames):
        for offset in (0, 1):
            desc = _mixture(seed=0x9E3779B97F4A7C15, group=group)
            g = bo.num_streams(desc, b)
            if g >= 3:
                # the first step at which the oracle's table shows all three kinds among the streams
                step = next(s for s in range(256) if set(bo.stream_params(desc, g, s)["kind"].tolist()) == {0, 1, 2})
                assert set(bo.blur_params_table(desc, b, step)[1::4].tolist()) == {0, 1, 2}
            else:
                step = 7
            _check(frames, desc, step, offset=offset)
    # the largest seed and step
    _check(frames, _mixture(seed=2 ** 64 - 1), step=FULL)


def test_all_three_kinds_in_one_launch():
    """six frames (the grouped shape, ungrouped) and three (the odd shape): kinds 0, 1 and 2 side by side in one grid"""
    for name in ("grouped", "odd"):
        frames = _input(name)
        b = frames.size // (frames.shape[-3] * frames.shape[-2] * 3)
        desc = _mixture(seed=77)
        step = next(s for s in range(256) if set(bo.stream_params(desc, b, s)["kind"].tolist()) == {0, 1, 2})
        table = bo.blur_params_table(desc, b, step)
        assert set(table[1::4].tolist()) == {0, 1, 2}                                   # on the oracle's table, before the device is asked
        got, params = _check(frames, desc, step)
        assert np.array_equal(params, table)


def test_torch_op_equals_the_wrapper():
    from rgb_proprioceptive_pose_estimator_amd import ops
    import rgb_proprioceptive_pose_estimator_amd.torch_ops  # noqa: F401  (registers torch.ops.rpe.*)
    frames = _input("odd")
    dev = torch.from_numpy(frames.copy()).cuda()
    desc = _mixture(seed=2 ** 63 + 5, gauss_thresh=FULL // 2, motion_thresh=FULL // 2)
    s1, s2 = (torch.tensor([41], dtype=torch.int32, device="cuda") for _ in range(2))
    a = ops.blur_frames_u8(dev, ops.blur_desc(**desc), s1)
    b = torch.ops.rpe.blur_frames_u8(dev, ops.blur_desc_numbers(**desc), s2)
    assert torch.equal(a, b) and s1.item() == 41 and s2.item() == 41
    assert np.array_equal(a.cpu().numpy(), bo.blur(frames, desc, 41)[0]) and not torch.equal(a, dev)
    with pytest.raises(Exception, match="overlap"):
        ops.blur_frames_u8(dev, ops.blur_desc(**desc), s1, out=dev)


# -- through FrameAugment -------------------------------------------------------------------------------------------------------------

ALL = dict(brightness=0.4, contrast=0.5, saturation=0.6, noise_std=4.0, erase_prob=0.5, erase_scale=(0.2, 0.5), erase_fill="noise")
BLUR = dict(blur_prob=0.4, blur_sigma=(0.5, 2.0), motion_blur_prob=0.4, motion_blur_max_length=15)


def _descs(aug, hs, ws, group):
    """the two oracles' descs of a FrameAugment for one frame size"""
    f = dict(aug.desc_fields(hs, ws, group))
    f["fill_rgb"] = (f.pop("fill_r"), f.pop("fill_g"), f.pop("fill_b"))
    return bo.neutral_desc(**aug.blur_desc_fields(group)), ao.neutral_desc(**f)


def _both(frames, bdesc, adesc, step):
    blurred, btable = bo.blur(frames, bdesc, step)
    out, atable, _ = ao.augment(blurred, adesc, step)
    return out, btable, atable


def test_frame_augment_blurs_in_front_of_the_augmentation():
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import FrameAugment
    frames = _input("grouped")
    dev = torch.from_numpy(frames.copy()).cuda()
    kinds = set()
    for per_episode in (True, False):
        aug = FrameAugment(per_episode=per_episode, seed=12, **ALL, **BLUR)
        aug.load_state_dict({"seed": 12, "step": 6})
        group = frames.shape[1] if per_episode else 0
        bdesc, adesc = _descs(aug, 16, 24, group)
        assert bdesc["group"] == adesc["group"] == group
        outs = []
        for step in (6, 7):
            want, btable, atable = _both(frames, bdesc, adesc, step)
            got = aug(dev)
            assert got.data_ptr() != dev.data_ptr() and np.array_equal(got.cpu().numpy(), want)
            assert np.array_equal(aug.last_blur_params.cpu().numpy(), btable) and np.array_equal(aug.last_params.cpu().numpy(), atable)
            assert aug.last_blur_params[0].item() == aug.last_params[0].item() == step      # both tables carry the same step
            assert aug.step == step + 1                                                     # the counter advances by exactly 1 per call
            outs.append(want)
            kinds |= set(btable[1::4].tolist())
        assert not np.array_equal(outs[0], outs[1])
        flat = aug(dev.reshape(-1, 16, 24, 3))                      # a 4-D batch draws per frame whatever per_episode says
        assert np.array_equal(flat.cpu().numpy().reshape(frames.shape), _both(frames, dict(bdesc, group=0), dict(adesc, group=0), 8)[0])
    assert np.array_equal(dev.cpu().numpy(), frames)
    assert kinds == {0, 1, 2}                                       # (the oracle's tables: these steps did blur, both ways, and did not)


def test_frame_augment_without_the_new_keywords_is_unchanged():
    from rgb_proprioceptive_pose_estimator_amd import ops
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import FrameAugment
    frames = _input("odd")
    dev = torch.from_numpy(frames.copy()).cuda()
    aug = FrameAugment(seed=5, **ALL)
    aug.load_state_dict({"seed": 5, "step": 3})
    got = aug(dev)
    state = torch.tensor([3], dtype=torch.int32, device="cuda")
    alone = ops.augment_frames_u8(dev, ops.augment_desc(**aug.desc_fields(33, 47, 0)), state)
    assert torch.equal(got, alone) and aug.last_blur_params is None and aug.step == 4 and not aug.blurs
    assert not any(isinstance(k, tuple) and k and k[0] == "blur" for k in aug._keep)       # no blur buffer was made: no blur launch


def test_captured_call_draws_fresh_numbers_at_every_replay():
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import FrameAugment
    frames = _input("odd")
    static = torch.from_numpy(frames.copy()).cuda()
    aug = FrameAugment(brightness=0.5, contrast=0.5, noise_std=3.0, erase_prob=0.5, seed=4, **BLUR)
    out = torch.empty_like(static)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aug(static, out=out)                                           # step 0: the state, table and blur buffers exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        aug(static, out=out)
    assert aug.step == 1                                               # the capture itself ran nothing
    bdesc, adesc = _descs(aug, 33, 47, 0)
    outs = []
    for step in (1, 2):
        g.replay()
        outs.append(out.cpu().numpy())
        want, btable, atable = _both(frames, bdesc, adesc, step)
        assert np.array_equal(outs[-1], want) and aug.step == step + 1
        assert np.array_equal(aug.last_blur_params.cpu().numpy(), btable) and np.array_equal(aug.last_params.cpu().numpy(), atable)
    assert not np.array_equal(outs[0], outs[1])


# -- through the training loop (the smallest shapes of tests/test_gpu_augment.py's loop tests) ----------------------------------------

def _episode_file(tmp_path, e=4, t=4, hw=64):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset
    rng = np.random.default_rng(0)

    def poses():
        q = rng.normal(size=(e, t, 4))
        return np.concatenate([rng.random((e, t, 3)), q / np.linalg.norm(q, axis=-1, keepdims=True)], -1).astype(np.float32)
    return RecordedEpisodeDataset.save(str(tmp_path / "episodes.npz"), env_name="Lift", imgs=rng.integers(0, 256, (e, t, hw, hw, 3), dtype=np.uint8),
                                       true_self=poses(), true_obj=poses())


def _model(seed=3):
    from rgb_proprioceptive_pose_estimator_amd import models as M
    torch.manual_seed(seed)
    return M.NaiveObjectStateEstimator("cube", [32], 18, 32, False, (9,), False, False, False, compute_dtype=torch.float32).cuda()


def _criterion():
    from rgb_proprioceptive_pose_estimator_amd import models as M
    crit = lambda: M.PoseDistanceLoss("combined", 1.0, 0.5, 1e-4, "pose")
    return {"x0_loss": crit(), "x1_loss": crit(), "obj_loss": crit(), "val_loss": M.PoseDistanceLoss(mode="val")}


def test_train_with_blur(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import FrameAugment, RecordedEpisodeDataset
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import train
    ds = RecordedEpisodeDataset(_episode_file(tmp_path), obj_name="cube")
    model = _model()
    aug = FrameAugment(brightness=0.3, noise_std=2.0, erase_prob=0.5, seed=1, blur_prob=0.5, motion_blur_prob=0.5)
    model, best = train(model, ds, _criterion(), FusedAdam(model.parameters(), lr=1e-3), num_epochs=1, num_train_episodes_per_epoch=2,
                        num_val_episodes_per_epoch=2, params={"camera_name": "frontview", "noise_scale": 0.001}, device="cuda:0", save_model=False,
                        logging=False, augment=aug)
    assert np.isfinite(best)
    assert aug.step == 4                     # 4 train chunks; the 4 val chunks drew nothing
    assert tuple(aug.last_blur_params.shape) == (1 + 4 * 2,) and aug.last_blur_params[0].item() == aug.last_params[0].item() == 3
    assert all(torch.isfinite(v).all() for v in model.state_dict().values() if v.is_floating_point())


def test_graphed_train_step_with_blur():
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import FrameAugment
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import GraphedTrainStep
    g = torch.Generator().manual_seed(2)
    frames = torch.randint(0, 256, (2, 64, 64, 3), generator=g, dtype=torch.uint8)
    batch = (frames.cuda(), None, torch.randn(2, 7, generator=g).cuda(), torch.randn(2, 7, generator=g).cuda(), None, torch.randn(2, 7, generator=g).cuda())
    model = _model().train()
    aug = FrameAugment(brightness=0.3, contrast=0.3, noise_std=2.0, erase_prob=1.0, seed=8, blur_prob=0.5, motion_blur_prob=0.5, motion_blur_max_length=15)
    step = GraphedTrainStep(model, _criterion(), FusedAdam(model.parameters(), lr=1e-3, capturable=True), True, batch, warmup=2, augment=aug)
    assert aug.step == 2
    bdesc, adesc = _descs(aug, 64, 64, 0)
    for k in (2, 3):
        loss, _, _ = step(batch)
        assert torch.isfinite(loss).item() and aug.step == k + 1
        assert np.array_equal(step.fed[0].cpu().numpy(), _both(frames.numpy(), bdesc, adesc, k)[0])       # what the model was fed in replay k
        assert torch.equal(step.static[0].cpu(), frames)
