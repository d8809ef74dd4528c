"""GPU side of the raw-depth / recorded-episode path: the device depth transform (rpe_stage_depth_f32_resized) against Pillow's
mode-F resize through its numpy restatement (tests/_depth_resize.py, pinned to Pillow by tests/test_recorded_cpu.py) -- bit for
bit, no tolerance -- and raw depth through the models, the captured rollout frame, train() and scripts/rollout.py."""
import os

import numpy as np
import pytest
import torch

from _depth_resize import depth_transform, resize, resized_hw

pytestmark = pytest.mark.gpu

# (Hs, Ws) -> (Hr, Wr); None: torchvision's Resize(256) geometry through ops.stage_depth, otherwise the window form with that size
GEOMETRIES = [
    ((84, 84), None),            # -> 256 x 256: upsample
    ((130, 100), None),          # -> 332 x 256: non-square upsample, 3 taps
    ((600, 520), None),          # -> 295 x 256: downsample, 7 taps
    ((255, 256), (256, 256)),    # vertical pass only
    ((256, 255), (256, 256)),    # horizontal pass only
    ((256, 256), None),          # crop only
    ((257, 256), None),          # crop only; (257 - 224) / 2 = 16.5 -> top 16 (half to even)
]
_FRAMES = {}


def _frames(hw, rng_name):
    """3 seeded raw frames of one geometry and value range (made once, shared, never written to)"""
    key = (hw, rng_name)
    if key not in _FRAMES:
        lo, hi = (0.0, 1.0) if rng_name == "unit" else (0.5, 10.0)
        rng = np.random.default_rng(hw[0] * 1000 + hw[1] + (0 if rng_name == "unit" else 1))
        f = (lo + (hi - lo) * rng.random((3,) + hw)).astype(np.float32)
        f.setflags(write=False)
        _FRAMES[key] = f
    return _FRAMES[key]


def _crop_origin(hr, wr, ch, cw):
    return int(round((hr - ch) / 2.0)), int(round((wr - cw) / 2.0))


@pytest.mark.parametrize("rng_name", ["unit", "metres"])
@pytest.mark.parametrize("crop", [(224, 224), (32, 48)])
@pytest.mark.parametrize("hw,to", GEOMETRIES, ids=["%dx%d" % g[0] for g in GEOMETRIES])
def test_stage_depth_equals_pillow_bit_for_bit(hw, to, crop, rng_name):
    from rgb_proprioceptive_pose_estimator_amd import ops
    frames = _frames(hw, rng_name)
    hr, wr = to or resized_hw(*hw)
    if to is None:
        assert (hr, wr) == {(84, 84): (256, 256), (130, 100): (332, 256), (600, 520): (295, 256), (256, 256): (256, 256), (257, 256): (257, 256)}[hw]
    top, left = _crop_origin(hr, wr, *crop)
    if hw == (257, 256) and crop == (224, 224):
        assert top == 16
    want_all = torch.from_numpy(np.ascontiguousarray(resize(frames, hr, wr)[:, None, top:top + crop[0], left:left + crop[1]]))
    for b in (1, 3):
        raw = torch.from_numpy(frames[:b].copy()).cuda()
        if to is None:
            got = ops.stage_depth(raw.unsqueeze(-1), crop_hw=crop, size=256)       # channels-last (B, Hs, Ws, 1), as robosuite gives it
        else:
            got = ops.stage_depth_window(raw, hr, wr, top, left, *crop)
        assert got.dtype == torch.float32 and tuple(got.shape) == (b, 1) + crop
        got, want = got.cpu(), want_all[:b]
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (hw, b, float((got - want).abs().max()))


def test_stage_depth_equals_the_pillow_golden(golden_dir):
    from rgb_proprioceptive_pose_estimator_amd import ops
    gold = np.load(os.path.join(golden_dir, "resize_pil_f32.npz"))
    for i in range(3):
        got = ops.stage_depth(torch.from_numpy(gold["in%d" % i]).cuda()[None, :, :, None]).cpu()
        assert torch.equal(got[0, 0].view(torch.int32), torch.from_numpy(gold["out%d" % i]).view(torch.int32)), i


def test_stage_depth_arguments_and_cached_tables():
    from rgb_proprioceptive_pose_estimator_amd import ops
    from rgb_proprioceptive_pose_estimator_amd._lib import RpeError, lib
    raw = torch.from_numpy(_frames((84, 84), "unit").copy()).cuda()
    with pytest.raises(ValueError, match="smaller than"):
        ops.stage_depth(raw, crop_hw=(300, 224), size=256)                                        # 84 x 84 -> 256 x 256 < 300 rows
    with pytest.raises(ValueError):
        ops.stage_depth(raw.double())
    with pytest.raises(ValueError):
        ops.stage_depth_window(raw, 256, 256, 40, 0, 224, 224)                                   # window leaves the resized frame
    out = torch.empty(1, 224, 224, device="cuda")
    with pytest.raises(RpeError, match="tap tables"):   # a size-changing pass without its tables: status + message, no launch
        lib.rpe_stage_depth_f32_resized(ops._p(raw), ops._p(out), 1, 84, 84, 256, 256, 16, 16, 224, 224, None, None, 0, None, None, 0, ops._stream())
    # the second call with one geometry reuses the device tables: it can be replayed from a captured graph
    a = ops.stage_depth(raw)
    n_tables = len(ops._DEPTH_TABLES)
    ptrs = [t.data_ptr() for tab in ops._depth_tables(84, 84, 256, 256, raw.device) for t in tab[:2]]
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.stage_depth(raw)
    torch.cuda.current_stream().wait_stream(side)
    static = raw.clone()
    with torch.cuda.graph(g):
        b = ops.stage_depth(static)
    static.copy_(raw.flip(0))
    g.replay()
    assert torch.equal(b, ops.stage_depth(raw.flip(0))) and torch.equal(a, ops.stage_depth(raw))
    assert len(ops._DEPTH_TABLES) == n_tables
    assert ptrs == [t.data_ptr() for tab in ops._depth_tables(84, 84, 256, 256, raw.device) for t in tab[:2]]


# -- raw depth through the models -----------------------------------------------------------------------------------------------

HS, WS = 130, 100


def _raw_batch(lead, seed=0):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (*lead, HS, WS, 3), generator=g, dtype=torch.uint8)
    depth = 0.5 + 9.5 * torch.rand(*lead, HS, WS, 1, generator=g)
    x0bar = torch.randn(*lead, 7, generator=g)
    staged = torch.from_numpy(depth_transform(depth[..., 0].numpy())).unsqueeze(-3)      # (..., 1, 224, 224): the host transform
    return img.cuda(), depth.cuda(), staged.cuda(), x0bar.cuda()


def _no_model(dtype, seed=3):
    from rgb_proprioceptive_pose_estimator_amd import models as M
    torch.manual_seed(seed)
    return M.NaiveObjectStateEstimator("cube", [32], 18, 32, False, (9,), True, False, False, compute_dtype=dtype).cuda()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_raw_depth_equals_preprocessed_depth(dtype):
    """the staged depth is bit-identical to the host transform and the forward is deterministic: same output bits"""
    model = _no_model(dtype)
    img, raw, staged, x0bar = _raw_batch((2,))
    model.eval()
    with torch.no_grad():
        a, b = model(img, raw, x0bar), model(img, staged, x0bar)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    model.train()   # forward only: batch statistics, the bn1 head fused into the stem pass
    a, b = model(img, raw, x0bar), model(img, staged, x0bar)
    assert torch.isfinite(a).all() and torch.equal(a.detach(), b.detach())


def test_raw_depth_sequence_model():
    from rgb_proprioceptive_pose_estimator_amd import models as M
    torch.manual_seed(5)
    model = M.TemporallyDependentObjectStateEstimator("hammer", 32, 18, 32, 2, 0.1, False, (9,), True, False, False, compute_dtype=torch.float32).cuda().eval()
    img, raw, staged, x0bar = _raw_batch((2, 2), seed=1)
    assert tuple(raw.shape) == (2, 2, HS, WS, 1) and tuple(staged.shape) == (2, 2, 1, 224, 224)
    with torch.no_grad():
        model.reset_initial_state(2)
        a = model(img, raw, x0bar)
        model.reset_initial_state(2)
        b = model(img, staged, x0bar)
    assert tuple(a.shape) == (2, 2, 7) and torch.isfinite(a).all() and torch.equal(a, b)


def test_preprocessed_depth_beside_uint8_frames_stays(golden_dir):
    """the shape rule leaves the existing path alone: uint8 frames + (N, 1, 224, 224) depth == the all-preprocessed call, to the
    tolerance of tests/test_gpu_train.py::test_uint8_frames_resized_like_pillow"""
    from oracle.pil_resize import reference_transform
    model = _no_model(torch.float32).eval()
    img, _, staged, x0bar = _raw_batch((2,), seed=2)
    host = torch.from_numpy(np.stack([reference_transform(f) for f in img.cpu().numpy()])).cuda()
    with torch.no_grad():
        a, b = model(img, staged, x0bar), model(host, staged, x0bar)
    assert torch.allclose(a, b, rtol=1e-4, atol=1e-5), float((a - b).abs().max())


def test_raw_depth_shape_rule_edges():
    model = _no_model(torch.float32).eval()
    img, raw, staged, x0bar = _raw_batch((2,))
    with torch.no_grad():
        with pytest.raises(ValueError):    # raw-shaped depth beside float (preprocessed) images
            model(torch.zeros(2, 3, 224, 224, device="cuda"), raw, x0bar)
        with pytest.raises(ValueError):    # raw depth of another geometry than the frames
            model(img, raw[:, :64, :64].contiguous(), x0bar)
        model(img, raw, x0bar)             # and the model still runs afterwards


def test_graphed_rollout_frame_with_raw_depth():
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import GraphedRolloutFrame
    model = _no_model(torch.float32).eval()
    frames = [_raw_batch((1,), seed=10 + i) for i in range(4)]
    g = GraphedRolloutFrame(model, frames[0][0], frames[0][1], frames[0][3], calibrate=0)   # (no calibration: the replay itself is under test)
    assert g.replaying
    for img, raw, _, x0bar in frames[1:]:
        got = g(img, raw, x0bar).clone()
        with torch.no_grad():
            want = model(img, raw, x0bar)
        assert torch.equal(got, want)


def test_capture_layer_takes_raw_depth():
    from rgb_proprioceptive_pose_estimator_amd.util.model_utils import capture_layer
    model = _no_model(torch.float32).eval()
    img, raw, staged, _ = _raw_batch((2,))
    a, b = capture_layer(model, "d0", img, raw), capture_layer(model, "d0", img, staged)
    assert tuple(a.shape) == (2, 1, 56, 56) and torch.equal(a, b)


# -- recorded episodes ----------------------------------------------------------------------------------------------------------

def _episode_file(tmp_path, e=3, t=4, hw=64):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset
    rng = np.random.default_rng(0)
    def poses():
        q = rng.normal(size=(e, t, 4))
        return np.concatenate([rng.random((e, t, 3)), q / np.linalg.norm(q, axis=-1, keepdims=True)], -1).astype(np.float32)
    return RecordedEpisodeDataset.save(str(tmp_path / "episodes.npz"), env_name="Lift", imgs=rng.integers(0, 256, (e, t, hw, hw, 3), dtype=np.uint8),
                                       depths=(0.5 + 2.0 * rng.random((e, t, hw, hw, 1))).astype(np.float32), true_self=poses(), true_obj=poses())


def test_train_on_recorded_episodes(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd import models as M
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import train
    ds = RecordedEpisodeDataset(_episode_file(tmp_path), use_depth=True, obj_name="cube")
    model = _no_model(torch.float32)
    crit = lambda: M.PoseDistanceLoss("combined", 1.0, 0.5, 1e-4, "pose")
    criterion = {"x0_loss": crit(), "x1_loss": crit(), "obj_loss": crit(), "val_loss": M.PoseDistanceLoss(mode="val")}
    path = str(tmp_path / "best.pth")
    model, best = train(model, ds, criterion, FusedAdam(model.parameters(), lr=1e-3), num_epochs=1, num_train_episodes_per_epoch=2,
                        num_val_episodes_per_epoch=1, params={"camera_name": "frontview", "noise_scale": 0.001}, device="cuda:0", save_path=path,
                        logging=False)
    assert np.isfinite(best) and os.path.exists(path)
    assert ds.selected == [2]   # train took episodes 0-1, val the next one


def test_rollout_script_on_recorded_episodes(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.scripts.rollout import main
    out = str(tmp_path / "o.npy")
    main(["--model", "no", "--use_depth", "--latent_dim", "32", "--hidden_dim", "32", "--obj_name", "cube", "--episodes", _episode_file(tmp_path),
          "--n_episodes", "2", "--no_graph", "--out", out])
    o = np.load(out)
    assert o.shape == (8, 7) and np.isfinite(o).all()
