"""CPU side of the batched evaluator (util.learn_utils.evaluate_episodes): the per-sample fixture recorded from the reference's own
PoseDistanceLoss(mode="val") (tests/golden/pose_errors.npz, tools/gen_pose_errors_golden.py) against the oracle, the dispatcher entry,
the summary text, the chunk-length rule, the noise-sweep construction and the refusal to run without the device."""
import os

import numpy as np
import pytest
import torch

from oracle import pose_oracle as po


def test_golden_rows_match_the_oracle_per_row(golden_dir):
    """every row on its own, at the tolerance tests/test_oracle_golden.py::test_pose_loss_matches_reference uses for the two sums"""
    gold = np.load(os.path.join(golden_dir, "pose_errors.npz"))
    pred, truth = torch.from_numpy(gold["pred"]), torch.from_numpy(gold["truth"])
    assert pred.shape == (257, 7) and truth.shape == (257, 7) and gold["pos"].shape == (257,) and gold["ori"].shape == (257,)
    assert float(gold["w_max"]) < 0.98
    for i in range(257):
        pe, oe = po.pose_loss(pred[i:i + 1], truth[i:i + 1], mode="val")
        np.testing.assert_allclose(float(pe), gold["pos"][i], rtol=1e-6, err_msg=str(i))
        np.testing.assert_allclose(oe, gold["ori"][i], rtol=1e-6, err_msg=str(i))
    np.testing.assert_allclose(np.average(gold["pos"]), gold["pos_average"], rtol=1e-12)
    np.testing.assert_allclose(np.std(gold["pos"]), gold["pos_std"], rtol=1e-12)
    np.testing.assert_allclose(np.average(gold["ori"]), gold["ori_average"], rtol=1e-12)
    np.testing.assert_allclose(np.std(gold["ori"]), gold["ori_std"], rtol=1e-12)


def test_pose_errors_op_is_registered_for_the_device_only():
    from torch._subclasses.fake_tensor import FakeTensorMode

    import rgb_proprioceptive_pose_estimator_amd.torch_ops as T
    assert "pose_errors" in T.NAMES
    assert torch.ops.rpe.pose_errors.default._schema.name == "rpe::pose_errors"
    with pytest.raises(NotImplementedError):
        torch.ops.rpe.pose_errors(torch.randn(3, 7), torch.randn(3, 7), 1e-4)
    with FakeTensorMode():
        p = torch.empty(5, 7, device="cuda")
        pos, ori, pose = torch.ops.rpe.pose_errors(p, torch.empty(5, 7, device="cuda"), 1e-4)
        assert pos.shape == (5,) and ori.shape == (5,) and pose.shape == (5, 7)
        assert pos.dtype == torch.float32 and ori.dtype == torch.float32 and pose.dtype == torch.float32


def _stats(err):
    """the rpe_error_stats layout from numpy, float64"""
    err = np.asarray(err, dtype=np.float64)
    return np.concatenate([[np.average(err), np.std(err), err.max()], err.sum(1), err.mean(1)])


def test_summary_prints_the_reference_lines():
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import EpisodeEvaluation
    pos = np.array([[0.012, 0.034, 0.0564], [0.1, 0.25, 0.4]])
    ori = np.array([[0.5, 1.25, 3.0], [0.001, 0.002, 0.0035]])
    res = EpisodeEvaluation(None, None, None, None, np.stack([_stats(pos), _stats(ori)])[None])
    want = []
    for e in range(2):   # the reference's own format strings applied to the same numbers (util/learn_utils.py:527-538)
        want.append("EPISODE COMPLETED -- Total Pos/Ori err: {:.3f} m / {:.3f} rad, Per-Step Err: {:.3f} m / {:.3f} rad"
                    .format(np.sum(pos[e]), np.sum(ori[e]), np.average(pos[e]), np.average(ori[e])))
    want += ["", "*" * 90,
             "EVALUATION COMPLETED -- Per-Step Pos Mean/Std Err: {:.5f} / {:.5f} m || Ori Mean/Std Err: {:.5f} / {:.5f} rad"
             .format(np.average(pos), np.std(pos), np.average(ori), np.std(ori)), "*" * 90]
    assert res.summary() == "\n".join(want)
    assert res.summary().splitlines()[0] == "EPISODE COMPLETED -- Total Pos/Ori err: 0.102 m / 4.750 rad, Per-Step Err: 0.034 m / 1.583 rad"
    assert res.pos_mean == np.average(pos) and res.ori_std == np.std(ori) and res.pos_max == 0.4
    assert res.pos_episode_sum.shape == (2,) and np.array_equal(res.ori_episode_mean, ori.mean(1))
    # a sweep: one block per scale, every host field with a leading K
    sweep = EpisodeEvaluation(None, None, None, None, np.stack([np.stack([_stats(pos), _stats(ori)]), np.stack([_stats(2 * pos), _stats(ori)])]),
                              noise_scales=[0.0, 0.01])
    lines = sweep.summary().splitlines()
    assert lines[0] == "noise scale 0:" and lines[1:7] == res.summary().splitlines() and lines[7] == "noise scale 0.01:"
    assert sweep.pos_mean.shape == (2,) and sweep.pos_episode_mean.shape == (2, 2) and sweep.pos_mean[1] == np.average(2 * pos)
    with pytest.raises(ValueError):
        EpisodeEvaluation(None, None, None, None, np.zeros((2, 2, 7)))


def test_chunk_length_rule():
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import eval_chunk_length
    assert eval_chunk_length(256, 10) == 25 and eval_chunk_length(6, 3) == 2 and eval_chunk_length(1000, 3) == 333
    assert eval_chunk_length(1, 3) == 1 and eval_chunk_length(256, 257) == 1 and eval_chunk_length(256, 256) == 1
    # the chunks of a 5-step horizon at 2 steps per call: 2, 2, 1 (the last one shorter)
    s = eval_chunk_length(6, 3)
    assert [min(s, 5 - t0) for t0 in range(0, 5, s)] == [2, 2, 1]


def test_noise_sweep_construction():
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import random_poses
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import sweep_draw, sweep_measurements
    x0 = random_poses((3, 5), torch.Generator().manual_seed(2), "cpu")
    z = sweep_draw(3, 5, 7)
    assert z.shape == (3, 5, 7) and torch.equal(z, sweep_draw(3, 5, 7)) and not torch.equal(z, sweep_draw(3, 5, 8))
    assert torch.equal(z, torch.randn((3, 5, 7), generator=torch.Generator().manual_seed(7)))
    scales = [0.0, 0.001, 0.1]
    m = sweep_measurements(x0, scales, z)
    assert m.shape == (3, 3, 5, 7) and torch.equal(m, sweep_measurements(x0, scales, z))
    # one draw for every scale: the position offsets are the same z, scaled
    for k in (1, 2):
        torch.testing.assert_close((m[k, ..., :3] - x0[..., :3]) / scales[k] ** 0.5, z[..., :3], rtol=0, atol=2e-5)
        xb = x0 + scales[k] ** 0.5 * z
        assert torch.equal(m[k, ..., 3:], xb[..., 3:] / xb[..., 3:].norm(dim=-1, keepdim=True))
    # s = 0: the truth, to within 1 ulp (the unit quaternion is divided by its fp32 norm, 1 to within rounding)
    assert torch.equal(m[0, ..., :3], x0[..., :3])
    ulp = torch.abs(torch.nextafter(x0[..., 3:], torch.full_like(x0[..., 3:], 2.0)) - x0[..., 3:])
    assert ((m[0, ..., 3:] - x0[..., 3:]).abs() <= ulp).all()
    # unit quaternions at every scale (fp32 rounding of four squares, a root and a division)
    assert ((m[..., 3:].double().norm(dim=-1) - 1).abs() < 4 * 2.0 ** -24).all()


def test_evaluate_episodes_refuses_cpu_tensors():
    from rgb_proprioceptive_pose_estimator_amd import models as M
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import SyntheticEpisodeDataset
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import evaluate_episodes
    model = M.TemporallyDependentObjectStateEstimator("cube", 32, 18, 32, 2, 0.1, False, (9,), False, False, False, compute_dtype=torch.float32)
    ds = SyntheticEpisodeDataset(horizon=3, obj_name="cube", hw=32, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate_episodes(model, ds, 2, {"camera_name": "frontview", "noise_scale": 0.001})
    assert model.training and model.rollout is False
