"""CPU side of the input pipeline (util.data_utils.TrainInputs): the order of the four device stages and which field of the six-tuple
each replaces, the refusals train() and GraphedTrainStep share through its constructor, the one step counter under the four stage
classes, and the one measurement function under the datasets and the noise sweep.  The stages' arithmetic is checked against their
numpy oracles in tests/test_gpu_sampler.py::test_the_four_stages_together_equal_their_oracles."""
import types

import pytest
import torch

from test_sampler_cpu import _episode_file

SEQ_MODEL = types.SimpleNamespace(use_depth=True, requires_sequence=True, sequence_length=3)
FLAT_MODEL = types.SimpleNamespace(use_depth=True, requires_sequence=False, sequence_length=1)


def _du():
    from rgb_proprioceptive_pose_estimator_amd.util import data_utils
    return data_utils


def _six(lead, g):
    return (torch.randint(0, 256, lead + (4, 4, 3), generator=g, dtype=torch.uint8), torch.rand(lead + (4, 4, 1), generator=g),
            torch.randn(lead + (7,), generator=g), torch.randn(lead + (7,), generator=g), None, torch.randn(lead + (7,), generator=g))


def _recording_stages(tmp_path, calls, sequence_length=3):
    """the four real stage classes with a __call__ that records its name and what it was given, and returns its input (or `out`)"""
    du = _du()

    def recorder(base, name):
        def call(self, x, out=None):
            calls.append((name, x))
            return x if out is None else out
        return type("Recording" + base.__name__, (base,), {"__call__": call})

    ds = du.ResidentEpisodeDataset(_episode_file(tmp_path), device="cpu")
    ds.refresh_data(3)
    drawn = _six((sequence_length, 2), torch.Generator().manual_seed(1))

    class Sampler(du.WindowSampler):
        def __call__(self):
            calls.append(("sampler", None))
            return drawn

    aug = recorder(du.FrameAugment, "augment")()
    return dict(sampler=Sampler(ds, 2, sequence_length=sequence_length), measurement_noise=recorder(du.MeasurementNoise, "measurement_noise")(),
                augment=aug, depth_augment=recorder(du.DepthAugment, "depth_augment")(share_erase=aug)), drawn


def test_stage_order_and_field_placement(tmp_path):
    du = _du()
    calls = []
    stages, drawn = _recording_stages(tmp_path, calls)
    inputs = du.TrainInputs(SEQ_MODEL, **stages)
    fed = inputs()
    assert [c[0] for c in calls] == ["sampler", "measurement_noise", "augment", "depth_augment"]
    # noise reads x0 (field 3) and replaces x0bar (field 2); augment field 0; depth augment field 1; the rest pass through
    assert calls[1][1] is drawn[3] and calls[2][1] is drawn[0] and calls[3][1] is drawn[1]
    assert fed[2] is drawn[3] and fed[0] is drawn[0] and fed[1] is drawn[1]
    assert fed[3] is drawn[3] and fed[4] is None and fed[5] is drawn[5]
    # out=: every stage writes its slot of it (the captured case), and the batch given is the one read
    del calls[:]
    batch, out = _six((3, 2), torch.Generator().manual_seed(2)), _six((3, 2), torch.Generator().manual_seed(3))
    fed = inputs(batch, out=out)
    assert [c[0] for c in calls] == ["sampler", "measurement_noise", "augment", "depth_augment"]
    assert calls[1][1] is batch[3] and calls[2][1] is batch[0] and calls[3][1] is batch[1]
    assert fed[0] is out[0] and fed[1] is out[1] and fed[2] is out[2] and fed[3] is batch[3] and fed[4] is None and fed[5] is batch[5]
    # without a sampler, and with single stages, the other fields are the input's own
    plain_depth = type(stages["depth_augment"])()      # (one without share_erase: it may stand alone)
    for name, stage, src, dst in (("measurement_noise", stages["measurement_noise"], 3, 2), ("augment", stages["augment"], 0, 0),
                                  ("depth_augment", plain_depth, 1, 1)):
        del calls[:]
        fed = du.TrainInputs(SEQ_MODEL, **{name: stage})(batch)
        assert [c[0] for c in calls] == [name] and calls[0][1] is batch[src] and fed[dst] is batch[src]      # (the recorder returns its input)
        assert all(fed[i] is batch[i] for i in range(6) if i != dst)
    # a model without a sequence takes the sampler's S = 1 windows without that dimension
    del calls[:]
    stages, drawn = _recording_stages(tmp_path, calls, sequence_length=1)
    fed = du.TrainInputs(FLAT_MODEL, **stages)()
    assert tuple(fed[0].shape) == (2, 4, 4, 3) and fed[0].data_ptr() == drawn[0].data_ptr() and torch.equal(fed[5], drawn[5][0]) and fed[4] is None
    assert torch.equal(du.model_batch(drawn, False)[3], drawn[3][0]) and du.model_batch(drawn, True) == drawn


def test_no_stage_is_the_identity():
    du = _du()
    batch = _six((2,), torch.Generator().manual_seed(4))
    inputs = du.TrainInputs(None)
    assert inputs(batch) is batch and inputs.fed_like(batch) is batch
    assert inputs.sampler is None and inputs.measurement_noise is None and inputs.augment is None and inputs.depth_augment is None


def test_fed_like_checks_what_the_stages_will_read():
    du = _du()
    batch = _six((2,), torch.Generator().manual_seed(5))
    aug = du.FrameAugment()
    with pytest.raises(ValueError, match="device only"):      # the stages' own checks: host tensors are refused
        du.TrainInputs(None, measurement_noise=du.MeasurementNoise()).fed_like(batch)
    with pytest.raises(ValueError, match="device only"):
        du.TrainInputs(None, augment=aug).fed_like(batch)
    no_depth = (batch[0], None) + batch[2:]
    for call in (du.TrainInputs(FLAT_MODEL, depth_augment=du.DepthAugment()).fed_like, du.TrainInputs(FLAT_MODEL, depth_augment=du.DepthAugment())):
        with pytest.raises(ValueError, match="needs a batch with depth frames"):      # worded once, captured or eager
            call(no_depth)


def test_train_and_the_pipeline_refuse_alike(tmp_path):
    """every bad combination is refused by TrainInputs(...) -- which GraphedTrainStep builds first thing -- and by train(...) with the
    same message, before the model, the optimizer or the device are touched"""
    du = _du()
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import train
    synthetic = du.SyntheticEpisodeDataset(horizon=2, device="cpu")
    assert synthetic.frame_dtype != torch.uint8
    fa = du.FrameAugment(erase_prob=1.0)
    no_depth, with_depth = types.SimpleNamespace(use_depth=False), types.SimpleNamespace(use_depth=True)
    cases = [
        (no_depth, None, dict(depth_augment=du.DepthAugment()), "use_depth"),
        (with_depth, None, dict(depth_augment=fa), "DepthAugment"),
        (with_depth, None, dict(depth_augment=du.DepthAugment(share_erase=fa)), "share_erase"),
        (with_depth, None, dict(augment=du.FrameAugment(), depth_augment=du.DepthAugment(share_erase=fa)), "share_erase"),
        (None, None, dict(measurement_noise=0.001), "MeasurementNoise"),
        (None, None, dict(measurement_noise=fa), "MeasurementNoise"),
        (None, synthetic, dict(augment=fa), "uint8"),
    ]
    for model, dataset, kw, word in cases:
        with pytest.raises(ValueError, match=word) as direct:
            du.TrainInputs(model, dataset, **kw)
        with pytest.raises(ValueError, match=word) as through:
            train(model, synthetic if dataset is None else dataset, {}, None, 1, 1, 1, {}, "cuda:0", **kw)
        assert str(through.value) == str(direct.value), kw
    # a sampler whose windows do not fit the model (train() makes its own sampler, for the model's length: only a caller's can be wrong)
    ds = du.ResidentEpisodeDataset(_episode_file(tmp_path), device="cpu")
    ds.refresh_data(3)
    for model, length in ((FLAT_MODEL, 3), (SEQ_MODEL, 1), (SEQ_MODEL, 2)):
        with pytest.raises(ValueError, match="sampler") as direct:
            du.TrainInputs(model, sampler=ds.sampler(2, sequence_length=length))
        with pytest.raises(ValueError, match="sampler") as later:
            du.TrainInputs(model).draw_from(ds.sampler(2, sequence_length=length))
        assert str(later.value) == str(direct.value)
    assert du.TrainInputs(SEQ_MODEL, sampler=ds.sampler(2, sequence_length=3)).sampler.sequence_length == 3
    assert du.TrainInputs(FLAT_MODEL, sampler=ds.sampler(2)).sampler.sequence_length == 1


def test_one_step_counter_under_the_four_stages(tmp_path):
    du = _du()
    base = du._DeviceStepCounter
    for cls in (du.WindowSampler, du.FrameAugment, du.DepthAugment, du.MeasurementNoise):
        assert issubclass(cls, base)
        assert cls.load_state_dict is base.load_state_dict and cls.state_dict is base.state_dict and cls.step is base.step
        assert cls._wrap_i32 is base._wrap_i32 and cls._kept is base._kept
    for step in (0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1):
        w = base._wrap_i32(step)
        assert -2 ** 31 <= w < 2 ** 31 and w & 0xFFFFFFFF == step
        assert torch.tensor([w], dtype=torch.int32).item() == w      # it does fit the tensor element
    assert [base._wrap_i32(s) for s in (0, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1)] == [0, 2 ** 31 - 1, -2 ** 31, -1]
    ds = du.ResidentEpisodeDataset(_episode_file(tmp_path), device="cpu")
    ds.refresh_data(3)
    for make in (lambda seed: ds.sampler(2, seed=seed), lambda seed: du.FrameAugment(seed=seed), lambda seed: du.DepthAugment(seed=seed),
                 lambda seed: du.MeasurementNoise(seed=seed)):
        s = make(7)
        assert s.step == 0 and s.state_dict() == {"seed": 7, "step": 0}
        s.load_state_dict({"seed": 2 ** 64 - 1, "step": 2 ** 32 - 1})
        assert s.state_dict() == {"seed": 2 ** 64 - 1, "step": 2 ** 32 - 1}
        for bad in ({"seed": -1, "step": 0}, {"seed": 2 ** 64, "step": 0}, {"seed": 0, "step": 2 ** 32}, {"seed": 0, "step": -1}):
            with pytest.raises(ValueError, match="out of range"):
                s.load_state_dict(bad)
        assert s.state_dict() == {"seed": 2 ** 64 - 1, "step": 2 ** 32 - 1}
        for seed in (-1, 2 ** 64):
            with pytest.raises(ValueError, match="seed must fit 64"):
                make(seed)
    # the kept buffers: one per key, made once, never replaced
    n = du.MeasurementNoise()
    made = []
    first = n._kept(("a", 1), lambda: made.append(1) or object())
    assert n._kept(("a", 1), lambda: made.append(2) or object()) is first and made == [1]
    assert n._kept(("a", 2), lambda: made.append(3) or object()) is not first and n._kept(("a", 1), None) is first and made == [1, 3]
    assert du.MeasurementNoise()._keep == {} and du.FrameAugment()._state is None      # nothing is made before the first call


def test_one_measurement_function():
    du = _du()
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import sweep_measurements
    g = torch.Generator().manual_seed(11)
    x0 = du.random_poses((3, 5), g, "cpu")
    z = torch.randn(3, 5, 7, generator=g)
    for scale in (0.001, 0.01, 1, 0.0):
        xb = x0 + (scale ** 0.5) * z      # the expression the function replaces, written out
        want = torch.cat([xb[..., :3], xb[..., 3:] / xb[..., 3:].norm(dim=-1, keepdim=True)], dim=-1)
        got = du.noisy_measurement(x0, scale, z)
        assert got.dtype == torch.float32 and torch.equal(got, want)
        assert torch.equal(sweep_measurements(x0, [scale], z)[0], want)
    # s = 0: the true pose with a renormalised quaternion, whatever the draw
    q = x0[..., 3:]
    truth = torch.cat([x0[..., :3], q / q.norm(dim=-1, keepdim=True)], dim=-1)
    assert torch.equal(sweep_measurements(x0, [0.0, 0.5], z)[0], truth) and torch.equal(sweep_measurements(2.0 * x0, [0], 7.0 * z)[0][..., 3:], truth[..., 3:])
    # the position part is the truth plus the scaled draw, untouched by the renormalisation
    assert torch.equal(du.noisy_measurement(x0, 0.01, z)[..., :3], x0[..., :3] + (0.01 ** 0.5) * z[..., :3])


def test_the_datasets_measure_through_the_function(tmp_path):
    du = _du()
    path = _episode_file(tmp_path)
    ds = du.RecordedEpisodeDataset(path, obj_name="cube", seed=5)
    ds.refresh_data(3, None, 0.01)
    ds.refresh_data(3, None, 0.02)      # the second selection wraps: [3, 0, 1]
    gen = torch.Generator().manual_seed(5)
    torch.randn(3, 7, 7, generator=gen)
    x0 = ds.data["true_self"]
    assert ds.selected == [3, 0, 1] and torch.equal(ds.data["measurement_self"], du.noisy_measurement(x0, 0.02, torch.randn(x0.shape, generator=gen)))
    assert len(ds) == 7 and [tuple(t.shape) for t in ds[6]] == [(3, 8, 8, 3), (0,), (3, 7), (3, 7), (3, 7), (3, 7)]
    with pytest.raises(ValueError, match="were asked for"):
        ds.refresh_data(5)
    syn = du.SyntheticEpisodeDataset(horizon=2, hw=8, device="cpu", obj_name="cube")
    syn.refresh_data(2)
    assert len(syn) == 2 and [tuple(t.shape) for t in syn[1]] == [(2, 3, 8, 8), (0,), (2, 7), (2, 7), (2, 7), (2, 7)]
    assert type(syn).__getitem__ is type(ds).__getitem__
