"""CPU side of the raw-depth / recorded-episode path: the Pillow mode-F resize restatement against Pillow's own output, the double
tap tables the device kernel multiplies with, and the RecordedEpisodeDataset contract.  No GPU."""
import os

import numpy as np
import pytest
import torch

from _depth_resize import depth_transform, tables
from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset, pil_bilinear_tables, pil_bilinear_tables_f64


def test_restatement_equals_pillow_bit_for_bit(golden_dir):
    gold = np.load(os.path.join(golden_dir, "resize_pil_f32.npz"))
    for i, hw in enumerate(((84, 84), (130, 100), (200, 180))):
        frame, want = gold["in%d" % i], gold["out%d" % i]
        assert frame.shape == hw and frame.dtype == np.float32 and want.shape == (224, 224) and want.dtype == np.float32
        assert frame.min() >= 0.5 and frame.max() < 10.0
        assert np.array_equal(depth_transform(frame), want), (i, str(gold["pillow_version"]))


@pytest.mark.parametrize("sizes", [(84, 256), (100, 256), (600, 295), (255, 256), (130, 332), (520, 256), (1000, 365)])
def test_f64_tables_equal_the_restatement(sizes):
    bounds, kk = pil_bilinear_tables_f64(*sizes)
    rb, rk = tables(*sizes)
    assert bounds.dtype == np.int32 and kk.dtype == np.float64 and kk.flags["C_CONTIGUOUS"]
    assert np.array_equal(bounds, rb) and kk.shape == rk.shape and np.array_equal(kk, rk)
    # every row's taps lie inside the source and inside the table: what the kernel's reads rely on
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= sizes[0]).all() and (bounds[:, 1] <= kk.shape[1]).all()


@pytest.mark.parametrize("sizes", [(84, 256), (100, 256), (600, 295), (255, 256)])
def test_f64_bounds_equal_the_u8_tables_bounds(sizes):
    assert np.array_equal(pil_bilinear_tables_f64(*sizes)[0], pil_bilinear_tables(*sizes)[0])


# -- RecordedEpisodeDataset ---------------------------------------------------------------------------------------------------------

E, T, HS, WS = 3, 4, 10, 12


def _arrays(seed=0):
    rng = np.random.default_rng(seed)
    def poses():
        q = rng.normal(size=(E, T, 4))
        return np.concatenate([rng.random((E, T, 3)), q / np.linalg.norm(q, axis=-1, keepdims=True)], -1).astype(np.float32)
    return {"imgs": rng.integers(0, 256, (E, T, HS, WS, 3), dtype=np.uint8), "depths": rng.random((E, T, HS, WS, 1), dtype=np.float32),
            "true_self": poses(), "true_other": poses(), "true_obj": poses()}


def _file(tmp_path, name="ep.npz", drop=(), **over):
    arrays = {k: v for k, v in _arrays().items() if k not in drop}
    path = str(tmp_path / name)
    RecordedEpisodeDataset.save(path, **{**arrays, **over})
    return path, arrays


def test_save_load_round_trip(tmp_path):
    path, arrays = _file(tmp_path, env_name="TwoArmLift")
    assert os.path.exists(path)
    ds = RecordedEpisodeDataset(path, use_depth=True, obj_name="cube")
    assert type(ds.env).__name__ == "TwoArmLift" and ds.env.horizon == T and ds.is_two_arm
    ds.refresh_data(E)
    for k, v in arrays.items():
        assert np.array_equal(ds.data[k].numpy(), v), k
    # the default environment name, and tensors as input
    p2 = RecordedEpisodeDataset.save(str(tmp_path / "b.npz"), imgs=torch.from_numpy(arrays["imgs"]), true_self=torch.from_numpy(arrays["true_self"]))
    d2 = RecordedEpisodeDataset(p2)
    assert type(d2.env).__name__ == "Recorded" and not d2.is_two_arm


def test_getitem_shapes_and_dtypes(tmp_path):
    path, arrays = _file(tmp_path)
    ds = RecordedEpisodeDataset(path, use_depth=True, obj_name="cube")
    ds.refresh_data(2, "frontview", 0.001)
    assert len(ds) == T and not hasattr(ds, "chunk")
    img, depth, x0bar, x0, x1, obj = ds[1]
    assert not any(t.is_cuda for t in (img, depth, x0bar, x0, x1, obj))
    assert img.dtype == torch.uint8 and tuple(img.shape) == (2, HS, WS, 3)
    assert depth.dtype == torch.float32 and tuple(depth.shape) == (2, HS, WS, 1)
    for t in (x0bar, x0, x1, obj):
        assert t.dtype == torch.float32 and tuple(t.shape) == (2, 7)
    assert np.array_equal(img.numpy(), arrays["imgs"][:2, 1]) and np.array_equal(depth.numpy(), arrays["depths"][:2, 1])
    assert np.array_equal(x0.numpy(), arrays["true_self"][:2, 1]) and np.array_equal(obj.numpy(), arrays["true_obj"][:2, 1])
    # without depth / object / second arm: the placeholders of the reference's contract
    plain = RecordedEpisodeDataset(path)
    plain.refresh_data(1)
    img, depth, x0bar, x0, x1, obj = plain[0]
    assert depth.numel() == 0 and tuple(x1.shape) == tuple(obj.shape) == (1, 7)


def test_refresh_walks_through_the_file_and_wraps(tmp_path):
    path, arrays = _file(tmp_path)
    ds = RecordedEpisodeDataset(path)
    ds.refresh_data(2)
    assert ds.selected == [0, 1] and np.array_equal(ds.data["true_self"].numpy(), arrays["true_self"][[0, 1]])
    ds.refresh_data(2)
    assert ds.selected == [2, 0] and np.array_equal(ds.data["imgs"].numpy(), arrays["imgs"][[2, 0]])
    ds.refresh_data(3)
    assert ds.selected == [1, 2, 0]
    with pytest.raises(ValueError):
        ds.refresh_data(E + 1)


def test_measurement_noise(tmp_path):
    path, arrays = _file(tmp_path)
    a, b, c = (RecordedEpisodeDataset(path, seed=s) for s in (7, 7, 8))
    for ds in (a, b, c):
        ds.refresh_data(E, noise_scale=0.01)
    m = a.data["measurement_self"]
    assert torch.allclose(m[..., 3:].norm(dim=-1), torch.ones(E, T), atol=1e-6)         # unit quaternions
    assert torch.equal(m, b.data["measurement_self"]) and not torch.equal(m, c.data["measurement_self"])   # seeded
    err = m[..., :3] - torch.from_numpy(arrays["true_self"][..., :3])
    assert 0.03 < float(err.std()) < 0.3                                                   # N(0, 0.01 I): sigma 0.1
    a.refresh_data(E, noise_scale=0.01)
    assert not torch.equal(a.data["measurement_self"], m)                                 # the generator advances per refresh
    a.refresh_data(E, noise_scale=0.0)
    assert torch.allclose(a.data["measurement_self"], a.data["true_self"], atol=1e-6)


def test_constructor_errors(tmp_path):
    no_depth, _ = _file(tmp_path, "nd.npz", drop=("depths",))
    with pytest.raises(ValueError, match="depths"):
        RecordedEpisodeDataset(no_depth, use_depth=True)
    RecordedEpisodeDataset(no_depth)
    no_obj, _ = _file(tmp_path, "no.npz", drop=("true_obj",))
    with pytest.raises(ValueError, match="true_obj"):
        RecordedEpisodeDataset(no_obj, obj_name="cube")
    two_arm, _ = _file(tmp_path, "ta.npz", drop=("true_other",), env_name="TwoArmHandoff")
    with pytest.raises(ValueError, match="true_other"):
        RecordedEpisodeDataset(two_arm)
    # wrong ranks / dtypes: refused by save(), and by the constructor for a file written some other way
    a = _arrays()
    bad = [dict(a, imgs=a["imgs"].astype(np.float32)), dict(a, imgs=a["imgs"][..., 0]), dict(a, depths=a["depths"][..., 0]),
           dict(a, depths=a["depths"].astype(np.float64)), dict(a, true_self=a["true_self"][..., :6]), dict(a, true_obj=a["true_obj"][:2]),
           dict(a, true_other=a["true_other"].astype(np.float64)), {k: v for k, v in a.items() if k != "true_self"}]
    for i, arrays in enumerate(bad):
        with pytest.raises(ValueError):
            RecordedEpisodeDataset.save(str(tmp_path / "bad.npz"), **arrays)
        path = str(tmp_path / ("bad%d.npz" % i))
        np.savez(path, **arrays)
        with pytest.raises(ValueError):
            RecordedEpisodeDataset(path)
