"""Host side of episodes of unequal length: the `lengths` array of the episode file, the numpy oracle of the ragged window index
(tests/_ragged_oracle.py), the sampler's host figures, write_video(lengths=...), and the refusals of train() and of the two scripts,
all of which come before a device is touched."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _ragged_oracle as ro
import _sampler_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (9, 3, 2, 4, 5, 1)      # with S = 3, stride = 2, T = 9: K = (4, 1, 0, 1, 2, 0), M = 8
T, S, STRIDE = 9, 3, 2


def _poses(rng, t):
    q = rng.normal(size=(t, 4))
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    return np.concatenate([rng.random((t, 3)), np.where(q[..., 3:] < 0, -q, q)], -1).astype(np.float32)


def _episodes(lengths=LENGTHS, hw=8, seed=0):
    rng = np.random.default_rng(seed)
    return [dict(imgs=rng.integers(0, 256, (t, hw, hw, 3), dtype=np.uint8), true_self=_poses(rng, t), true_obj=_poses(rng, t)) for t in lengths]


def _packed(tmp_path, lengths=LENGTHS, name="ragged.npz"):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset
    return RecordedEpisodeDataset.pack(str(tmp_path / name), _episodes(lengths), env_name="Lift")


# -- the file format --------------------------------------------------------------------------------------------------------------

def test_pack_and_save_round_trip(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset
    eps = _episodes()
    path = RecordedEpisodeDataset.pack(str(tmp_path / "r.npz"), eps, env_name="Lift")
    with np.load(path) as f:
        assert f["lengths"].dtype == np.int32 and f["lengths"].tolist() == list(LENGTHS) and f["imgs"].shape == (6, T, 8, 8, 3)
        for e, ep in enumerate(eps):
            n = LENGTHS[e]
            for k, v in ep.items():
                assert np.array_equal(f[k][e, :n], v) and not f[k][e, n:].any(), (e, k)      # the episode, then zeros
        arrays = {k: f[k] for k in f.files if k != "env_name"}
    ds = RecordedEpisodeDataset(path, obj_name="cube")
    assert ds.lengths.tolist() == list(LENGTHS) and type(ds.env).__name__ == "Lift" and ds.env.horizon == T and ds.selected_lengths is None
    assert RecordedEpisodeDataset.file_lengths(path).tolist() == list(LENGTHS)
    ds.refresh_data(4)
    ds.refresh_data(4)      # wraps: episodes 4, 5, 0, 1
    assert ds.selected == [4, 5, 0, 1] and ds.selected_lengths.tolist() == [5, 1, 9, 3] and ds.data["lengths"].tolist() == [5, 1, 9, 3]
    assert len(ds) == T and ds.data["imgs"].shape[:2] == (4, T)
    assert ds.peek_lengths(3).tolist() == [2, 4, 5] and ds.selected == [4, 5, 0, 1]          # peeking selects nothing
    # save(lengths=...) writes the same file; int64 lengths are taken as well
    again = RecordedEpisodeDataset.save(str(tmp_path / "s.npz"), env_name="Lift", **dict(arrays, lengths=arrays["lengths"].astype(np.int64)))
    assert RecordedEpisodeDataset(again, obj_name="cube").lengths.tolist() == list(LENGTHS)


def test_a_dense_file_has_no_lengths(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset, ResidentEpisodeDataset
    eps = _episodes((4, 4, 4))
    path = RecordedEpisodeDataset.save(str(tmp_path / "d.npz"), env_name="Lift", **{k: np.stack([ep[k] for ep in eps]) for k in eps[0]})
    with np.load(path) as f:
        assert "lengths" not in f.files
    assert RecordedEpisodeDataset.file_lengths(path) is None
    for ds in (RecordedEpisodeDataset(path, obj_name="cube"), ResidentEpisodeDataset(path, obj_name="cube", device="cpu")):
        ds.refresh_data(2)
        assert ds.lengths is None and ds.selected_lengths is None and ds.valid(0, 2) is None and ds.peek_lengths(2) is None
    assert "lengths" not in RecordedEpisodeDataset(path).episodes and ds.lengths_dev is None
    s = ds.sampler(2, sequence_length=2)
    assert not s.ragged and (s.windows_per_episode, s.num_windows, s.steps_per_epoch) == (2, 4, 2)


def test_check_refuses_bad_lengths(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset
    eps = _episodes((4, 4, 4))
    arrays = {k: np.stack([ep[k] for ep in eps]) for k in eps[0]}
    save = lambda n: RecordedEpisodeDataset.save(str(tmp_path / "x.npz"), lengths=n, **arrays)
    with pytest.raises(ValueError, match="int32 or int64"):
        save(np.array([4.0, 4.0, 4.0]))
    with pytest.raises(ValueError, match="int32 or int64"):
        save(np.array([4, 4, 4], dtype=np.int16))
    with pytest.raises(ValueError, match=r"\(3,\)"):
        save(np.array([4, 4], dtype=np.int32))
    with pytest.raises(ValueError, match=r"\(3,\)"):
        save(np.array([[4, 4, 4]], dtype=np.int32))
    with pytest.raises(ValueError, match="got 0 for episode 1"):
        save(np.array([4, 0, 4], dtype=np.int32))
    with pytest.raises(ValueError, match="got 5 for episode 2"):
        save(np.array([1, 4, 5], dtype=np.int64))
    with pytest.raises(ValueError, match="got -1 for episode 0"):
        save(np.array([-1, 9, 4], dtype=np.int64))
    save(np.array([1, 4, 2], dtype=np.int32))      # the edges are inside
    # a file written by other means is checked on loading
    bad = str(tmp_path / "bad.npz")
    with open(bad, "wb") as f:
        np.savez(f, lengths=np.array([4, 4, 7]), **arrays)
    with pytest.raises(ValueError, match="got 7 for episode 2"):
        RecordedEpisodeDataset(bad)


def test_pack_refuses_episodes_that_do_not_match(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset
    path = str(tmp_path / "p.npz")
    a, b = _episodes((3, 2))
    for other in (dict(b, depths=np.zeros((2, 8, 8, 1), np.float32)),                      # keys
                  dict(b, true_self=b["true_self"].astype(np.float64)),                      # dtype
                  dict(b, imgs=np.zeros((2, 8, 10, 3), np.uint8)),                           # frame geometry
                  dict(b, true_obj=b["true_obj"][:1])):                                      # its own arrays disagree on T_e
        with pytest.raises(ValueError, match="pack"):
            RecordedEpisodeDataset.pack(path, [a, other])
    with pytest.raises(ValueError, match="pack"):
        RecordedEpisodeDataset.pack(path, [])


def test_valid_mask_on_the_host_path(tmp_path):
    """(device="cpu" holds the pools in host memory: the mask logic runs)"""
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import ResidentEpisodeDataset
    ds = ResidentEpisodeDataset(_packed(tmp_path), obj_name="cube", device="cpu")
    with pytest.raises(ValueError, match="refresh_data"):
        ds.valid(0, 2)
    ds.refresh_data(4)
    ds.refresh_data(4)
    assert ds.lengths_dev.dtype == torch.int32 and ds.lengths_dev.tolist() == list(LENGTHS) and ds.sel[:4].tolist() == [4, 5, 0, 1]
    v = ds.valid(2, 4)
    assert v.dtype == torch.uint8 and tuple(v.shape) == (4, 4)
    assert np.array_equal(v.numpy().astype(bool), ro.valid_mask([5, 1, 9, 3], T)[:, 2:6].T)


# -- the oracle's window table ----------------------------------------------------------------------------------------------------

def _desc(n, shuffle, seed=9, e=len(LENGTHS)):
    return dict(seed=seed, E=e, T=T, S=S, stride=STRIDE, N=n, shuffle=shuffle)


def test_oracle_table_at_the_edges():
    sel = list(range(6))
    ks, prefix, m = ro.window_table(_desc(1, 0), sel, LENGTHS)
    assert ks == [4, 1, 0, 1, 2, 0] and prefix == [0, 4, 5, 5, 6, 8, 8] and m == 8
    assert ro.valid_windows(_desc(1, 0), sel, LENGTHS) == [(0, 0), (0, 2), (0, 4), (0, 6), (1, 0), (3, 0), (4, 0), (4, 2)]
    # through a selection: the lengths are the file's, read at sel[e]
    assert ro.window_table(_desc(1, 0, e=3), [5, 4, 0], LENGTHS)[0] == [0, 2, 4]


@pytest.mark.parametrize("shuffle", [0, 1])
def test_oracle_windows_stay_inside_and_an_epoch_visits_each_once(shuffle):
    sel = [3, 0, 5, 4, 1, 2]      # file order is not selection order
    for n in (1, 2, 3, 8):
        d = _desc(n, shuffle)
        m = ro.window_table(d, sel, LENGTHS)[2]
        for epoch in range(2):
            seen = []
            for step in range(epoch * m, (epoch + 1) * m):      # one draw a step: these m steps are the epoch
                idx = ro.window_index(dict(d, N=1), sel, LENGTHS, step)
                assert idx[0] == step
                seen.append((int(idx[1]), int(idx[2])))
            assert all(t0 + S <= LENGTHS[e] for e, t0 in seen)
            assert sorted(seen) == sorted(ro.valid_windows(d, sel, LENGTHS)), (n, epoch)
        # a batch of N is N consecutive draws
        batch = ro.window_index(d, sel, LENGTHS, 2)
        singles = [ro.window_index(dict(d, N=1), sel, LENGTHS, 2 * n + i)[1:] for i in range(n)]
        assert np.array_equal(batch[1:], np.concatenate(singles))
        assert np.array_equal(ro.window_index_fast(d, sel, LENGTHS, 2), batch)
    if shuffle:      # the order changes with the epoch
        d = _desc(8, 1)
        assert not np.array_equal(ro.window_index(d, sel, LENGTHS, 0)[1:], ro.window_index(d, sel, LENGTHS, 1)[1:])


@pytest.mark.parametrize("shuffle", [0, 1])
def test_oracle_equal_lengths_reproduce_the_dense_oracle(shuffle):
    sel = [3, 0, 1]
    for length in (9, 4):      # the dense sampler knows T only: a file whose episodes all have 4 of 9 steps is the dense T = 4 table
        d = dict(seed=77, E=3, T=length, S=S, stride=STRIDE, N=5, shuffle=shuffle)
        for step in (0, 1, 2, 2 ** 32 - 1):
            want = so.window_index(d, sel, step)
            assert np.array_equal(ro.window_index(dict(d, T=9), sel, [length] * 4, step), want)
            assert np.array_equal(ro.window_index_fast(dict(d, T=9), sel, [length] * 4, step), want)


def test_oracle_without_any_window():
    d = _desc(3, 1, e=2)
    assert ro.window_index(d, [5, 2], LENGTHS, 4).tolist() == [4, 5, 0, 5, 0, 5, 0]
    assert ro.window_index_fast(d, [5, 2], LENGTHS, 4).tolist() == [4, 5, 0, 5, 0, 5, 0]


def test_oracle_statistics():
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    got = ro.error_stats(x, [4, 1, 2])
    flat = np.array([0, 1, 2, 3, 4, 8, 9], dtype=np.float64)
    assert np.allclose(got, [flat.mean(), flat.std(), 9, 6, 4, 17, 1.5, 4, 8.5])
    x[1, 2] = np.nan      # padding
    assert np.array_equal(ro.error_stats(x, [4, 1, 2]), got)


# -- declarations -----------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_and_bound():
    from rgb_proprioceptive_pose_estimator_amd import _lib, ops
    import rgb_proprioceptive_pose_estimator_amd.torch_ops as TO
    header = open(os.path.join(ROOT, "include", "rpe_hip.h")).read()
    for name in ("rpe_sample_windows_ragged", "rpe_pose_loss_masked", "rpe_error_stats_ragged"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS and hasattr(_lib.raw, name), name
    assert _lib.ABI_VERSION == 3      # additive: the version stays
    for name in ("sample_windows_ragged", "pose_loss_masked", "error_stats_ragged"):
        assert name in TO.NAMES and getattr(torch.ops.rpe, name).default._schema.name == "rpe::" + name
    with pytest.raises(NotImplementedError):      # registered for the device only
        torch.ops.rpe.pose_loss_masked(torch.randn(2, 7), torch.randn(2, 7), torch.ones(2, dtype=torch.uint8), 3, 1, 1.0, 0.5, 1e-4)
    assert list(inspect.signature(ops.pose_loss).parameters)[-1] == "valid" and list(inspect.signature(ops.error_stats).parameters) == ["err", "lengths"]
    assert list(inspect.signature(ops.sample_windows_ragged).parameters) == ["desc", "sel", "lengths", "state", "out"]


def test_rejected_arguments_need_no_device():
    """bad arguments come back as a status, or as a ValueError of the wrapper, before anything is launched"""
    import ctypes
    from rgb_proprioceptive_pose_estimator_amd import _lib, ops
    d = ops.sample_desc(seed=1, E=8193, T=4, S=1, stride=1, N=2, shuffle=1)
    one = ctypes.c_void_p(16)      # never dereferenced: the shape checks come first
    assert _lib.raw.rpe_sample_windows_ragged(ctypes.byref(d), one, one, one, one, None) != 0 and b"8192" in _lib.raw.rpe_last_error()
    d.E = 8192
    assert _lib.raw.rpe_sample_windows_ragged(ctypes.byref(d), one, None, one, one, None) != 0 and b"null" in _lib.raw.rpe_last_error()
    d.E, d.T, d.S = 4, 2 ** 30, 1      # E * max K reaches 2^31
    assert _lib.raw.rpe_sample_windows_ragged(ctypes.byref(d), one, one, one, one, None) != 0 and b"2^31" in _lib.raw.rpe_last_error()
    assert _lib.raw.rpe_pose_loss_masked(one, one, one, 0, 0, 0, 1.0, 0.0, 1e-4, one, None, None) != 0
    assert _lib.raw.rpe_pose_loss_masked(one, one, None, 4, 0, 0, 1.0, 0.0, 1e-4, one, None, None) != 0
    assert _lib.raw.rpe_error_stats_ragged(one, 2, 2, None, one, None) != 0 and _lib.raw.rpe_error_stats_ragged(one, 0, 2, one, one, None) != 0
    # the wrappers: wrong dtypes and devices (host tensors here) are ValueErrors
    p, v = torch.zeros(4, 7), torch.ones(4, dtype=torch.uint8)
    for bad in (lambda: ops.pose_loss(p, p, 0, 0, 1.0, 0.0, 1e-4, valid=v.float()), lambda: ops.pose_loss(p, p, 0, 0, 1.0, 0.0, 1e-4, valid=v[:3]),
                lambda: ops.pose_loss(p, p, 0, 0, 1.0, 0.0, 1e-4, valid=v),                   # a host mask
                lambda: ops.error_stats(torch.zeros(2, 3), torch.ones(2, dtype=torch.int64)), lambda: ops.error_stats(torch.zeros(2, 3), torch.ones(3, dtype=torch.int32)),
                lambda: ops.error_stats(torch.zeros(2, 3), torch.ones(2, dtype=torch.int32)),   # host lengths
                lambda: ops.sample_windows_ragged(ops.sample_desc(E=2, T=3), torch.zeros(2, dtype=torch.int32), torch.ones(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)),
                lambda: ops.sample_windows_ragged(ops.sample_desc(E=2, T=3), torch.zeros(2, dtype=torch.int32), torch.ones(2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))):
        with pytest.raises(ValueError):
            bad()


# -- the sampler's host figures -----------------------------------------------------------------------------------------------------

def test_sampler_figures_follow_the_selection(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import ResidentEpisodeDataset, ragged_window_counts
    assert ragged_window_counts(LENGTHS, S, STRIDE) == ([4, 1, 0, 1, 2, 0], 8)
    ds = ResidentEpisodeDataset(_packed(tmp_path), obj_name="cube", device="cpu")
    ds.refresh_data(3)      # episodes 0, 1, 2: lengths 9, 3, 2
    s = ds.sampler(2, sequence_length=S, stride=STRIDE)
    assert s.ragged and (s.windows_per_episode, s.num_windows, s.steps_per_epoch) == ([4, 1, 0], 5, 2)
    assert s.desc_fields() == dict(seed=0, E=3, T=T, S=S, stride=STRIDE, N=2, shuffle=1)
    ds.refresh_data(3)      # episodes 3, 4, 5: lengths 4, 5, 1
    assert (s.windows_per_episode, s.num_windows, s.steps_per_epoch) == ([1, 2, 0], 3, 1)
    ds.refresh_data(3)
    assert s.num_windows == 5
    # fewer windows than a batch: at construction, and at the call that follows a refresh that makes it so
    with pytest.raises(ValueError, match="at least as many windows"):
        ds.sampler(6, sequence_length=S, stride=STRIDE)
    s4 = ds.sampler(4, sequence_length=S, stride=STRIDE)
    ds.refresh_data(3)      # 3 windows
    with pytest.raises(ValueError, match="at least as many windows"):
        s4()
    # an episode shorter than a window is never drawn: with S = 6 only episode 0 holds windows
    ds.refresh_data(6)
    assert ds.sampler(2, sequence_length=6, stride=1).windows_per_episode == [4, 0, 0, 0, 0, 0]
    with pytest.raises(ValueError, match="does not fit"):
        ds.sampler(1, sequence_length=T + 1)


# -- write_video --------------------------------------------------------------------------------------------------------------------

def test_write_video_drops_the_padding(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import write_video
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (3, 4, 6, 5, 3), dtype=np.uint8)
    lengths = np.array([4, 1, 2])
    path = write_video(torch.from_numpy(frames), str(tmp_path / "v.npy"), lengths=lengths)
    got = np.load(path)
    assert got.shape == (7, 6, 5, 3) and np.array_equal(got, np.concatenate([frames[0, :4], frames[1, :1], frames[2, :2]]))
    assert np.load(write_video(frames, str(tmp_path / "w.npy"))).shape == (12, 6, 5, 3)      # without lengths: as before
    from PIL import Image
    gif = Image.open(write_video(frames, str(tmp_path / "v.gif"), fps=5, lengths=torch.tensor([4, 1, 2])))
    assert gif.n_frames == 7
    for bad in (np.array([4, 1]), np.array([4, 1, 5]), np.array([4.0, 1.0, 2.0]), np.array([0, 0, 0])):
        with pytest.raises(ValueError, match="lengths"):
            write_video(frames, str(tmp_path / "x.npy"), lengths=bad)
    with pytest.raises(ValueError, match="lengths"):
        write_video(frames.reshape(12, 6, 5, 3), str(tmp_path / "x.npy"), lengths=lengths)


# -- refusals before any device use -------------------------------------------------------------------------------------------------

def test_train_refusals_need_no_device(tmp_path, monkeypatch):
    from rgb_proprioceptive_pose_estimator_amd.util import learn_utils as lu
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset, ResidentEpisodeDataset
    path = _packed(tmp_path)

    class Untouchable:      # the model: reading its shape is fine, moving it to a device is not
        requires_sequence, sequence_length, use_depth = True, S, False

        def __getattr__(self, name):
            raise AssertionError("train() touched the model (%s) before refusing" % name)

    sig = inspect.signature(lu.train_step)
    assert list(sig.parameters)[-1] == "valid" and sig.parameters["valid"].default is None
    # the lockstep walk of a ragged file
    for ds in (RecordedEpisodeDataset(path, obj_name="cube"), ResidentEpisodeDataset(path, obj_name="cube", device="cpu")):
        with pytest.raises(ValueError, match=r"batch_size.*--resident --batch_size"):
            lu.train(Untouchable(), ds, {}, None, 1, 3, 1, {}, "cuda:0")
    # a process group
    ds = ResidentEpisodeDataset(path, obj_name="cube", device="cpu")
    monkeypatch.setattr(lu.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(lu.dist, "get_world_size", lambda: 2)
    with pytest.raises(ValueError, match="process group"):
        lu.train(Untouchable(), ds, {}, None, 1, 3, 1, {}, "cuda:0", batch_size=2)
    monkeypatch.undo()
    # fewer windows than the batch in the first train selection: episodes 0, 1, 2 hold 4 + 1 + 0
    with pytest.raises(ValueError, match="hold 5"):
        lu.train(Untouchable(), ds, {}, None, 1, 3, 1, {}, "cuda:0", batch_size=6, window_stride=STRIDE)
    assert ds.selected == [] and ds.num_selected == 0      # nothing was selected on the way


def test_script_refusals_need_no_device(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.scripts import rollout, train_model
    path = _packed(tmp_path)
    common = ["--model", "no", "--obj_name", "cube", "--episodes", path]
    for flags in ([], ["--resident"]):
        with pytest.raises(SystemExit, match=r"--resident --batch_size"):
            train_model.main(common + flags)
    for flags in ([], ["--no_graph"], ["--video_out", str(tmp_path / "v.npy"), "--camera_matrix", _camera(tmp_path), "--model_outputs_file", "o.npy"]):
        with pytest.raises(SystemExit, match="--batched"):
            rollout.main(common + flags)
    # a dense file passes both checks (and stops at the next one when there is no device)
    eps = _episodes((4, 4))
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset
    dense = RecordedEpisodeDataset.save(str(tmp_path / "d.npz"), env_name="Lift", **{k: np.stack([ep[k] for ep in eps]) for k in eps[0]})
    args = train_model.build_parser().parse_args(["--episodes", dense])
    assert train_model.check_ragged(args, {}) is None
    assert train_model.check_ragged(train_model.build_parser().parse_args(["--episodes", path, "--resident", "--batch_size", "2"]), {"batch_size": 2}) is None


def _camera(tmp_path):
    cam = str(tmp_path / "camera.npy")
    np.save(cam, np.array([[30.0, 0, 8, 12], [0, 26.0, 6, 9], [0, 0, 1.0, 1.5]]))
    return cam


def test_evaluation_result_carries_the_lengths():
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import EpisodeEvaluation
    stats = np.zeros((1, 2, 3 + 2 * 2))
    assert EpisodeEvaluation(None, None, None, None, stats).lengths is None
    ev = EpisodeEvaluation(None, None, None, None, stats, lengths=[3, 1])
    assert isinstance(ev.lengths, np.ndarray) and ev.lengths.tolist() == [3, 1] and "EVALUATION COMPLETED" in ev.summary()
    for a, b in zip(ev.summary().splitlines(), EpisodeEvaluation(None, None, None, None, stats).summary().splitlines()):
        assert a == b      # the same lines, from whatever figures the table holds
