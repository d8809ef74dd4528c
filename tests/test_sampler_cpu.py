"""CPU side of the minibatch sampler: the numpy oracle (tests/_sampler_oracle.py) against the specification's properties -- the kernels
are compared with it for equality in tests/test_gpu_sampler.py, so the permutation is checked here, once -- and the host logic of
ResidentEpisodeDataset, WindowSampler, train(), GraphedTrainStep and scripts/train_model.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _sampler_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M_VALUES = (1, 2, 3, 4, 5, 7, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 4097, 70000)
SEEDS = (0, 0x123456789ABCDEF, 2 ** 64 - 1)


@pytest.mark.parametrize("m", M_VALUES)
def test_permutation_is_a_bijection_and_epochs_differ(m):
    pos = np.arange(m)
    for seed in SEEDS:
        orders = []
        for epoch in (0, 1, 2 ** 32 + 5):
            walks = []
            w = so.permute(pos, m, epoch, seed, walks)
            assert np.array_equal(np.sort(w), pos.astype(np.uint64)), (m, seed, epoch)
            assert walks == [] or walks[0] <= 4 ** so.half_bits(m)      # a cycle of the 2h-bit domain is no longer than the domain
            orders.append(w)
        if m >= 16:   # (2 orders of a handful of windows may coincide; from 16 windows on a coincidence would be a defect)
            assert not np.array_equal(orders[0], orders[1]) and not np.array_equal(orders[1], orders[2])
            assert not np.array_equal(orders[0], pos)
    if m >= 16:
        assert not np.array_equal(so.permute(pos, m, 0, SEEDS[0]), so.permute(pos, m, 0, SEEDS[1]))
    # the epoch enters modulo 2^32
    assert np.array_equal(so.permute(pos, m, 5, 1), so.permute(pos, m, 2 ** 32 + 5, 1))


def test_half_bits():
    assert [so.half_bits(m) for m in (1, 2, 3, 4, 5, 16, 17, 256, 257, 70000, 2 ** 31 - 1)] == [1, 1, 1, 1, 2, 2, 3, 4, 5, 9, 16]


def test_window_arithmetic():
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import window_counts
    # (E, T, S, stride) -> (K, M); the tail (T - S) % stride != 0 is not a window
    for args, want in (((3, 7, 1, 1), (7, 21)), ((3, 7, 3, 3), (2, 6)), ((3, 7, 3, 1), (5, 15)), ((3, 7, 7, 1), (1, 3)), ((2, 10, 4, 4), (2, 4)),
                       ((2, 10, 4, 5), (2, 4)), ((2, 10, 4, 7), (1, 2)), ((5, 100, 10, 10), (10, 50)), ((1, 1, 1, 1), (1, 1))):
        assert window_counts(*args) == want, args
        assert so.window_counts(dict(E=args[0], T=args[1], S=args[2], stride=args[3])) == want
    for bad in ((3, 7, 8, 1), (3, 7, 0, 1), (3, 7, 1, 0), (0, 7, 1, 1)):
        with pytest.raises(ValueError):
            window_counts(*bad)


def test_oracle_index_layout_and_coverage():
    sel = [3, 0, 1]
    d = dict(seed=9, E=3, T=7, S=3, stride=2, N=3, shuffle=0)      # K = 3, M = 9
    idx = so.window_index(d, sel, 1)                                 # draws 3, 4, 5 -> windows 3, 4, 5 = episode 1 of sel
    assert idx.dtype == np.int32 and idx.tolist() == [1, 0, 0, 0, 2, 0, 4]
    idx = so.window_index(d, sel, 3)                                 # epoch 1 starts: windows 0, 1, 2
    assert idx.tolist() == [3, 3, 0, 3, 2, 3, 4]
    d["shuffle"] = 1
    seen = np.concatenate([so.window_index(d, sel, s)[1:].reshape(-1, 2) for s in range(3)])
    want = sorted((e, t) for e in sel for t in (0, 2, 4))
    assert sorted(map(tuple, seen.tolist())) == want                 # M draws from a multiple of M: every window once
    assert so.window_index(dict(d, E=1, T=1, S=1, stride=1, N=2), [2], 7).tolist() == [7, 2, 0, 2, 0]      # M = 1
    pool = np.arange(4 * 7 * 2).reshape(4, 7, 2)
    got = so.gather(pool, so.window_index(d, sel, 0), 3)
    assert got.shape == (3, 3, 2)
    idx = so.window_index(d, sel, 0)
    assert np.array_equal(got[2, 1], pool[idx[3], idx[4] + 2])


# -- the C ABI ------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_and_bound():
    from rgb_proprioceptive_pose_estimator_amd import _lib
    import rgb_proprioceptive_pose_estimator_amd.torch_ops as T
    header = open(os.path.join(ROOT, "include", "rpe_hip.h")).read()
    for name in ("rpe_sample_windows", "rpe_gather_rows"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS and hasattr(_lib.raw, name)
    names = [n for n, _ in _lib.SampleDesc._fields_]
    body = header[header.rindex("typedef struct {", 0, header.index("} rpe_sample_desc;")):header.index("} rpe_sample_desc;")]
    assert [n for n in re.findall(r"\b([A-Za-z_]+)(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))] == names
    assert ctypes.sizeof(_lib.SampleDesc) == 32 and _lib.SampleDesc.E.offset == 8 and _lib.SampleDesc.shuffle.offset == 28
    assert "sample_windows" in T.NAMES and "gather_rows" in T.NAMES
    s = torch.ops.rpe.sample_windows.default._schema
    assert s.name == "rpe::sample_windows" and [a.name for a in s.arguments] == ["desc", "sel", "state"]
    assert [a.name for a in s.arguments if a.alias_info is not None and a.alias_info.is_write] == ["state"]
    g = torch.ops.rpe.gather_rows.default._schema
    assert g.name == "rpe::gather_rows" and [a.name for a in g.arguments] == ["pool", "index", "S", "T"]
    with pytest.raises(NotImplementedError):     # the HIP key only: no CPU kernel to fall back to
        torch.ops.rpe.gather_rows(torch.zeros(2, 3, 4), torch.zeros(3, dtype=torch.int32), 1, 3)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        pool = torch.empty(4, 7, 8, 8, 3, dtype=torch.uint8, device="cuda")
        idx = torch.ops.rpe.sample_windows([0, 3, 7, 2, 1, 5, 1], torch.empty(3, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"))
        assert idx.shape == (11,) and idx.dtype == torch.int32
        out = torch.ops.rpe.gather_rows(pool, idx, 2, 7)
        assert out.shape == (2, 5, 8, 8, 3) and out.dtype == torch.uint8


def test_rejected_arguments_need_no_device():
    """bad arguments come back as a status before anything is launched"""
    from rgb_proprioceptive_pose_estimator_amd import ops
    from rgb_proprioceptive_pose_estimator_amd._lib import raw
    one = ctypes.c_void_p(16)   # never dereferenced: every call below is refused
    good = dict(seed=1, E=3, T=7, S=3, stride=1, N=4, shuffle=1)
    sample = lambda d, sel=one, state=one, index=one: raw.rpe_sample_windows(ctypes.byref(d) if d is not None else None, sel, state, index, None)
    for kw in (dict(E=0), dict(T=0), dict(S=0), dict(stride=0), dict(N=0), dict(E=-1), dict(N=-5), dict(S=8), dict(shuffle=2),
               dict(E=2 ** 31 - 1, T=2 ** 20, S=1)):
        assert sample(ops.sample_desc(**dict(good, **kw))) == 1, kw      # RPE_ERR_SHAPE
    assert b"sample_windows" in raw.rpe_last_error()
    d = ops.sample_desc(**good)
    assert sample(None) == 1 and sample(d, sel=None) == 1 and sample(d, state=None) == 1 and sample(d, index=None) == 1
    gather = lambda pool=one, out=one, row_bytes=192, t=7, index=one, s=3, n=4: raw.rpe_gather_rows(pool, out, row_bytes, t, index, s, n, None)
    assert gather(pool=None) == 1 and gather(out=None) == 1 and gather(index=None) == 1
    assert gather(row_bytes=0) == 1 and gather(row_bytes=-16) == 1 and gather(t=0) == 1 and gather(s=0) == 1 and gather(n=0) == 1 and gather(s=8) == 1
    assert b"gather_rows" in raw.rpe_last_error()


# -- host logic -------------------------------------------------------------------------------------------------------------------

def _episode_file(tmp_path, e=4, t=7, hw=8, two_arm=False):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset
    rng = np.random.default_rng(0)
    def poses():
        q = rng.normal(size=(e, t, 4))
        return np.concatenate([rng.random((e, t, 3)), q / np.linalg.norm(q, axis=-1, keepdims=True)], -1).astype(np.float32)
    return RecordedEpisodeDataset.save(str(tmp_path / "episodes.npz"), env_name="TwoArmLift" if two_arm else "Lift",
                                       imgs=rng.integers(0, 256, (e, t, hw, hw, 3), dtype=np.uint8), true_self=poses(), true_obj=poses(),
                                       true_other=poses() if two_arm else None)


def test_resident_dataset_refresh_matches_the_parent_on_the_host(tmp_path):
    """(device="cpu" holds the pools in host memory: the refresh logic runs; the gathers have no CPU path)"""
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset, ResidentEpisodeDataset
    path = _episode_file(tmp_path)
    a, b = RecordedEpisodeDataset(path, obj_name="cube", seed=5), ResidentEpisodeDataset(path, obj_name="cube", seed=5, device="cpu")
    assert isinstance(b, RecordedEpisodeDataset) and b.frame_dtype == torch.uint8 and b.env.horizon == 7
    with pytest.raises(ValueError, match="refresh_data"):
        b.sampler(2)
    with pytest.raises(ValueError, match="refresh_data"):
        b.chunk(0, 1)
    for n in (3, 3):      # the second selection wraps: [3, 0, 1]
        a.refresh_data(n, None, 0.01)
        b.refresh_data(n, None, 0.01)
        assert a.selected == b.selected and b.num_selected == n and b.sel[:n].tolist() == a.selected and len(b) == len(a) == 7
        assert torch.equal(b.pool["measurement_self"][b.sel[:n].long()], a.data["measurement_self"])
    assert b.selected == [3, 0, 1] and tuple(b.pool["measurement_self"].shape) == (4, 7, 7)
    with pytest.raises(ValueError):
        b.refresh_data(5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        b.chunk(0, 2)


def test_sampler_validation_and_state_dict(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import ResidentEpisodeDataset, WindowSampler
    ds = ResidentEpisodeDataset(_episode_file(tmp_path), device="cpu")
    ds.refresh_data(3)
    s = ds.sampler(4, sequence_length=3)
    assert isinstance(s, WindowSampler) and (s.stride, s.windows_per_episode, s.num_windows, s.steps_per_epoch, s.shuffle) == (3, 2, 6, 1, True)
    assert ds.sampler(4, sequence_length=3, stride=1).steps_per_epoch == 15 // 4 and ds.sampler(5).steps_per_epoch == 21 // 5
    assert s.desc_fields() == dict(seed=0, E=3, T=7, S=3, stride=3, N=4, shuffle=1) and tuple(s.index.shape) == (9,) and s.index.dtype == torch.int32
    for kw in (dict(batch_size=7, sequence_length=3), dict(batch_size=2, sequence_length=8), dict(batch_size=2, stride=0), dict(batch_size=2, seed=2 ** 64),
               dict(batch_size=2, seed=-1), dict(batch_size=0)):
        with pytest.raises(ValueError):
            ds.sampler(**kw)
    assert s.step == 0 and s.state_dict() == {"seed": 0, "step": 0}
    s.load_state_dict({"seed": 2 ** 64 - 1, "step": 2 ** 32 - 1})
    assert s.state_dict() == {"seed": 2 ** 64 - 1, "step": 2 ** 32 - 1} and s.desc_fields()["seed"] == 2 ** 64 - 1
    for bad in ({"seed": -1, "step": 0}, {"seed": 0, "step": 2 ** 32}):
        with pytest.raises(ValueError):
            s.load_state_dict(bad)
    ds.refresh_data(2)      # another number of episodes than the sampler was made for
    with pytest.raises(ValueError, match="selected"):
        s()


def test_smallest_shard_step_count():
    from rgb_proprioceptive_pose_estimator_amd.dist import shard_bounds
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import sampled_steps_per_epoch
    # one process: M // N
    assert sampled_steps_per_epoch(3, 1, 7, 1, 1, 5) == 21 // 5 and sampled_steps_per_epoch(3, 1, 7, 3, 3, 2) == 3
    # 10 episodes over 4 ranks: shards of 3, 3, 2, 2 -> the 2-episode shards set the count for everyone
    sizes = [hi - lo for lo, hi in (shard_bounds(10, r, 4) for r in range(4))]
    assert sorted(sizes) == [2, 2, 3, 3]
    assert sampled_steps_per_epoch(10, 4, 20, 4, 4, 3) == (2 * 5) // 3 == 3
    assert sampled_steps_per_epoch(10, 4, 20, 4, 1, 8) == (2 * 17) // 8 == 4
    # 7 episodes over 2 ranks: 4 and 3
    assert sampled_steps_per_epoch(7, 2, 9, 2, 2, 4) == (3 * 4) // 4 == 3
    # an even split changes nothing
    assert sampled_steps_per_epoch(8, 2, 9, 2, 2, 4) == (4 * 4) // 4
    with pytest.raises(ValueError):       # a rank without episodes cannot sample
        sampled_steps_per_epoch(3, 4, 9, 2, 2, 1)


def test_train_and_graphed_step_signatures_and_refusals(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset, SyntheticEpisodeDataset
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import GraphedTrainStep, train
    sig = inspect.signature(train).parameters
    for name, default in (("batch_size", None), ("window_stride", None), ("shuffle_seed", 0)):
        assert sig[name].default == default and sig[name].kind == inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(GraphedTrainStep.__init__).parameters["sampler"].default is None
    assert inspect.signature(GraphedTrainStep.__call__).parameters["batch"].default is None
    with pytest.raises(ValueError, match="sampler"):
        train(None, SyntheticEpisodeDataset(horizon=2, device="cpu"), {}, None, 1, 1, 1, {}, "cuda:0", batch_size=4)
    with pytest.raises(ValueError, match="sampler"):
        train(None, RecordedEpisodeDataset(_episode_file(tmp_path)), {}, None, 1, 1, 1, {}, "cuda:0", batch_size=4)
    with pytest.raises(ValueError, match="batch_size"):
        train(None, SyntheticEpisodeDataset(horizon=2, device="cpu"), {}, None, 1, 1, 1, {}, "cuda:0", window_stride=2)


def test_script_flags():
    from rgb_proprioceptive_pose_estimator_amd.scripts.train_model import build_parser, build_sampling
    p = build_parser()
    args = p.parse_args([])
    assert args.resident is False and args.batch_size is None and args.window_stride is None and args.shuffle_seed is None
    assert build_sampling(args) == {}
    assert build_sampling(p.parse_args(["--episodes", "x.npz", "--resident"])) == {}
    got = build_sampling(p.parse_args(["--episodes", "x.npz", "--resident", "--batch_size", "256", "--window_stride", "1", "--shuffle_seed", "7"]))
    assert got == dict(batch_size=256, window_stride=1, shuffle_seed=7)
    assert build_sampling(p.parse_args(["--episodes", "x.npz", "--resident", "--batch_size", "8"])) == dict(batch_size=8, window_stride=None, shuffle_seed=0)
    with pytest.raises(SystemExit, match="--episodes"):
        build_sampling(p.parse_args(["--resident"]))
    for flags in (["--batch_size", "8"], ["--episodes", "x.npz", "--batch_size", "8"], ["--resident", "--batch_size", "8"],
                  ["--episodes", "x.npz", "--window_stride", "2"], ["--shuffle_seed", "1"]):
        with pytest.raises(SystemExit, match="--resident"):
            build_sampling(p.parse_args(flags))
    for flags in (["--window_stride", "2"], ["--shuffle_seed", "3"]):
        with pytest.raises(SystemExit, match="--batch_size"):
            build_sampling(p.parse_args(["--episodes", "x.npz", "--resident"] + flags))
    for flags in (["--batch_size", "0"], ["--batch_size", "4", "--window_stride", "0"], ["--batch_size", "4", "--shuffle_seed", "-1"]):
        with pytest.raises(SystemExit):
            build_sampling(p.parse_args(["--episodes", "x.npz", "--resident"] + flags))
