"""GPU side of the minibatch sampler: rpe_sample_windows and rpe_gather_rows against the numpy oracle (tests/_sampler_oracle.py) for
equality -- the arithmetic is all integer and the gather is a copy, so there is no tolerance anywhere -- and the sampler through
ResidentEpisodeDataset, a captured graph, train() and GraphedTrainStep."""
import numpy as np
import pytest
import torch

import _sampler_oracle as so

pytestmark = pytest.mark.gpu

E_FILE, T = 4, 7
SEL = [3, 0, 1]            # a wrapped selection
# (S, stride, N): K = 7, 2, 5, 1, 1 start positions -> M = 21, 6, 15, 3, 3 windows; the last draws more than an epoch per step
SHAPES = [(1, 1, 5), (3, 3, 2), (3, 1, 4), (7, 1, 3), (7, 1, 5)]


def _ops():
    from rgb_proprioceptive_pose_estimator_amd import ops
    return ops


def _desc(s, stride, n, shuffle, seed):
    return dict(seed=seed, E=len(SEL), T=T, S=s, stride=stride, N=n, shuffle=shuffle)


@pytest.mark.parametrize("seed", [0, 2 ** 64 - 1], ids=["seed0", "seedmax"])
@pytest.mark.parametrize("shuffle", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=["S%d_k%d_N%d" % s for s in SHAPES])
def test_index_equals_the_oracle(shape, shuffle, seed):
    ops = _ops()
    d = _desc(*shape, shuffle, seed)
    m, n = so.window_counts(d)[1], d["N"]
    sel = torch.tensor(SEL, dtype=torch.int32, device="cuda")
    # steps 0 and 1, the step whose draws reach the end of epoch 0 (they cross into epoch 1 where N does not divide M), and the last
    # value of the 32-bit counter (g needs 64 bits; the counter wraps to 0)
    for step in (0, 1, m // n, 2 ** 32 - 1):
        state = torch.tensor([step - 2 ** 32 if step >= 2 ** 31 else step], dtype=torch.int32, device="cuda")
        idx = ops.sample_windows(ops.sample_desc(**d), sel, state)
        want = so.window_index(d, SEL, step)
        assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), want), (step, idx.tolist(), want.tolist())
        assert int(state.item()) & 0xFFFFFFFF == (step + 1) & 0xFFFFFFFF
    if m % n:
        g0 = (m // n) * n
        assert g0 < m < g0 + n      # that step did straddle the epoch boundary


def test_an_epoch_visits_every_window_once():
    ops = _ops()
    sel = torch.tensor(SEL, dtype=torch.int32, device="cuda")
    for s, stride, n in ((1, 1, 7), (3, 1, 5), (3, 3, 2)):
        d = _desc(s, stride, n, 1, 77)
        k, m = so.window_counts(d)
        assert m % n == 0
        state = torch.zeros(1, dtype=torch.int32, device="cuda")
        for epoch in range(2):
            seen = torch.cat([ops.sample_windows(ops.sample_desc(**d), sel, state)[1:].reshape(n, 2) for _ in range(m // n)]).cpu().tolist()
            assert sorted(map(tuple, seen)) == sorted((e, j * stride) for e in SEL for j in range(k)), (s, stride, n, epoch)
        assert state.item() == 2 * (m // n)


def test_torch_op_equals_the_wrapper():
    ops = _ops()
    import rgb_proprioceptive_pose_estimator_amd.torch_ops  # noqa: F401  (registers torch.ops.rpe.*)
    d = _desc(3, 1, 4, 1, 5)
    sel = torch.tensor(SEL, dtype=torch.int32, device="cuda")
    state = torch.tensor([2], dtype=torch.int32, device="cuda")
    idx = torch.ops.rpe.sample_windows([d[k] for k in ops.SAMPLE_DESC_FIELDS], sel, state)
    assert np.array_equal(idx.cpu().numpy(), so.window_index(d, SEL, 2)) and state.item() == 3
    pool = torch.arange(E_FILE * T * 7, dtype=torch.float32, device="cuda").reshape(E_FILE, T, 7)
    assert torch.equal(torch.ops.rpe.gather_rows(pool, idx, 3, T), ops.gather_rows(pool, idx, 3, T))


# -- the gather -----------------------------------------------------------------------------------------------------------------

_POOLS = {}


def _pool(tail, dtype, offset=0):
    """a seeded pool (E_FILE, T) + tail on the device, every byte random (a wrong row or a torn tail shows), and its host copy.  offset:
    the pool is a view that starts `offset` bytes into its allocation."""
    key = (tail, dtype, offset)
    if key not in _POOLS:
        rng = np.random.default_rng(len(_POOLS) + 1)
        shape = (E_FILE, T) + tail
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        raw = rng.integers(0, 256, offset + nbytes, dtype=np.uint8)
        if dtype == np.float32:      # no NaN patterns: equality is checked on values as well as bits
            raw[offset + 3::4] &= 0x3F
        host = raw[offset:].view(dtype).reshape(shape)
        dev = torch.from_numpy(raw).cuda()[offset:].view(torch.uint8 if dtype == np.uint8 else torch.float32).reshape(shape)
        assert dev.is_contiguous() and dev.data_ptr() % 16 == offset % 16
        _POOLS[key] = (host, dev)
    return _POOLS[key]


def _hand_index(n, s, seed):
    rng = np.random.default_rng(seed)
    idx = np.zeros(1 + 2 * n, dtype=np.int32)
    idx[0] = 12345
    idx[1::2] = rng.integers(0, E_FILE, n)
    idx[2::2] = rng.integers(0, T - s + 1, n)
    return idx


GATHERS = [
    # tail shape, dtype, byte offset of the pool view            row bytes -> path
    ((8, 8, 3), np.uint8, 0),        # 192: 16-byte units
    ((10, 6, 3), np.uint8, 0),       # 180: 4-byte units
    ((5, 3, 3), np.uint8, 0),        # 45: single bytes
    ((8, 8, 1), np.float32, 0),      # 256: 16-byte units
    ((10, 6, 1), np.float32, 0),     # 240: 16-byte units
    ((5, 3, 1), np.float32, 0),      # 60: 4-byte units
    ((7,), np.float32, 0),           # 28: the pose rows, 4-byte units
    ((8, 8, 3), np.uint8, 4),        # 192 bytes behind a pointer that is 4 mod 16: the 16-byte path must be refused
    ((8, 8, 3), np.uint8, 1),        # and behind an odd pointer: single bytes
    ((76, 76, 3), np.uint8, 0),      # 17,328 = 16 x 1,083: one whole tile of 1,024 units and a tail tile per row
    ((76, 76, 3), np.uint8, 4),      # 4,332 dwords: four whole tiles and a tail
    ((76, 76, 3), np.uint8, 1),      # 17,328 bytes: sixteen whole tiles and a tail
]


@pytest.mark.parametrize("tail,dtype,offset", GATHERS, ids=["%s_%s_off%d" % ("x".join(map(str, g[0])), np.dtype(g[1]).name, g[2]) for g in GATHERS])
def test_gather_equals_the_oracle(tail, dtype, offset):
    ops = _ops()
    host, dev = _pool(tail, dtype, offset)
    for s, n in ((1, 5), (3, 4), (7, 2)):
        idx = _hand_index(n, s, seed=s * 100 + n)
        got = ops.gather_rows(dev, torch.from_numpy(idx).cuda(), s, T)
        assert tuple(got.shape) == (s, n) + tail and got.dtype == dev.dtype
        assert np.array_equal(got.cpu().numpy(), so.gather(host, idx, s)), (s, n)
    # `out=`: written in place, and the bytes behind it stay
    idx = _hand_index(3, 2, seed=9)
    buf = torch.full((2 * 3 * int(np.prod(tail)) + 8,), 7, dtype=dev.dtype, device="cuda")
    out = buf[:-8].view((2, 3) + tail)
    assert ops.gather_rows(dev, torch.from_numpy(idx).cuda(), 2, T, out=out) is out
    assert np.array_equal(out.cpu().numpy(), so.gather(host, idx, 2)) and (buf[-8:] == 7).all()


def test_gather_walks_more_tiles_than_blocks():
    """490 rows of 17 byte tiles = 8,330 tiles, past the 8,192 blocks of one launch: the grid-stride walk"""
    ops = _ops()
    host, dev = _pool((76, 76, 3), np.uint8, 1)
    idx = _hand_index(70, 7, seed=3)
    got = ops.gather_rows(dev, torch.from_numpy(idx).cuda(), 7, T)
    assert np.array_equal(got.cpu().numpy(), so.gather(host, idx, 7))


def test_gather_arguments():
    ops = _ops()
    _, dev = _pool((7,), np.float32, 0)
    idx = torch.from_numpy(_hand_index(2, 1, 0)).cuda()
    for bad in (lambda: ops.gather_rows(dev, idx, 8, T), lambda: ops.gather_rows(dev, idx, 0, T), lambda: ops.gather_rows(dev, idx, 1, T + 1),
                lambda: ops.gather_rows(dev, idx.long(), 1, T), lambda: ops.gather_rows(dev, idx[:4], 1, T), lambda: ops.gather_rows(dev.transpose(0, 1), idx, 1, E_FILE),
                lambda: ops.gather_rows(dev, idx, 1, T, out=torch.empty(1, 2, 8, device="cuda")), lambda: ops.gather_rows(dev, idx, 1, T, out=torch.empty(1, 2, 7))):
        with pytest.raises(ValueError):
            bad()


# -- the resident dataset -------------------------------------------------------------------------------------------------------

def _episode_file(tmp_path, e=4, t=7, hw=16, name="episodes.npz"):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset
    rng = np.random.default_rng(0)
    def poses():
        q = rng.normal(size=(e, t, 4))
        return np.concatenate([rng.random((e, t, 3)), q / np.linalg.norm(q, axis=-1, keepdims=True)], -1).astype(np.float32)
    return RecordedEpisodeDataset.save(str(tmp_path / name), env_name="Lift", imgs=rng.integers(0, 256, (e, t, hw, hw, 3), dtype=np.uint8),
                                       depths=(0.5 + 2.0 * rng.random((e, t, hw, hw, 1))).astype(np.float32), true_self=poses(), true_obj=poses())


def _datasets(tmp_path, **kw):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset, ResidentEpisodeDataset
    path = _episode_file(tmp_path, **kw)
    return RecordedEpisodeDataset(path, use_depth=True, obj_name="cube", seed=5), ResidentEpisodeDataset(path, use_depth=True, obj_name="cube", seed=5)


def test_chunks_equal_the_host_dataset(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import _chunks, _host_chunks
    host, res = _datasets(tmp_path)
    for _ in range(2):     # the second selection wraps: [3, 0, 1]
        host.refresh_data(3, None, 0.01)
        res.refresh_data(3, None, 0.01)
    assert res.selected == host.selected == [3, 0, 1] and res.sel[:3].tolist() == [3, 0, 1] and len(res) == len(host) == 7
    assert torch.equal(res.pool["measurement_self"][res.sel[:3].long()].cpu(), host.data["measurement_self"])
    want = list(_host_chunks(host, 7, 3, True))
    got = list(_chunks(res, 7, 3, True))                   # (train() and evaluate_episodes walk the dataset through this)
    assert [w[0].shape[0] for w in want] == [3, 3, 1] and len(got) == 3      # t0 = 0, 3 and the short tail chunk at 6
    for (t0, length), w, g in zip(((0, 3), (3, 3), (6, 1)), want, got):
        direct = res.chunk(t0, length)
        for j in (0, 1, 2, 3, 5):                         # img, depth, x0bar, x0, obj (there is no second arm: x1 is None)
            assert g[j].is_cuda and g[j].dtype == w[j].dtype and torch.equal(g[j].cpu(), w[j]) and torch.equal(direct[j], g[j]), (t0, j)
        assert g[4] is None
    item, ref = res[6], host[6]
    for j in (0, 1, 2, 3, 5):
        assert item[j].is_cuda and torch.equal(item[j].cpu(), ref[j])
    with pytest.raises(ValueError):
        res.chunk(6, 2)


# -- the sampler ----------------------------------------------------------------------------------------------------------------

def _check_batch(batch, res, index, s):
    """a sampler batch equals the oracle's gather of the dataset's pools"""
    keys = ("imgs", "depths", "measurement_self", "true_self", None, "true_obj")
    for got, k in zip(batch, keys):
        if k is None:
            assert got is None
        else:
            assert np.array_equal(got.cpu().numpy(), so.gather(res.pool[k].cpu().numpy(), index, s)), k


def test_captured_sampler_draws_the_next_batch_at_every_replay(tmp_path):
    _, res = _datasets(tmp_path)
    res.refresh_data(3, None, 0.01)
    sampler = res.sampler(4, sequence_length=3, stride=1, shuffle=True, seed=11)
    assert sampler.steps_per_epoch == 15 // 4
    d = sampler.desc_fields()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = sampler()                                  # step 0: the buffers exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert np.array_equal(sampler.index.cpu().numpy(), so.window_index(d, res.selected, 0))
    _check_batch(first, res, sampler.index.cpu().numpy(), 3)
    ptrs = [None if t is None else t.data_ptr() for t in first]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        batch = sampler()
    assert sampler.step == 1 and [None if t is None else t.data_ptr() for t in batch] == ptrs      # the capture itself ran nothing
    for step in (1, 2, 3):
        g.replay()
        want = so.window_index(d, res.selected, step)
        assert np.array_equal(sampler.index.cpu().numpy(), want) and sampler.step == step + 1
        _check_batch(batch, res, want, 3)
    # resuming: a new sampler from the state dict draws the same next batch
    sd = sampler.state_dict()
    assert sd == {"seed": 11, "step": 4}
    g.replay()
    again = res.sampler(4, sequence_length=3, stride=1, shuffle=True, seed=0)
    again.load_state_dict(sd)
    other = again()
    assert torch.equal(again.index, sampler.index) and again.index[0].item() == 4
    for a, b in zip(other, batch):
        assert (a is None and b is None) or torch.equal(a, b)
    # a refresh between replays: the next replay reads the new selection and the new measurements
    old_meas = res.pool["measurement_self"].clone()
    res.refresh_data(3, None, 0.01)
    assert res.selected == [3, 0, 1] and not torch.equal(res.pool["measurement_self"], old_meas)
    g.replay()
    want = so.window_index(d, [3, 0, 1], 5)
    assert np.array_equal(sampler.index.cpu().numpy(), want) and not np.array_equal(want, so.window_index(d, [0, 1, 2], 5))
    _check_batch(batch, res, want, 3)


# -- the input pipeline -----------------------------------------------------------------------------------------------------------

def test_the_four_stages_together_equal_their_oracles(tmp_path):
    """TrainInputs, eager (nothing is captured): sampler, measurement noise, frame and depth augmentation in one call, each against its
    own numpy oracle at steps 0, 1, 2.  A namespace stands in for the model: no trunk runs."""
    import types
    import _augment_oracle as ao
    import _depth_augment_oracle as do
    import _measure_oracle as mo
    from test_gpu_augment import _desc_of as rgb_desc
    from test_gpu_depth_augment import _bits, _desc_of as depth_desc, _episode_arrays
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import (DepthAugment, FrameAugment, MeasurementNoise, RecordedEpisodeDataset,
                                                                       ResidentEpisodeDataset, TrainInputs)
    path = RecordedEpisodeDataset.save(str(tmp_path / "episodes.npz"), env_name="Lift", **_episode_arrays(e=4, t=4, hw=64))
    ds = ResidentEpisodeDataset(path, use_depth=True, obj_name="cube")
    ds.refresh_data(3)
    before = {k: v.clone() for k, v in ds.pool.items()}
    host = {k: v.cpu().numpy() for k, v in before.items()}
    sampler = ds.sampler(4, seed=6)
    noise = MeasurementNoise([0.001, 0.01], correlation=0.5, seed=3)
    aug = FrameAugment(brightness=0.3, erase_prob=1.0, seed=8)
    daug = DepthAugment(noise=(0.01, 0.01), holes=(1, 2), share_erase=aug, occluder_value=0.25, seed=8)
    model = types.SimpleNamespace(use_depth=True, requires_sequence=False, sequence_length=1)
    inputs = TrainInputs(model, ds, sampler=sampler, measurement_noise=noise, augment=aug, depth_augment=daug)
    stages = (sampler, noise, aug, daug)
    assert [s.step for s in stages] == [0, 0, 0, 0]
    for k in range(3):
        img, depth, x0bar, x0, x1, obj = inputs()
        index = so.window_index(sampler.desc_fields(), ds.selected, k)
        assert np.array_equal(sampler.index.cpu().numpy(), index), k
        raw = {key: so.gather(host[key], index, 1)[0] for key in ("imgs", "depths", "true_self", "true_obj")}      # S = 1, squeezed away
        want_img, table, _ = ao.augment(raw["imgs"], rgb_desc(aug, 64, 64, 0), k)
        assert img.dtype == torch.uint8 and np.array_equal(img.cpu().numpy(), want_img), k
        assert np.array_equal(aug.last_params.cpu().numpy(), table) and table[1:].reshape(-1, 8)[:, 3].all()      # every frame has an occluder
        want_depth, want_params = do.augment(raw["depths"], depth_desc(daug, 64, 64, 0), k, rgb_params=table)
        assert np.array_equal(_bits(depth.cpu().numpy()), _bits(want_depth)), k
        assert np.array_equal(daug.last_params.cpu().numpy(), want_params) and (depth == 0.25).any().item()         # the shared occluder is in it
        want_meas, want_picks = mo.measure(raw["true_self"], 3, [0.001, 0.01], 0.5, k)
        beyond, differ = mo.compare(x0bar.cpu().numpy(), want_meas)
        print("step %d: x0bar %d of %d elements beyond one ulp, %d differ" % (k, beyond, want_meas.size, differ))
        assert beyond == 0 and np.array_equal(noise.last_picks.cpu().numpy(), want_picks), k
        # the fields no stage writes are the sampler's own
        assert np.array_equal(x0.cpu().numpy(), raw["true_self"]) and np.array_equal(obj.cpu().numpy(), raw["true_obj"]) and x1 is None
        assert [s.step for s in stages] == [k + 1] * 4
    for key, v in before.items():      # nothing wrote the dataset's pools
        assert torch.equal(ds.pool[key].view(torch.uint8), v.view(torch.uint8)), key
    # the picks of one batch size outlive a call at another: a captured call would still be writing them
    x8 = torch.from_numpy(host["true_self"][:2].reshape(8, 7)).cuda()
    noise(x8)
    first, ptr = noise.last_picks, noise.last_picks.data_ptr()
    noise(x8[:4].contiguous())
    assert noise.last_picks.numel() == 5 and noise.last_picks.data_ptr() != ptr
    assert first.numel() == 9 and first.data_ptr() == ptr and noise._kept((8, x8.device), None) is first
    noise(x8)
    assert noise.last_picks is first and noise.step == 6


# -- through the training loop ----------------------------------------------------------------------------------------------------

def _model(seed=3):
    from rgb_proprioceptive_pose_estimator_amd import models as M
    torch.manual_seed(seed)
    return M.NaiveObjectStateEstimator("cube", [32], 18, 32, False, (9,), True, False, False, compute_dtype=torch.float32).cuda()


def _criterion():
    from rgb_proprioceptive_pose_estimator_amd import models as M
    crit = lambda: M.PoseDistanceLoss("combined", 1.0, 0.5, 1e-4, "pose")
    return {"x0_loss": crit(), "x1_loss": crit(), "obj_loss": crit(), "val_loss": M.PoseDistanceLoss(mode="val")}


def test_train_on_sampled_minibatches(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import train
    _, res = _datasets(tmp_path, e=4, t=4, hw=64)
    made = []
    make = res.sampler
    res.sampler = lambda *a, **kw: made.append(make(*a, **kw)) or made[-1]      # (train() makes the sampler: keep a handle on it)
    model = _model()
    opt = FusedAdam(model.parameters(), lr=1e-3)
    model, best = train(model, res, _criterion(), opt, num_epochs=2, num_train_episodes_per_epoch=2, num_val_episodes_per_epoch=1,
                        params={"camera_name": "frontview", "noise_scale": 0.001}, device="cuda:0", save_model=False, logging=False,
                        batch_size=3, shuffle_seed=21)
    assert np.isfinite(best) and len(made) == 1
    sampler = made[0]
    assert (sampler.num_windows, sampler.steps_per_epoch, sampler.sequence_length, sampler.stride, sampler.seed) == (8, 2, 1, 1, 21)
    assert sampler.step == 4 and opt.state_dict()["step"] == 4           # 2 epochs x steps_per_epoch optimizer steps; val takes none
    # epoch 0 trained on episodes [0, 1] and validated on [2]; epoch 1 trained on [3, 0]: the last batch is the oracle's step 3 of those
    assert np.array_equal(sampler.index.cpu().numpy(), so.window_index(sampler.desc_fields(), [3, 0], 3))
    assert res.selected == [1]


def test_graphed_train_step_with_a_sampler(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import GraphedTrainStep
    _, res = _datasets(tmp_path, e=4, t=4, hw=64)
    res.refresh_data(3, None, 0.001)
    sampler = res.sampler(4, seed=6)
    model = _model().train()
    step = GraphedTrainStep(model, _criterion(), FusedAdam(model.parameters(), lr=1e-3, capturable=True), True, None, warmup=2, sampler=sampler)
    assert sampler.step == 2                                   # the warm-up steps advance the counter, the capture does not
    for k in (2, 3, 4):
        loss, _, _ = step()
        assert torch.isfinite(loss).item() and sampler.step == k + 1
        want = so.window_index(sampler.desc_fields(), res.selected, k)
        assert np.array_equal(sampler.index.cpu().numpy(), want)
        assert np.array_equal(step.static[0].cpu().numpy(), so.gather(res.pool["imgs"].cpu().numpy(), want, 1)[0])      # what replay k was fed
    assert sampler.step == 2 + 3
    with pytest.raises(ValueError):
        step(tuple(step.static))
    with pytest.raises(ValueError):                            # windows of 2 timesteps for a model without a sequence
        GraphedTrainStep(model, _criterion(), FusedAdam(model.parameters(), lr=1e-3, capturable=True), True, None, warmup=1,
                         sampler=res.sampler(2, sequence_length=2))
