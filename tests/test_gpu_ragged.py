"""GPU side of episodes of unequal length: rpe_sample_windows_ragged against the numpy oracle (tests/_ragged_oracle.py) for equality,
rpe_pose_loss_masked and rpe_error_stats_ragged against their dense counterparts bit for bit where the specification says so, and
padding that never leaks through evaluate_episodes, train(), GraphedTrainStep and scripts/rollout.py."""
import numpy as np
import pytest
import torch

import _ragged_oracle as ro
import _sampler_oracle as so

pytestmark = pytest.mark.gpu

DEV = "cuda"
LENGTHS = (9, 3, 2, 4, 5, 1)      # with S = 3, stride = 2, T = 9: K = (4, 1, 0, 1, 2, 0), M = 8
PARAMS = {"camera_name": "frontview", "noise_scale": 0.0}      # no measurement noise: a measurement is a function of the file alone


def _ops():
    from rgb_proprioceptive_pose_estimator_amd import ops
    return ops


def _i32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(DEV)


def _bits(t):
    """the bit patterns of a float tensor, as numpy integers (NaN compares equal to itself)"""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64).numpy()


# -- the index kernel -------------------------------------------------------------------------------------------------------------

def _random_lengths(e_file, t, seed):
    n = np.random.default_rng(seed).integers(1, t + 1, e_file)
    n[:2] = (1, t)      # both ends are in
    return n


# name -> (lengths of the file, sel, T, S, stride, N)
INDEX_CASES = {
    "edges": (LENGTHS, [3, 0, 5, 4, 1, 2], 9, 3, 2, 3),
    "edges_N_above_M": (LENGTHS, [3, 0, 5, 4, 1, 2], 9, 3, 2, 11),
    "E1": ([9, 5], [1], 9, 3, 2, 3),                                                        # M = 2
    "E257": (_random_lengths(300, 9, 1), np.random.default_rng(2).permutation(300)[:257], 9, 3, 2, 7),   # two scan elements per thread
    "E8192": (_random_lengths(8192, 4, 3), np.random.default_rng(4).permutation(8192), 4, 2, 1, 64),      # the whole LDS table
}


@pytest.mark.parametrize("shuffle", [0, 1])
@pytest.mark.parametrize("case", list(INDEX_CASES))
def test_index_equals_the_oracle(case, shuffle):
    ops = _ops()
    lengths, sel, t, s, stride, n = INDEX_CASES[case]
    d = dict(seed=0xC0FFEE1234, E=len(sel), T=t, S=s, stride=stride, N=n, shuffle=shuffle)
    m = ro.window_table(d, sel, lengths)[2]
    assert m >= 1 and (case != "edges_N_above_M" or n > m)
    oracle = ro.window_index if len(sel) <= 16 else ro.window_index_fast
    sel_d, len_d = _i32(sel), _i32(lengths)
    # steps 0 and 1, the step whose draws reach the end of epoch 0, and the last value of the 32-bit counter (it wraps to 0)
    for step in (0, 1, m // n, 2 ** 32 - 1):
        state = torch.tensor([step - 2 ** 32 if step >= 2 ** 31 else step], dtype=torch.int32, device=DEV)
        idx = ops.sample_windows_ragged(ops.sample_desc(**d), sel_d, len_d, state)
        want = oracle(d, sel, lengths, step)
        assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), want), (step, idx.tolist()[:9], want.tolist()[:9])
        assert int(state.item()) & 0xFFFFFFFF == (step + 1) & 0xFFFFFFFF
        ep, t0 = want[1::2], want[2::2]
        assert (t0 + s <= np.asarray(lengths)[ep]).all()      # (the oracle's windows stay inside their episodes)


def test_index_refuses_more_episodes_than_the_table_holds():
    ops = _ops()
    from rgb_proprioceptive_pose_estimator_amd._lib import RpeError
    sel, lengths, state = torch.zeros(8193, dtype=torch.int32, device=DEV), torch.ones(8193, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RpeError, match="8192"):
        ops.sample_windows_ragged(ops.sample_desc(seed=1, E=8193, T=4, S=1, stride=1, N=2, shuffle=1), sel, lengths, state)
    assert state.item() == 0      # nothing was launched


@pytest.mark.parametrize("shuffle", [0, 1])
def test_equal_lengths_give_the_dense_table(shuffle):
    ops = _ops()
    sel = _i32([3, 0, 1])
    for t, s, stride, n in ((7, 3, 1, 4), (7, 1, 1, 5), (7, 7, 1, 5), (9, 3, 2, 16)):
        d = ops.sample_desc(seed=5, E=3, T=t, S=s, stride=stride, N=n, shuffle=shuffle)
        full = torch.full((4,), t, dtype=torch.int32, device=DEV)
        for step in (0, 3, 2 ** 31 + 5):
            a, b = (torch.tensor([step - 2 ** 32 if step >= 2 ** 31 else step], dtype=torch.int32, device=DEV) for _ in range(2))
            assert torch.equal(ops.sample_windows_ragged(d, sel, full, a), ops.sample_windows(d, sel, b)) and torch.equal(a, b), (t, s, stride, n, step)


def test_a_second_launch_follows_sel_and_lengths_rewritten_in_place():
    ops = _ops()
    d = dict(seed=3, E=3, T=9, S=3, stride=2, N=6, shuffle=1)
    sel, lengths, state = _i32([0, 1, 2]), _i32(LENGTHS), torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.empty(13, dtype=torch.int32, device=DEV)
    assert ops.sample_windows_ragged(ops.sample_desc(**d), sel, lengths, state, out=out) is out
    assert np.array_equal(out.cpu().numpy(), ro.window_index(d, [0, 1, 2], LENGTHS, 0))
    sel.copy_(_i32([4, 5, 3]))
    ops.sample_windows_ragged(ops.sample_desc(**d), sel, lengths, state, out=out)
    assert np.array_equal(out.cpu().numpy(), ro.window_index(d, [4, 5, 3], LENGTHS, 1))
    other = (3, 3, 3, 9, 7, 2)
    lengths.copy_(_i32(other))
    ops.sample_windows_ragged(ops.sample_desc(**d), sel, lengths, state, out=out)
    want = ro.window_index(d, [4, 5, 3], other, 2)
    assert np.array_equal(out.cpu().numpy(), want) and not np.array_equal(want, ro.window_index(d, [4, 5, 3], LENGTHS, 2))


def test_no_window_at_all_is_in_bounds():
    ops = _ops()
    d = ops.sample_desc(seed=3, E=2, T=9, S=3, stride=2, N=3, shuffle=1)
    state = torch.tensor([4], dtype=torch.int32, device=DEV)
    idx = ops.sample_windows_ragged(d, _i32([5, 2]), _i32(LENGTHS), state)      # lengths 1 and 2: no window of 3
    assert idx.tolist() == [4, 5, 0, 5, 0, 5, 0] and state.item() == 5


def test_torch_ops_equal_the_wrappers():
    ops = _ops()
    import rgb_proprioceptive_pose_estimator_amd.torch_ops  # noqa: F401  (registers torch.ops.rpe.*)
    d = dict(seed=5, E=6, T=9, S=3, stride=2, N=4, shuffle=1)
    state = torch.tensor([2], dtype=torch.int32, device=DEV)
    idx = torch.ops.rpe.sample_windows_ragged([d[k] for k in ops.SAMPLE_DESC_FIELDS], _i32(range(6)), _i32(LENGTHS), state)
    assert np.array_equal(idx.cpu().numpy(), ro.window_index(d, list(range(6)), LENGTHS, 2)) and state.item() == 3
    pred, truth, valid = _loss_case(7)
    out3, grad = torch.ops.rpe.pose_loss_masked(pred, truth, valid, 3, 1, 1.0, 0.5, 1e-4)
    want3, wantg = ops.pose_loss(pred, truth, 3, 1, 1.0, 0.5, 1e-4, valid=valid)
    assert torch.equal(out3, want3) and torch.equal(grad, wantg)
    err, n = torch.rand(3, 4, device=DEV), _i32([4, 1, 2])
    assert torch.equal(torch.ops.rpe.error_stats_ragged(err, n), ops.error_stats(err, n))


# -- the masked loss --------------------------------------------------------------------------------------------------------------

_LOSS = {}


def _loss_case(n):
    """(pred, truth, valid) on the device, made once and never written: truth has unit quaternions with w >= 0, the mask is random and
    never all zero"""
    if n not in _LOSS:
        g = torch.Generator().manual_seed(100 + n)
        pred = torch.randn(n, 7, generator=g)
        q = torch.randn(n, 4, generator=g)
        q = q / q.norm(dim=-1, keepdim=True)
        truth = torch.cat([torch.randn(n, 3, generator=g), torch.where(q[:, 3:] < 0, -q, q)], -1)
        valid = (torch.rand(n, generator=g) < 0.6).to(torch.uint8)
        valid[n // 2] = 1
        if n > 1:
            valid[0] = 0
        _LOSS[n] = (pred.to(DEV), truth.to(DEV), valid.to(DEV))
    return _LOSS[n]


def _within_one_ulp(a, b):
    a, b = np.float32(a), np.float32(b)
    return a == b or a == np.nextafter(b, np.float32(np.inf)) or a == np.nextafter(b, np.float32(-np.inf))


@pytest.mark.parametrize("n", [1, 7, 257])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("metric", [0, 1, 2, 3])
def test_masked_loss(metric, mode, n):
    """The 1-ulp allowance on the sums: the masked call and the dense call on the compacted rows both round ONE fp64 sum to fp32; the two
    fp64 sums hold the same terms in another order (a row's thread is its index mod 256, and compaction moves the rows), and
    reordering an fp64 sum of at most 257 non-negative terms moves it by less than 257 * 2^-53 = 3e-14 relative -- eight orders
    below half an fp32 ulp, so the rounded values agree unless the sum lies on a rounding boundary, where they are neighbours."""
    ops = _ops()
    pred, truth, valid = _loss_case(n)
    args = (metric, mode, 1.5, 0.5, 1e-4)
    dense3, dense_g = ops.pose_loss(pred, truth, *args)
    # an all-ones mask: the dense bits, uint8 and bool alike
    for ones in (torch.ones(n, dtype=torch.uint8, device=DEV), torch.ones(n, dtype=torch.bool, device=DEV)):
        out3, grad = ops.pose_loss(pred, truth, *args, valid=ones)
        assert np.array_equal(_bits(out3), _bits(dense3)) and np.array_equal(_bits(grad), _bits(dense_g))
    # a random mask
    out3, grad = ops.pose_loss(pred, truth, *args, valid=valid)
    keep = valid.bool()
    assert np.array_equal(_bits(grad[keep]), _bits(dense_g[keep]))
    assert (_bits(grad[~keep]) == 0).all()      # +0.0, not -0.0
    want3, _ = ops.pose_loss(pred[keep].contiguous(), truth[keep].contiguous(), *args)
    got, want = out3.cpu().numpy(), want3.cpu().numpy()
    print("metric %d mode %d n %d: masked %r compacted %r" % (metric, mode, n, got.tolist(), want.tolist()))
    assert all(_within_one_ulp(a, b) for a, b in zip(got, want)) and np.isfinite(got).all()
    # whatever the masked rows hold changes no bit
    for junk in (float("nan"), float("inf"), 0.0):
        p2, t2 = pred.clone(), truth.clone()
        p2[~keep] = junk
        t2[~keep] = junk
        o2, g2 = ops.pose_loss(p2, t2, *args, valid=valid)
        assert np.array_equal(_bits(o2), _bits(out3)) and np.array_equal(_bits(g2), _bits(grad)), junk
    o2, _ = ops.pose_loss(pred, truth, *args, want_grad=False, valid=valid)      # without the gradient: the same sums
    assert np.array_equal(_bits(o2), _bits(out3))
    # all rows masked
    p2 = torch.full_like(pred, float("nan"))
    out3, grad = ops.pose_loss(p2, p2, *args, valid=torch.zeros(n, dtype=torch.uint8, device=DEV))
    assert (_bits(out3) == 0).all() and (_bits(grad) == 0).all()


def test_pose_distance_loss_takes_the_mask():
    from rgb_proprioceptive_pose_estimator_amd import models as M
    pred, truth, valid = _loss_case(7)
    pred, truth, valid = pred.reshape(7, 1, 7), truth.reshape(7, 1, 7), valid.reshape(7, 1)
    keep = valid.bool()
    crit, val = M.PoseDistanceLoss("combined", 2.0, 0.5, 1e-4, "pose"), M.PoseDistanceLoss(mode="val")
    p = pred.clone().requires_grad_(True)
    poisoned = truth.clone()
    poisoned[~keep] = float("nan")
    loss = crit(p, poisoned, valid=valid)
    loss.backward()
    q = pred[keep].clone().requires_grad_(True)
    want = crit(q, truth[keep])
    want.backward()
    assert _within_one_ulp(loss.item(), want.item()) and torch.equal(p.grad[keep], q.grad) and (_bits(p.grad[~keep]) == 0).all()
    a, b = val.forward_device(pred, poisoned, valid=keep), val.forward_device(pred[keep], truth[keep])      # a bool mask
    assert all(_within_one_ulp(x.item(), y.item()) for x, y in zip(a, b))
    pe, oe = val(pred, poisoned, valid=valid)
    assert np.isfinite(pe) and np.isfinite(oe)
    assert torch.equal(crit(pred, truth, valid=None), crit(pred, truth))
    for bad in (valid.float(), valid[:3], valid.cpu(), valid.reshape(7)):
        with pytest.raises(ValueError):
            crit(pred, truth, valid=bad)


# -- the ragged statistics --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("e,t", [(1, 1), (3, 4), (7, 37), (16, 256)])
def test_ragged_stats(e, t):
    """rtol 1e-9 / atol 1e-300: the bars of test_gpu_evaluate.py::test_error_stats_match_numpy (the worst-case reordering bound of an
    fp64 sum of 4096 values is 4.5e-13)"""
    ops = _ops()
    rng = np.random.default_rng(e * 1000 + t)
    x = (rng.random((e, t)) * 3.0).astype(np.float32)
    lengths = rng.integers(1, t + 1, e)
    lengths[0] = t
    lengths[-1] = 1 if e > 1 else t      # both ends are in
    xd, nd = torch.from_numpy(x).to(DEV), _i32(lengths)
    got = ops.error_stats(xd, nd)
    again = ops.error_stats(xd, nd)
    assert got.dtype == torch.float64 and got.shape == (3 + 2 * e,) and np.array_equal(_bits(got), _bits(again))
    want = ro.error_stats(x, lengths)
    g = got.cpu().numpy()
    print("(%d, %d): worst rel %.2e" % (e, t, np.abs(g / np.where(want == 0, 1, want) - 1).max()))
    np.testing.assert_allclose(g, want, rtol=1e-9, atol=1e-300)
    assert g[2] == want[2]
    # full lengths: the dense kernel's bits
    full = torch.full((e,), t, dtype=torch.int32, device=DEV)
    assert np.array_equal(_bits(ops.error_stats(xd, full)), _bits(ops.error_stats(xd)))
    # NaN (and inf) in the padding is invisible
    mask = ro.valid_mask(lengths, t)
    for junk in (np.nan, np.inf):
        y = x.copy()
        y[~mask] = junk
        assert np.array_equal(_bits(ops.error_stats(torch.from_numpy(y).to(DEV), nd)), _bits(got)), junk
    # NaN in a valid entry spoils exactly the figures it takes part in: the totals, and its episode's sum and mean
    r = e // 2
    y = x.copy()
    y[r, lengths[r] - 1] = np.nan
    bad = ops.error_stats(torch.from_numpy(y).to(DEV), nd).cpu().numpy()
    spoiled = np.zeros(3 + 2 * e, dtype=bool)
    spoiled[[0, 1, 2, 3 + r, 3 + e + r]] = True
    assert np.isnan(bad[spoiled]).all() and np.array_equal(bad[~spoiled], g[~spoiled])


def test_ragged_stats_arguments():
    ops = _ops()
    x = torch.zeros(2, 3, device=DEV)
    for bad in (torch.ones(2, dtype=torch.int64, device=DEV), torch.ones(3, dtype=torch.int32, device=DEV), torch.ones(2, dtype=torch.int32)):
        with pytest.raises(ValueError):
            ops.error_stats(x, bad)


# -- files: dense D, ragged R with the same arrays, and R' with other padding ---------------------------------------------------------

E, T, HW = 3, 6, 64
R_LENGTHS = (6, 2, 4)


def _poses(rng, e, t):
    q = rng.normal(size=(e, t, 4))
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    return np.concatenate([rng.random((e, t, 3)), np.where(q[..., 3:] < 0, -q, q)], -1).astype(np.float32)


def _arrays(e=E, t=T, seed=0):
    rng = np.random.default_rng(seed)
    return dict(imgs=rng.integers(0, 256, (e, t, HW, HW, 3), dtype=np.uint8), true_self=_poses(rng, e, t), true_obj=_poses(rng, e, t))


def _poisoned(arrays, lengths, seed=9):
    """the same episodes with other padding: random bytes in the frames, NaN in the poses"""
    rng = np.random.default_rng(seed)
    out = {k: v.copy() for k, v in arrays.items()}
    for e, n in enumerate(lengths):
        out["imgs"][e, n:] = rng.integers(0, 256, out["imgs"][e, n:].shape, dtype=np.uint8)
        out["true_self"][e, n:] = np.nan
        out["true_obj"][e, n:] = np.nan
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """paths of D, R, R' (made once; the tests only read them)"""
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset
    d = tmp_path_factory.mktemp("ragged")
    arrays, n = _arrays(), np.asarray(R_LENGTHS, dtype=np.int32)
    return dict(D=RecordedEpisodeDataset.save(str(d / "dense.npz"), env_name="Lift", **arrays),
                R=RecordedEpisodeDataset.save(str(d / "ragged.npz"), env_name="Lift", lengths=n, **arrays),
                Rp=RecordedEpisodeDataset.save(str(d / "ragged_poisoned.npz"), env_name="Lift", lengths=n, **_poisoned(arrays, R_LENGTHS)))


def _model(kind, seed=5):
    from rgb_proprioceptive_pose_estimator_amd import models as M
    torch.manual_seed(seed)
    if kind == "tdo":
        m = M.TemporallyDependentObjectStateEstimator("cube", 32, 18, 32, 2, 0.1, False, (9,), False, False, False, compute_dtype=torch.float32)
    else:
        m = M.NaiveObjectStateEstimator("cube", [32], 18, 32, False, (9,), False, False, False, compute_dtype=torch.float32)
    return m.cuda()


def _criterion():
    from rgb_proprioceptive_pose_estimator_amd import models as M
    crit = lambda: M.PoseDistanceLoss("combined", 1.0, 0.5, 1e-4, "pose")
    return {"x0_loss": crit(), "x1_loss": crit(), "obj_loss": crit(), "val_loss": M.PoseDistanceLoss(mode="val")}


def _same_evaluation(a, b):
    for name in ("outputs", "poses", "pos_err", "ori_err", "measurements", "truth"):
        assert np.array_equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    assert np.array_equal(a.stats.view(np.int64), b.stats.view(np.int64)) and np.array_equal(a.lengths, b.lengths)


# -- evaluate_episodes ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["tdo", "no"])
def test_evaluation_never_reads_the_padding(kind, files):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset, ResidentEpisodeDataset
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import evaluate_episodes
    model = _model(kind)
    run = lambda name, cls=RecordedEpisodeDataset, **kw: evaluate_episodes(model, cls(files[name], obj_name="cube"), E, PARAMS, max_frames=2 * E, **kw)
    dense, ragged, poisoned = run("D"), run("R"), run("Rp")      # three chunks of two timesteps: the LSTM state is carried across them
    assert dense.lengths is None and isinstance(ragged.lengths, np.ndarray) and ragged.lengths.tolist() == list(R_LENGTHS)
    mask = torch.from_numpy(ro.valid_mask(R_LENGTHS, T)).to(DEV)
    for name in ("pos_err", "ori_err", "outputs", "poses", "measurements", "truth"):
        a, b = getattr(dense, name), getattr(ragged, name)
        assert np.array_equal(_bits(a[mask]), _bits(b[mask])) and torch.isfinite(b[mask]).all(), name      # where the episode exists: the dense bits
        assert torch.isnan(b[~mask]).all(), name                                                          # beyond: NaN
    for i, err in enumerate((ragged.pos_err, ragged.ori_err)):
        want = ro.error_stats(err.cpu().numpy(), R_LENGTHS)
        np.testing.assert_allclose(ragged.stats[0, i], want, rtol=1e-9, atol=1e-300)
    assert ragged.pos_episode_mean.shape == (E,) and np.isfinite(ragged.stats).all()
    assert np.allclose(ragged.pos_episode_sum / np.asarray(R_LENGTHS), ragged.pos_episode_mean, rtol=1e-12)
    assert len(ragged.summary().splitlines()) == len(dense.summary().splitlines())
    _same_evaluation(ragged, poisoned)      # the padding never leaks
    _same_evaluation(ragged, run("Rp", cls=ResidentEpisodeDataset))      # nor through the resident dataset's gathered chunks
    if kind == "tdo":      # one sweep, K = 2
        a, b = run("R", noise_scales=[0.0, 0.01], noise_seed=4), run("Rp", noise_scales=[0.0, 0.01], noise_seed=4)
        _same_evaluation(a, b)
        assert tuple(a.pos_err.shape) == (2, E, T) and torch.isnan(a.pos_err[:, ~mask]).all() and torch.isfinite(a.pos_err[:, mask]).all()
        for k in range(2):
            np.testing.assert_allclose(a.stats[k, 1], ro.error_stats(a.ori_err[k].cpu().numpy(), R_LENGTHS), rtol=1e-9, atol=1e-300)


# -- training ---------------------------------------------------------------------------------------------------------------------

class _NoOptimizer:
    def zero_grad(self):
        pass


def _val_by_hand(model, ds, seq, masked=True):
    """the `val` phase of train() on the episodes `ds` has selected, by hand: (loss, pos_err, ori_err) sums / the timesteps that exist"""
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import model_batch
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import train_step
    model.eval()
    model.reset_initial_state(ds.num_selected)
    sums = torch.zeros(3, dtype=torch.float64, device=DEV)
    for t0 in range(0, T, seq):
        batch = model_batch(ds.chunk(t0, min(seq, T - t0)), model.requires_sequence)
        valid = ds.valid(t0, min(seq, T - t0)) if masked else None
        loss, pe, oe = train_step(model, batch, _criterion(), _NoOptimizer(), True, "val", None, valid=valid)
        sums += torch.stack([loss.double(), pe.double(), oe.double()])
    return [v / int(ds.selected_lengths.sum()) for v in sums.tolist()]


def test_train_on_a_ragged_file(files):
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import ResidentEpisodeDataset
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import train
    ds = ResidentEpisodeDataset(files["R"], obj_name="cube")
    made = []
    make = ds.sampler
    ds.sampler = lambda *a, **kw: made.append(make(*a, **kw)) or made[-1]      # (train() makes the sampler: keep a handle on it)
    model = _model("tdo")
    opt = FusedAdam(model.parameters(), lr=1e-3)
    model, best = train(model, ds, _criterion(), opt, num_epochs=2, num_train_episodes_per_epoch=2, num_val_episodes_per_epoch=1, params=PARAMS,
                        device="cuda:0", save_model=False, logging=False, batch_size=2)
    sampler = made[0]
    # episodes 0 and 1 (6 and 2 timesteps) hold 3 + 1 windows of 2: two steps an epoch, and no window ever reached into padding
    assert np.isfinite(best) and sampler.step == 4 and opt.state_dict()["step"] == 4 and ds.selected == [2]
    # (the sampler's figures follow the selection: the last `val` phase left episode 2, 4 timesteps, selected)
    assert sampler.ragged and (sampler.windows_per_episode, sampler.num_windows, sampler.steps_per_epoch) == ([2], 2, 1)
    assert np.array_equal(sampler.index.cpu().numpy(), ro.window_index(sampler.desc_fields(), [0, 1], R_LENGTHS, 3))
    # the best `val` loss is the hand loop's over episode 2 (4 of 6 timesteps) with the weights train() returned, divided by 4
    ds.refresh_data(2, None, 0.0)
    ds.refresh_data(1, None, 0.0)
    assert ds.selected == [2] and ds.selected_lengths.tolist() == [4]
    by_hand = _val_by_hand(model, ds, 2)
    print("best val loss %r, by hand %r" % (best, by_hand))
    assert best == by_hand[0] and all(np.isfinite(by_hand))
    # the same numbers from the file with other padding, bit for bit
    other = ResidentEpisodeDataset(files["Rp"], obj_name="cube")
    other.refresh_data(2, None, 0.0)
    other.refresh_data(1, None, 0.0)
    assert _val_by_hand(model, other, 2) == by_hand
    # the mask is what keeps the padding out: without it the NaN poses behind the episode's end reach the sums
    assert np.isnan(_val_by_hand(model, other, 2, masked=False)[0])


def test_graphed_train_step_with_a_ragged_sampler(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset, ResidentEpisodeDataset
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import GraphedTrainStep
    lengths = (6, 2, 4, 3, 6, 5)
    path = RecordedEpisodeDataset.save(str(tmp_path / "six.npz"), env_name="Lift", lengths=np.asarray(lengths), **_poisoned(_arrays(e=6, seed=1), lengths))
    ds = ResidentEpisodeDataset(path, obj_name="cube")
    ds.refresh_data(3, None, 0.001)
    sampler = ds.sampler(4, seed=6)      # windows of one timestep: episodes 0, 1, 2 hold 6 + 2 + 4
    assert sampler.num_windows == 12
    model = _model("no").train()
    step = GraphedTrainStep(model, _criterion(), FusedAdam(model.parameters(), lr=1e-3, capturable=True), True, None, warmup=2, sampler=sampler)
    imgs = ds.pool["imgs"].cpu().numpy()
    for k in (2, 3, 4):
        loss, _, _ = step()
        want = ro.window_index(sampler.desc_fields(), ds.selected, lengths, k)
        assert torch.isfinite(loss).item() and sampler.step == k + 1      # (a window in the NaN padding would have made the loss NaN)
        assert np.array_equal(sampler.index.cpu().numpy(), want)
        assert np.array_equal(step.static[0].cpu().numpy(), so.gather(imgs, want, 1)[0])      # what replay k was fed
    ds.refresh_data(3, None, 0.001)      # episodes 3, 4, 5: 3 + 6 + 5 windows, another domain for the permutation
    assert ds.selected == [3, 4, 5] and sampler.num_windows == 14
    loss, _, _ = step()
    want = ro.window_index(sampler.desc_fields(), [3, 4, 5], lengths, 5)
    assert torch.isfinite(loss).item() and np.array_equal(sampler.index.cpu().numpy(), want)
    assert not np.array_equal(want, ro.window_index(sampler.desc_fields(), [0, 1, 2], lengths, 5))


def test_sampler_batch_equals_the_oracle_gather(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import RecordedEpisodeDataset, ResidentEpisodeDataset
    rng = np.random.default_rng(0)
    eps = [dict(imgs=rng.integers(0, 256, (t, 16, 16, 3), dtype=np.uint8), true_self=_poses(rng, 1, t)[0], true_obj=_poses(rng, 1, t)[0]) for t in LENGTHS]
    ds = ResidentEpisodeDataset(RecordedEpisodeDataset.pack(str(tmp_path / "p.npz"), eps, env_name="Lift"), obj_name="cube")
    ds.refresh_data(4, None, 0.01)
    ds.refresh_data(4, None, 0.01)      # wraps: episodes 4, 5, 0, 1
    sampler = ds.sampler(3, sequence_length=3, stride=2, seed=11)
    assert sampler.windows_per_episode == [2, 0, 4, 1]
    v = ds.valid(1, 3)
    assert v.is_cuda and v.dtype == torch.uint8 and np.array_equal(v.cpu().numpy().astype(bool), ro.valid_mask([5, 1, 9, 3], 9)[:, 1:4].T)
    for k in range(4):      # 7 windows, 3 a step: the third step crosses into the next epoch
        batch = sampler()
        want = ro.window_index(sampler.desc_fields(), ds.selected, LENGTHS, k)
        assert np.array_equal(sampler.index.cpu().numpy(), want)
        for got, key in zip(batch, ("imgs", None, "measurement_self", "true_self", None, "true_obj")):
            assert (got is None) if key is None else np.array_equal(got.cpu().numpy(), ro.gather(ds.pool[key].cpu().numpy(), want, 3)), key


# -- the scripts ------------------------------------------------------------------------------------------------------------------

def test_rollout_script_on_a_ragged_file(files, tmp_path, capsys):
    from rgb_proprioceptive_pose_estimator_amd.scripts.rollout import main
    cam = str(tmp_path / "camera.npy")
    np.save(cam, np.array([[50.0, 0, 8, 12], [0, 46.0, 6, 9], [0, 0, 1.0, 1.5]]))
    flags = lambda name: ["--model", "no", "--latent_dim", "32", "--hidden_dim", "32", "--obj_name", "cube", "--dtype", "f32", "--episodes", files[name],
                          "--n_episodes", str(E), "--noise_scale", "0", "--out", str(tmp_path / "o.npy")]
    common = flags("R")
    errs, video = str(tmp_path / "errs.npz"), str(tmp_path / "v.npy")
    res = main(common + ["--batched", "--errors_out", errs])
    with np.load(errs) as f:
        assert f["lengths"].tolist() == list(R_LENGTHS) and f["pos_err"].shape == (E, T)
        assert np.array_equal(np.isnan(f["pos_err"]), ~ro.valid_mask(R_LENGTHS, T)) and np.array_equal(np.isnan(f["poses"][..., 0]), ~ro.valid_mask(R_LENGTHS, T))
    assert "EVALUATION COMPLETED" in capsys.readouterr().out and res.lengths.tolist() == list(R_LENGTHS)
    main(common + ["--video_out", video, "--camera_matrix", cam])
    assert "wrote %d frames" % sum(R_LENGTHS) in capsys.readouterr().out
    frames = np.load(video)
    assert frames.dtype == np.uint8 and frames.shape == (sum(R_LENGTHS), HW, HW, 3)
    # the same video from the file with other padding
    main(flags("Rp") + ["--video_out", str(tmp_path / "w.npy"), "--camera_matrix", cam])
    assert np.array_equal(np.load(str(tmp_path / "w.npy")), frames)
