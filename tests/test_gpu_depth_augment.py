"""GPU side of the depth augmentation: rpe_augment_depth_f32 against the numpy fp64 oracle (tests/_depth_augment_oracle.py).  The
arithmetic is specified to the bit, so every comparison is `np.array_equal` on the uint32 view of the floats -- output, parameter
table and step counter -- and then the feature through DepthAugment, the torch operator, a captured graph, train() and
GraphedTrainStep (that test is last: see DESIGN.md sections 3 and 5 on captured train steps)."""
import ctypes

import numpy as np
import pytest
import torch

import _augment_oracle as ao
import _depth_augment_oracle as do

pytestmark = pytest.mark.gpu

FULL = 2 ** 32 - 1

# the kernel walks the batch as one flat array in groups of 4 pixels (one 16-byte load), the remainder one pixel per thread:
SHAPES = {
    "sub_group": (1, 1, 3, 1),        # 3 pixels: fewer than one group
    "tail": (1, 5, 7, 1),             # 35 pixels: eight groups and three single pixels; every pixel single from a pointer off the 16-byte grid
    "odd": (3, 33, 47, 1),            # 1551 pixels per frame (= 3 mod 4): frame boundaries inside groups, five workgroups, a tail
    "grouped": (3, 2, 16, 24, 1),     # (S, N) windows: group = N and group = 0
    "rects": (2, 64, 64, 1),          # four rectangles per frame
    "planes": (2, 1, 16, 24),         # the synthetic dataset's layout (B, 1, H, W)
}
SPECIALS = np.array([0x80000000, 0x7FC00000, 0x00000001, 0x00000000, 0x3F800000, 0x7F800000, 0xFF800000], dtype=np.uint32)   # -0.0 NaN denormal 0.0 1.0 +inf -inf


def _features(hs, ws):
    """desc settings by name: every feature alone, and all together"""
    n = do.sigma_to_n(0.05, 0.02, 0.004)
    rect = dict(hh_lo=1, hh_hi=max(1, hs // 2), hw_lo=1, hw_hi=max(1, ws // 2))
    return {
        "neutral": {},
        "noise_constant": dict(n0=n[0]),
        "noise_linear": dict(n1=n[1]),
        "noise_quadratic": dict(n2=n[2]),
        "quant": dict(q=0.0625, inv_q=16.0),
        "quant_odd": dict(q=0.3, inv_q=1.0 / 0.3),
        "clamp": dict(lo=0.0, hi=7.5),
        "clamp_low_only": dict(lo=2.0),
        "drop_half": dict(drop_thresh=1 << 31, hole_value=-1.0),
        "drop_full": dict(drop_thresh=FULL, hole_value=-1.0),
        "holes_fixed": dict(hole_lo=2, hole_hi=2, hole_value=-2.0, **rect),
        "holes_drawn": dict(hole_lo=0, hole_hi=4, hole_value=-2.0, **rect),
        "four_holes": dict(hole_lo=4, hole_hi=4, hole_value=float("nan"), **rect),
        "all": dict(n0=n[0], n1=n[1], n2=n[2], q=0.0078125, inv_q=128.0, lo=0.25, hi=9.0, drop_thresh=1 << 30, hole_lo=1, hole_hi=4, hole_value=-1.0, **rect),
    }


_INPUTS = {}


def _input(name):
    """seeded depth of one shape: finite values in [0, 10] with -0.0, NaN, a denormal, 0.0, 1.0, +inf and -inf planted (as many as fit;
    made once, shared, never written to)"""
    if name not in _INPUTS:
        shape = SHAPES[name]
        rng = np.random.default_rng(len(name) * 131 + sum(shape))
        d = (10.0 * rng.random(shape)).astype(np.float32)
        flat = d.reshape(-1).view(np.uint32)
        stride = max(1, flat.size // (2 * len(SPECIALS)))
        k = min(len(SPECIALS), flat.size)
        flat[:k * stride:stride] = SPECIALS[:k]
        d.setflags(write=False)
        _INPUTS[name] = d
    return _INPUTS[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _to_desc(d):
    from rgb_proprioceptive_pose_estimator_amd import ops
    return ops.depth_augment_desc(**d)


def _device(depth, misaligned=False):
    """the depth frames on the device; misaligned: 4 bytes off the 16-byte grid"""
    t = torch.from_numpy(depth.copy())
    if not misaligned:
        dev = t.cuda()
        assert dev.data_ptr() % 16 == 0
        return dev
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


_ORACLE = {}


def _oracle(depth, desc, step):
    """the oracle's (out, params) of one case, computed once (the inputs are shared read-only arrays)"""
    key = (id(depth), tuple(sorted((k, repr(v)) for k, v in desc.items())), step)
    if key not in _ORACLE:
        _ORACLE[key] = do.augment(depth, desc, step)
    return _ORACLE[key]


def _i32(u):
    """a 32-bit word as the int32 tensor element that holds it"""
    return u - (1 << 32) if u >= (1 << 31) else u


def _check(depth, desc, step, in_place=False, misaligned=False, rgb_params=None, want=None):
    from rgb_proprioceptive_pose_estimator_amd import ops
    want, want_params = _oracle(depth, desc, step) if want is None else want
    hs, ws = do.frame_hw(depth.shape)
    g = do.num_streams(desc, depth.size // (hs * ws))
    dev = _device(depth, misaligned)
    state = torch.tensor([_i32(step), -7], dtype=torch.int32, device="cuda")
    params = torch.full((1 + 17 * g + 2,), -5, dtype=torch.int32, device="cuda")
    out = ops.augment_depth_f32(dev, _to_desc(desc), state, out=dev if in_place else None, params=params, rgb_params=rgb_params, rgb_group=desc["group"])
    if in_place:
        assert out.data_ptr() == dev.data_ptr()
    else:
        assert np.array_equal(_bits(dev.cpu().numpy()), _bits(depth)), "the input was written"
    assert state.tolist() == [_i32((step + 1) & FULL), -7]                                  # the counter moved by one; the guard word did not
    got_params = params.cpu().numpy()
    assert np.array_equal(got_params[:1 + 17 * g], want_params) and got_params[1 + 17 * g:].tolist() == [-5, -5]
    got = out.cpu().numpy()
    assert got.shape == depth.shape
    assert np.array_equal(_bits(got), _bits(want)), "%d of %d pixels differ" % ((_bits(got) != _bits(want)).sum(), got.size)
    return got


@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_equals_the_oracle(shape):
    depth = _input(shape)
    hs, ws = do.frame_hw(depth.shape)
    groups = (0, depth.shape[1]) if depth.ndim == 5 else (0,)
    finite = np.isfinite(depth)
    for i, (name, kw) in enumerate(_features(hs, ws).items()):
        for group in groups:
            desc = do.neutral_desc(seed=0x9E3779B97F4A7C15 + i, group=group, **kw)
            got = _check(depth, desc, step=3 + i)
            if name in ("neutral", "clamp_low_only") or name.startswith(("noise", "quant")):
                assert np.array_equal(_bits(got)[~finite], _bits(depth)[~finite])            # NaN and +-inf keep their bit patterns
            if name == "neutral":
                assert np.array_equal(_bits(got), _bits(depth))
            if name.startswith("noise") and depth.size >= 30:
                assert (got[finite] != depth[finite]).mean() > 0.5
            if name == "clamp" and (depth[finite] > 7.5).any():
                assert got[finite].max() == 7.5
            if name == "drop_full":
                assert (got == -1.0).mean() >= 1.0 - 2.0 / depth.size - 1e-3
            if name == "four_holes" and depth.size >= 30:
                assert np.isnan(got).sum() > np.isnan(depth).sum()
            _check(depth, desc, step=3 + i, in_place=True)
    if shape in ("tail", "odd"):      # every pixel through the one-pixel path
        for name in ("all", "noise_quadratic"):
            desc = do.neutral_desc(seed=5, **_features(hs, ws)[name])
            _check(depth, desc, step=9, misaligned=True)
            _check(depth, desc, step=9, misaligned=True, in_place=True)


def test_both_layouts_are_the_same_memory():
    depth = _input("planes")
    desc = do.neutral_desc(seed=8, **_features(16, 24)["all"])
    a = _check(depth, desc, step=1)
    want, want_params = _oracle(depth, desc, 1)
    b = _check(np.ascontiguousarray(depth.reshape(2, 16, 24, 1)), desc, step=1, want=(want.reshape(2, 16, 24, 1), want_params))
    assert np.array_equal(_bits(a).reshape(-1), _bits(b).reshape(-1))


def test_step_and_seed_extremes():
    depth = _input("rects")
    kw = _features(64, 64)["all"]
    _check(depth, do.neutral_desc(seed=2 ** 64 - 1, **kw), step=FULL)                         # the counter wraps to 0
    a = _check(depth, do.neutral_desc(seed=2, **kw), step=0)
    b = _check(depth, do.neutral_desc(seed=2, **kw), step=1 << 31)
    assert not np.array_equal(_bits(a), _bits(b))


def _mixed_step(rgb, b, hs, ws):
    """the first step at which some streams of the RGB descriptor erase and some do not"""
    for step in range(64):
        e = ao.params_table(rgb, b, hs, ws, step)[1:].reshape(-1, 8)[:, 3]
        if 0 < e.sum() < e.size:
            return step
    raise AssertionError("no step with mixed erase flags")


@pytest.mark.parametrize("grouped", [False, True])
def test_shared_occluder_equals_the_two_oracles_chained(grouped):
    from rgb_proprioceptive_pose_estimator_amd import ops
    depth = _input("grouped")
    s, n, hs, ws = depth.shape[:4]
    group = n if grouped else 0
    rng = np.random.default_rng(17)
    frames = rng.integers(0, 256, (s, n, hs, ws, 3), dtype=np.uint8)
    rgb = ao.neutral_desc(seed=21, erase_thresh=1 << 31, eh_lo=3, eh_hi=10, ew_lo=4, ew_hi=12, group=group)
    step = _mixed_step(rgb, s * n, hs, ws)
    _, rgb_table, _ = ao.augment(frames, rgb, step)
    r, g, b = rgb.pop("fill_rgb")
    state = torch.tensor([step], dtype=torch.int32, device="cuda")
    table = torch.empty(1 + 8 * (group or s * n), dtype=torch.int32, device="cuda")
    ops.augment_frames_u8(torch.from_numpy(frames).cuda(), ops.augment_desc(fill_r=r, fill_g=g, fill_b=b, **rgb), state, params=table)
    assert np.array_equal(table.cpu().numpy(), rgb_table)
    for kw in (dict(occluder_value=5.5), dict(occluder_value=-0.0, **_features(hs, ws)["all"])):
        desc = do.neutral_desc(seed=21, group=group, **kw)
        want = do.augment(depth, desc, step, rgb_params=rgb_table)
        got = _check(depth, desc, step, rgb_params=table, want=want)
        plain = do.augment(depth, desc, step)[0]
        covered = _bits(got) != _bits(plain)
        per_frame = covered.reshape(s * n, -1).any(1)
        assert per_frame.any() and not per_frame.all()                 # some streams erase and some do not
        if grouped:
            assert np.array_equal(covered[0], covered[1]) and np.array_equal(covered[0], covered[2])      # a window keeps its occluder along S
    assert np.array_equal(table.cpu().numpy(), rgb_table)             # the RGB table is read only


def test_refused_descriptors_launch_nothing():
    from rgb_proprioceptive_pose_estimator_amd import ops
    from rgb_proprioceptive_pose_estimator_amd._lib import raw
    depth = _input("tail")
    dev = _device(depth)
    out = torch.full_like(dev, -3.0)
    state = torch.tensor([11], dtype=torch.int32, device="cuda")
    params = torch.full((18,), -5, dtype=torch.int32, device="cuda")
    rgb = torch.zeros(9, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda d, hs=5, ws=7, rgb_params=None, rgb_group=0: raw.rpe_augment_depth_f32(p(dev), p(out), 1, hs, ws, ctypes.byref(d), p(state), p(params),
                                                                                       rgb_params, rgb_group, stream)
    assert call(ops.depth_augment_desc(seed=1, drop_thresh=1 << 31)) == 0                     # a valid call first
    torch.cuda.synchronize()
    assert state.item() == 12 and params[0].item() == 11
    snapshot = out.clone()
    inf, nan = float("inf"), float("nan")
    refused = (dict(n0=-1e-9), dict(n0=nan), dict(n1=inf), dict(n1=-1.0), dict(n2=nan), dict(n2=-inf), dict(q=-1.0), dict(q=inf), dict(q=nan), dict(inv_q=nan),
               dict(inv_q=-2.0), dict(inv_q=inf), dict(lo=1.0, hi=0.5), dict(lo=nan), dict(hi=nan), dict(hole_lo=2, hole_hi=1), dict(hole_hi=5),
               dict(hole_hi=1, hh_lo=0), dict(hole_hi=1, hh_lo=3, hh_hi=2), dict(hole_hi=1, hh_hi=6), dict(hole_hi=1, hw_lo=0), dict(hole_hi=1, hw_lo=3, hw_hi=2),
               dict(hole_hi=1, hw_hi=8), dict(group=-1))
    for kw in refused:
        assert call(ops.depth_augment_desc(**kw)) == 1, kw                                    # RPE_ERR_SHAPE
        assert raw.rpe_last_error().startswith(b"augment_depth_f32:"), kw
    assert call(ops.depth_augment_desc(), hs=1 << 16, ws=1 << 16) == 1                        # Hs * Ws >= 2^32
    assert call(ops.depth_augment_desc(group=1), rgb_params=p(rgb), rgb_group=0) == 1         # the RGB table was drawn with another group
    assert call(ops.depth_augment_desc(hh_lo=0, hh_hi=99, hw_lo=0, hw_hi=-4)) == 0            # hole_hi == 0: the rectangle bounds are not looked at
    torch.cuda.synchronize()
    assert state.item() == 13 and np.array_equal(_bits(out.cpu().numpy()), _bits(depth))      # only the two valid calls ran
    assert not torch.equal(snapshot, out)
    with pytest.raises(ValueError):
        ops.augment_depth_f32(dev, ops.depth_augment_desc(group=1), state, rgb_params=rgb, rgb_group=0)
    with pytest.raises(ValueError):
        ops.augment_depth_f32(dev, ops.depth_augment_desc(), state, params=params[:17])


def _desc_of(aug, hs, ws, group):
    """the oracle's desc of a DepthAugment for one frame size"""
    return do.neutral_desc(**aug.desc_fields(hs, ws, group))


def test_consecutive_calls_wrap_and_resume():
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import DepthAugment
    depth = _input("grouped")
    dev = torch.from_numpy(depth.copy()).cuda()
    for per_frame in (False, True):
        aug = DepthAugment(noise=(0.05, 0.01, 0.002), drop_prob=0.1, holes=(1, 3), hole_scale=(0.2, 0.5), hole_value=-1.0, quant=0.01, clamp=(0.5, 9.0),
                           per_frame=per_frame, seed=12)
        aug.load_state_dict({"seed": 12, "step": 6})
        group = 0 if per_frame else depth.shape[1]
        desc = _desc_of(aug, 16, 24, group)
        assert desc["group"] == group and (desc["hh_lo"], desc["hh_hi"], desc["hw_lo"], desc["hw_hi"]) == (3, 8, 5, 12)
        outs = []
        for step in (6, 7):
            want, want_params = do.augment(depth, desc, step)
            got = aug(dev)
            assert got.data_ptr() != dev.data_ptr() and np.array_equal(_bits(got.cpu().numpy()), _bits(want))
            assert np.array_equal(aug.last_params.cpu().numpy(), want_params) and aug.step == step + 1
            outs.append(_bits(got.cpu().numpy()))
        assert not np.array_equal(outs[0], outs[1]) and aug.state_dict() == {"seed": 12, "step": 8}
        flat = aug(dev.reshape(-1, 16, 24, 1))                        # a 4-D batch draws per frame whatever per_frame says
        assert np.array_equal(_bits(flat.cpu().numpy()).reshape(-1), _bits(do.augment(depth, dict(desc, group=0), 8)[0]).reshape(-1))
        # the counter wraps from 2^32 - 1 to 0
        aug.load_state_dict({"seed": 12, "step": FULL})
        got = aug(dev)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(do.augment(depth, desc, FULL)[0])) and aug.step == 0
        assert np.array_equal(_bits(aug(dev).cpu().numpy()), _bits(do.augment(depth, desc, 0)[0])) and aug.step == 1
        # another object resumes the stream from the state dict
        other = DepthAugment(noise=(0.05, 0.01, 0.002), drop_prob=0.1, holes=(1, 3), hole_scale=(0.2, 0.5), hole_value=-1.0, quant=0.01, clamp=(0.5, 9.0),
                             per_frame=per_frame, seed=99)
        other.load_state_dict(aug.state_dict())
        assert torch.equal(other(dev).view(torch.int32), aug(dev).view(torch.int32)) and other.step == aug.step == 2
    assert np.array_equal(_bits(dev.cpu().numpy()), _bits(depth))


def test_torch_op_equals_the_wrapper():
    from rgb_proprioceptive_pose_estimator_amd import ops
    import rgb_proprioceptive_pose_estimator_amd.torch_ops  # noqa: F401  (registers torch.ops.rpe.*)
    depth = _input("odd")
    dev = torch.from_numpy(depth.copy()).cuda()
    fields = dict(do.neutral_desc(seed=(5 << 32) | 77, **_features(33, 47)["all"]))
    s1, s2 = (torch.tensor([41], dtype=torch.int32, device="cuda") for _ in range(2))
    a = ops.augment_depth_f32(dev, ops.depth_augment_desc(**fields), s1)
    numbers = [77.0, 5.0] + [float(fields[k]) for k in ops.DEPTH_AUGMENT_DESC_FIELDS[1:]]
    b = torch.ops.rpe.augment_depth_f32(dev, numbers, s2)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and s1.item() == 42 and s2.item() == 42
    assert np.array_equal(_bits(a.cpu().numpy()), _bits(do.augment(depth, fields, 41)[0]))
    assert not torch.equal(a.view(torch.int32), dev.view(torch.int32))


def _graph_is_linear(graph):
    """(number of nodes, True iff the captured graph is one chain: n - 1 edges, no node with two successors or two predecessors)"""
    hip = None
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                hip = ctypes.CDLL(line.split()[-1])       # the runtime this process already uses
                break
    assert hip is not None
    handle = ctypes.c_void_p(graph.raw_cuda_graph())
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(handle, None, ctypes.byref(n)) == 0
    e = ctypes.c_size_t(0)
    assert hip.hipGraphGetEdges(handle, None, None, ctypes.byref(e)) == 0
    src, dst = (ctypes.c_void_p * max(1, e.value))(), (ctypes.c_void_p * max(1, e.value))()
    assert hip.hipGraphGetEdges(handle, src, dst, ctypes.byref(e)) == 0
    src, dst = list(src)[:e.value], list(dst)[:e.value]
    return n.value, e.value == n.value - 1 and len(set(src)) == len(src) and len(set(dst)) == len(dst)


def test_captured_call_is_linear_and_draws_fresh_numbers_at_every_replay():
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import DepthAugment
    depth = _input("odd")
    static = torch.from_numpy(depth.copy()).cuda()
    aug = DepthAugment(noise=(0.05, 0.01, 0.002), drop_prob=0.1, holes=(0, 4), hole_value=-1.0, quant=0.01, clamp=(0.5, 9.0), seed=4)
    aug.load_state_dict({"seed": 4, "step": 4})
    out = torch.empty_like(static)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aug(static, out=out)                                           # step 4: the state and table buffers exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        aug(static, out=out)
    assert aug.step == 5                                               # the capture itself ran nothing
    nodes, linear = _graph_is_linear(g)
    assert nodes == 2 and linear                                       # two launches, one after the other: no parallel branches
    desc = _desc_of(aug, 33, 47, 0)
    outs = []
    for step in (5, 6, 7):
        g.replay()
        outs.append(_bits(out.cpu().numpy()))
        assert np.array_equal(outs[-1], _bits(do.augment(depth, desc, step)[0])) and aug.step == step + 1
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])
    assert np.array_equal(_bits(static.cpu().numpy()), _bits(depth))


# -- through the training loop ----------------------------------------------------------------------------------------------------

def _episode_arrays(e=4, t=4, hw=64):
    rng = np.random.default_rng(0)
    def poses():
        q = rng.normal(size=(e, t, 4))
        return np.concatenate([rng.random((e, t, 3)), q / np.linalg.norm(q, axis=-1, keepdims=True)], -1).astype(np.float32)
    return dict(imgs=rng.integers(0, 256, (e, t, hw, hw, 3), dtype=np.uint8), depths=(0.5 + 2.0 * rng.random((e, t, hw, hw, 1))).astype(np.float32),
                true_self=poses(), true_obj=poses())


def _model(seed=3):
    """ResNet-18 trunk, latent 32, with the depth head"""
    from rgb_proprioceptive_pose_estimator_amd import models as M
    torch.manual_seed(seed)
    return M.NaiveObjectStateEstimator("cube", [32], 18, 32, False, (9,), True, False, False, compute_dtype=torch.float32).cuda()


def _criterion():
    from rgb_proprioceptive_pose_estimator_amd import models as M
    crit = lambda: M.PoseDistanceLoss("combined", 1.0, 0.5, 1e-4, "pose")
    return {"x0_loss": crit(), "x1_loss": crit(), "obj_loss": crit(), "val_loss": M.PoseDistanceLoss(mode="val")}


def test_train_with_depth_augmentation(tmp_path):
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import DepthAugment, FrameAugment, RecordedEpisodeDataset, ResidentEpisodeDataset
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import train
    arrays = _episode_arrays()
    path = RecordedEpisodeDataset.save(str(tmp_path / "episodes.npz"), env_name="Lift", **arrays)
    ds = ResidentEpisodeDataset(path, use_depth=True, obj_name="cube")
    model = _model()
    aug = FrameAugment(brightness=0.3, erase_prob=0.5, seed=1)
    daug = DepthAugment(noise=(0.01, 0.01), drop_prob=0.05, holes=(0, 2), quant=0.001, clamp=(0.0, 3.0), share_erase=aug, occluder_value=0.25, seed=1)
    model, best = train(model, ds, _criterion(), FusedAdam(model.parameters(), lr=1e-3), num_epochs=1, num_train_episodes_per_epoch=2,
                        num_val_episodes_per_epoch=2, params={"camera_name": "frontview", "noise_scale": 0.001}, device="cuda:0", save_model=False,
                        logging=False, augment=aug, depth_augment=daug)
    assert np.isfinite(best)
    assert daug.step == 4 and aug.step == 4      # 4 train chunks (horizon 4, one timestep per chunk); the 4 val chunks were not augmented
    assert tuple(daug.last_params.shape) == (1 + 17 * 2,) and daug.last_params[0].item() == 3
    assert np.array_equal(_bits(ds.pool["depths"].cpu().numpy()), _bits(arrays["depths"]))      # the dataset's own depth was not written
    with pytest.raises(ValueError, match="use_depth"):
        from rgb_proprioceptive_pose_estimator_amd import models as M
        plain = M.NaiveObjectStateEstimator("cube", [32], 18, 32, False, (9,), False, False, False, compute_dtype=torch.float32)
        train(plain, ds, _criterion(), None, 1, 1, 1, {}, "cuda:0", depth_augment=DepthAugment())


def test_graphed_train_step_with_the_shared_occluder():
    """(kept single, small and last: DESIGN.md sections 3 and 5 on captured train steps)"""
    from rgb_proprioceptive_pose_estimator_amd.optim import FusedAdam
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import DepthAugment, FrameAugment
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import GraphedTrainStep
    g = torch.Generator().manual_seed(2)
    frames = torch.randint(0, 256, (2, 64, 64, 3), generator=g, dtype=torch.uint8)
    depth = 0.5 + 2.0 * torch.rand(2, 64, 64, 1, generator=g)
    batch = (frames.cuda(), depth.cuda(), torch.randn(2, 7, generator=g).cuda(), torch.randn(2, 7, generator=g).cuda(), None, torch.randn(2, 7, generator=g).cuda())
    model = _model().train()
    aug = FrameAugment(brightness=0.3, noise_std=2.0, erase_prob=1.0, seed=8)
    daug = DepthAugment(noise=(0.01, 0.01, 0.001), drop_prob=0.05, holes=(1, 2), quant=0.001, clamp=(0.0, 3.0), share_erase=aug, occluder_value=0.25, seed=8)
    warmup, n = 2, 2
    step = GraphedTrainStep(model, _criterion(), FusedAdam(model.parameters(), lr=1e-3, capturable=True), True, batch, warmup=warmup, augment=aug,
                            depth_augment=daug)
    assert daug.step == warmup and step.fed[1].data_ptr() != step.static[1].data_ptr()
    for k in range(warmup, warmup + n):
        loss, _, _ = step(batch)
        assert torch.isfinite(loss).item()
    assert daug.step == warmup + n and aug.step == warmup + n
    last = warmup + n - 1
    rgb_desc = dict(aug.desc_fields(64, 64, 0))
    rgb_desc["fill_rgb"] = (rgb_desc.pop("fill_r"), rgb_desc.pop("fill_g"), rgb_desc.pop("fill_b"))
    rgb_table = ao.params_table(ao.neutral_desc(**rgb_desc), 2, 64, 64, last)
    want, want_params = do.augment(depth.numpy(), _desc_of(daug, 64, 64, 0), last, rgb_params=rgb_table)
    assert np.array_equal(_bits(step.fed[1].cpu().numpy()), _bits(want))                      # what the model was fed in the last replay
    assert np.array_equal(daug.last_params.cpu().numpy(), want_params)
    assert (step.fed[1] == 0.25).any().item()                                                 # the occluder is in it
    assert torch.equal(step.static[1].cpu().view(torch.int32), depth.view(torch.int32))       # the static depth is unchanged
