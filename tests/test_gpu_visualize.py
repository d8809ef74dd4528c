"""GPU checks of the layer capture / visualisation feature: the two capture kernels bit for bit, capture_layer against the fp64
oracle on every compute dtype, render_layer against the arrays the reference's own visualize_layer handed to imshow
(tests/golden/visualize_*.npz), the absence of side effects, every model class, and the script."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import pose_oracle as po
from _helpers import CASES, build, load_values
from _helpers_cases import R18
from _visualize_cases import (LAYERS, VIS_CASES, case_inputs, finite_minmax, grid_cols, mosaic, mosaic_t256, mosaic_tiles, oracle_maps,
                              perturbed_state)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _mu():
    from rgb_proprioceptive_pose_estimator_amd.util import model_utils
    return model_utils


def _ops():
    from rgb_proprioceptive_pose_estimator_amd import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- the two kernels
def _activation(dtype, b, h, w, c, seed):
    """random NHWC batch with non-finite values planted in image 1 and one all-NaN channel there"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((b, h, w, c), generator=g) * 3
    x[1, 0, 0, 0] = float("nan")
    x[1, h - 1, w - 1, c - 1] = float("inf")
    x[1, h // 2, w // 2, 1] = float("-inf")
    x[1, 0, w - 1, 2] = float("inf")
    x[1, :, :, 5] = float("nan")
    x[1, 1, 1, 3] = -0.0
    x[:, :, :, 6] = x[:, :, :, 6].abs()       # a channel without negative values ...
    x[:, :, :, 7] = -x[:, :, :, 7].abs()      # ... and one without positive values
    return x.to(dtype).cuda()


PLANE_SHAPES = [(112, 112, 64), (56, 56, 256), (14, 14, 1024), (7, 7, 2048), (7, 7, 512), (5, 7, 72)]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape", PLANE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_planes_kernel_is_exact(dt, shape):
    """No tolerance: the operation has no rounding.  Output bitwise equal to permute().float(), the range == torch's over finite values."""
    ops = _ops()
    h, w, c = shape
    x = _activation(DTYPES[dt], 3, h, w, c, 7 + c)
    want = x.permute(0, 3, 1, 2).float().contiguous()
    fin = torch.isfinite(want)
    lo = torch.where(fin, want, torch.full_like(want, float("inf"))).amin(dim=(2, 3))
    hi = torch.where(fin, want, torch.full_like(want, float("-inf"))).amax(dim=(2, 3))
    planes, minmax = ops.feature_planes(x)
    assert planes.shape == (3, c, h, w) and minmax.shape == (3, c, 2)
    assert torch.equal(_bits(planes), _bits(want))
    assert bool((minmax[..., 0] == lo).all()) and bool((minmax[..., 1] == hi).all())
    assert minmax[1, 5, 0].item() == float("inf") and minmax[1, 5, 1].item() == float("-inf")   # the all-NaN channel
    for i in (1, 2):   # an image index > 0 of the batch
        p1, m1 = ops.feature_planes(x, image=i)
        assert torch.equal(_bits(p1), _bits(want[i]))
        assert bool((m1[:, 0] == lo[i]).all()) and bool((m1[:, 1] == hi[i]).all())


def test_planes_kernel_single_channel_maps():
    """the heads' [B][h*w] fp32 vectors are C = 1 maps: the element-load path"""
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    v = torch.randn((3, 56 * 56), generator=g).cuda()
    planes, minmax = ops.feature_planes(v.view(3, 56, 56, 1))
    assert torch.equal(_bits(planes), _bits(v.view(3, 1, 56, 56)))
    assert torch.equal(minmax[:, 0, 0], v.amin(dim=1)) and torch.equal(minmax[:, 0, 1], v.amax(dim=1))


def _mosaic_planes(c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((c, h, w), generator=g) * torch.logspace(-3, 3, c).view(c, 1, 1) + torch.linspace(-5, 5, c).view(c, 1, 1)
    x[3] = 0.0                      # dead channels
    x[c - 1] = -2.5
    x[4] = torch.relu(x[4])         # min exactly 0
    x[0, 0, 0] = float("nan")
    x[1, h - 1, w - 1] = float("inf")
    x[2, 0, w - 1] = float("-inf")
    x[6] = float("nan")             # a channel without a finite value
    return x


@pytest.mark.parametrize("shape", [(72, 5, 7), (64, 28, 28), (1, 56, 56), (512, 7, 7)], ids=lambda s: "%dx%dx%d" % s)
def test_mosaic_kernel_is_exact(shape):
    """Index image equal to the numpy restatement for EVERY pixel: dead channels, non-finite values, flip_y both ways, gutter 0 and 1,
    C not a square (72 -> 9 columns, last row partial)."""
    ops = _ops()
    c, h, w = shape
    x = _mosaic_planes(c, h, w, 11 + c) if c > 8 else torch.randn((c, h, w), generator=torch.Generator().manual_seed(5))
    xd = x.cuda()
    _, mm = ops.feature_planes(xd.permute(1, 2, 0).contiguous().view(1, h, w, c))
    mm = mm[0].contiguous()
    want_mm = finite_minmax(x.numpy())
    assert np.array_equal(mm.cpu().numpy(), want_mm)
    cols = grid_cols(c)
    assert cols == {72: 9, 64: 8, 1: 1, 512: 23}[c]
    for gutter in (0, 1):
        for flip in (False, True):
            got = ops.feature_mosaic(xd, mm, cols, gutter=gutter, flip_y=flip).cpu().numpy()
            want = mosaic(x.numpy(), want_mm, cols, gutter, flip)
            assert got.shape == want.shape and got.dtype == np.uint8
            bad = np.argwhere(got != want)
            assert bad.size == 0, (gutter, flip, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


# ---------------------------------------------------------------------------------------------------------------- models
_cache = {}


def _case_model(name, dt):
    key = (name, dt)
    if key not in _cache:
        kind, cfg, wseed, _ = VIS_CASES[name]
        model = build(kind, cfg, DTYPES[dt], seq_len=1)
        load_values(model, kind, perturbed_state(kind, cfg, wseed))
        _cache[key] = model.cuda().eval()
    return _cache[key]


def _case_oracle(name, which):
    """which: "f64", "f32", or a 16-bit dtype name (the oracle's storage emulation)"""
    key = ("oracle", name, which)
    if key not in _cache:
        kind, cfg, wseed, _ = VIS_CASES[name]
        img, depth = case_inputs(name)
        sd = perturbed_state(kind, cfg, wseed)
        if which in ("bf16", "f16"):
            po.EMULATE = DTYPES[which]
            try:
                maps = oracle_maps(kind, cfg, sd, img, depth, torch.float32)
            finally:
                po.EMULATE = None
        else:
            maps = oracle_maps(kind, cfg, sd, img, depth, torch.float64 if which == "f64" else torch.float32)
        _cache[key] = {k: v[0].double() for k, v in maps.items()}
    return _cache[key]


def _case_args(name):
    """(img, depth) as the reference's function takes them for the case's model, on the device"""
    kind = VIS_CASES[name][0]
    img, depth = case_inputs(name)
    if kind == "no":
        return img[0].cuda(), depth.cuda()
    return img.cuda(), depth.unsqueeze(0).cuda()


def _captures(name, dt):
    key = ("capture", name, dt)
    if key not in _cache:
        mu = _mu()
        model = _case_model(name, dt)
        img, depth = _case_args(name)
        out = {}
        for layer in LAYERS:
            t = mu.capture_layer(model, layer, img, depth)
            if VIS_CASES[name][0] != "no":
                assert t.shape[0] == 1
                t = t[0]
            assert t.dtype == torch.float32 and t.is_cuda
            out[layer] = t.double().cpu()
        _cache[key] = out
    return _cache[key]


@pytest.mark.parametrize("name", list(VIS_CASES))
def test_capture_fp32_against_fp64_oracle(name):
    """e_gpu = max |capture - m64| / max |m64| <= 3 e_cpu + 1e-6, e_cpu the same figure of the CPU oracle in fp32 (the multiplier
    test_gpu_models.py uses for an fp32 implementation against the CPU-fp32 yardstick; the floor is 16 fp32 ulps of the maximum)."""
    m64, m32, got = _case_oracle(name, "f64"), _case_oracle(name, "f32"), _captures(name, "f32")
    rows = []
    for layer in LAYERS:
        assert got[layer].shape == m64[layer].shape, (layer, got[layer].shape)
        scale = m64[layer].abs().max().item()
        e_gpu = (got[layer] - m64[layer]).abs().max().item() / scale
        e_cpu = (m32[layer] - m64[layer]).abs().max().item() / scale
        rows.append((layer, e_gpu, e_cpu))
        print("capture fp32 %s %-3s e_gpu %.3e e_cpu %.3e" % (name, layer, e_gpu, e_cpu))
    assert got["f0"].min().item() < 0 and got["f9"].min().item() == 0      # conv1 raw; bn1 after the ReLU
    bad = [r for r in rows if not r[1] <= 3 * r[2] + 1e-6]
    assert not bad, bad


@pytest.mark.parametrize("name,dt", [("no_r18", "bf16"), ("no_r18", "f16"), ("tdo_r50", "bf16"), ("tdo_r50", "f16")])
def test_capture_16bit_against_storage_emulation(name, dt):
    """Per layer: relative l2 error against the fp64 oracle <= 1.25 x the error of the oracle's storage emulation + 2e-3
    (the margin where BatchNorm statistics are not chaotic, which holds for inference)."""
    m64, emu, got = _case_oracle(name, "f64"), _case_oracle(name, dt), _captures(name, dt)
    rows = []
    for layer in LAYERS:
        n64 = m64[layer].norm().item()
        e_gpu = (got[layer] - m64[layer]).norm().item() / n64
        e_emu = (emu[layer] - m64[layer]).norm().item() / n64
        rows.append((layer, e_gpu, e_emu))
        print("capture %s %s %-3s l2 e_gpu %.3e e_emu %.3e ratio %.2f" % (dt, name, layer, e_gpu, e_emu, e_gpu / max(e_emu, 1e-30)))
    bad = [r for r in rows if not r[1] <= 1.25 * r[2] + 2e-3]
    assert not bad, bad


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_capture_is_the_widened_engine_buffer(dt):
    """The definition: capture == hooked_feature, widened, bit for bit."""
    mu = _mu()
    model = _case_model("no_r18", dt)
    img, depth = _case_args("no_r18")
    trunk = model.trunk
    for n in (9, 1, 2, 3, 4):
        got = mu.capture_layer(model, "f%d" % n, img)
        buf = trunk._active.hooked_feature(n)
        assert buf.dtype == DTYPES[dt]
        assert torch.equal(_bits(got), _bits(buf[0].permute(2, 0, 1).float()))
    # conv1's raw output: with the model keeping it (as a conv1 hook makes it), the buffer survives the capture
    assert not trunk.keep_stem_raw
    trunk.keep_stem_raw = True
    try:
        got = mu.capture_layer(model, "f0", img)
        assert torch.equal(_bits(got), _bits(trunk._active.hooked_feature(0)[0].permute(2, 0, 1).float()))
        kept = got.clone()
    finally:
        trunk.keep_stem_raw = False
    assert torch.equal(_bits(mu.capture_layer(model, "f0", img)), _bits(kept))   # ... and the one-forward switch gives the same tensor
    assert not trunk.keep_stem_raw


def _fixture_planes(gold, layer):
    if layer + "_whole" in gold:
        return gold[layer + "_whole"], np.arange(gold[layer + "_whole"].shape[0])
    return gold[layer + "_chans"], gold[layer + "_chan_idx"]


@pytest.mark.parametrize("name", list(VIS_CASES))
def test_render_against_reference_imshow_arrays(name, golden_dir):
    """fp32 path: the tiles of the 's' / 'm' picture against the mosaic restatement applied to the arrays the reference handed to
    imshow.  With E = max |capture - fixture| of the layer, v, lo and hi each move t by at most E / (hi - lo): a pixel may differ, by
    one index step, only where the fixture's t * 256 lies within 256 * 3E / (hi - lo) of an integer; channels constant in the fixture
    are all 0."""
    mu = _mu()
    gold = np.load(os.path.join(golden_dir, "visualize_%s.npz" % name))
    model = _case_model(name, "f32")
    img, depth = _case_args(name)
    got = _captures(name, "f32")
    table = mu.colour_table()
    for layer in LAYERS:
        planes, chans = _fixture_planes(gold, layer)
        c, h, w = (int(v) for v in gold[layer + "_shape"])
        cap = got[layer].numpy()[chans]
        E = float(np.abs(cap - planes.astype(np.float64)).max())
        mm = np.stack([gold[layer + "_cmin"][chans], gold[layer + "_cmax"][chans]], axis=1).astype(np.float32)
        assert np.array_equal(mm, finite_minmax(planes))
        want = mosaic_tiles(planes, mm)
        t256 = mosaic_t256(planes, mm).astype(np.float64)
        with np.errstate(all="ignore"):
            slack = 256.0 * 3.0 * E / (mm[:, 1].astype(np.float64) - mm[:, 0].astype(np.float64))
            near = np.abs(t256 - np.round(t256)) <= slack[:, None, None]
        for mode in ("m", "s"):
            idx, (cc, hh, ww, cols) = mu.layer_index_image(model, layer + mode, img, depth, gutter=1, flip_y=True)
            assert (cc, hh, ww, cols) == ((c, h, w, grid_cols(c)) if mode == "m" else (1, h, w, 1))
            rows = -(-cc // cols)
            assert idx.shape == (rows * (h + 1) - 1, cols * (w + 1) - 1)
            n_close = n_diff = 0
            for k, ch in enumerate(chans):
                if mode == "s" and ch != 0:
                    continue
                r0, c0 = (int(ch) // cols) * (h + 1), (int(ch) % cols) * (w + 1)
                tile = idx[r0:r0 + h, c0:c0 + w][::-1].astype(np.int64)   # (row 0 is drawn at the bottom)
                if mm[k, 0] == mm[k, 1]:
                    assert not tile.any(), (layer, mode, int(ch))
                    continue
                d = tile - want[k].astype(np.int64)
                assert np.abs(d).max() <= 1, (layer, mode, int(ch), np.abs(d).max())
                assert not (d != 0)[~near[k]].any(), (layer, mode, int(ch), int(((d != 0) & ~near[k]).sum()), E, slack[k])
                n_diff += int((d != 0).sum())
                n_close += int(near[k].sum())
            print("render %s %s%s E %.2e: %d pixels differ by one step (%d within the slack)" % (name, layer, mode, E, n_diff, n_close))
        rgb = mu.render_layer(model, layer + "s", img, depth)
        assert rgb.shape == (h, w, 3) and rgb.dtype == np.uint8 and np.array_equal(rgb, table[idx])
    # the 'm' picture in colour: white gutters, tiles through the colour table
    rgb = mu.render_layer(model, "f9m", img, depth)
    idx, _ = mu.layer_index_image(model, "f9m", img, depth)
    assert rgb.shape == (8 * 113 - 1, 8 * 113 - 1, 3) and (rgb[112] == 255).all() and (rgb[:, 112] == 255).all()
    assert np.array_equal(rgb[:112, :112], table[idx[:112, :112]])
    rgb0 = mu.render_layer(model, "f9m", img, depth, gutter=0, flip_y=False)
    assert rgb0.shape == (8 * 112, 8 * 112, 3) and np.array_equal(rgb0[:112, :112], rgb[:112, :112][::-1])


# ---------------------------------------------------------------------------------------------------------------- side effects
def _state_bits(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _same_state(a, b):
    return all(torch.equal(a[k], b[k]) for k in a) and a.keys() == b.keys()


EVERY_KIND = ("f0", "f9", "f2", "f4", "a0", "d0")


def test_capture_has_no_side_effects_on_inference():
    """Eval outputs, a rollout frame (eager and as a captured graph), the carried (h, c), BN running statistics and
    num_batches_tracked are bit for bit what they are without a capture -- including f0 on a model without a conv1 hook, whose
    capture switches the packed stem weight for one forward."""
    from rgb_proprioceptive_pose_estimator_amd.util.learn_utils import GraphedRolloutFrame
    mu = _mu()
    model = _case_model("tdo_r50", "bf16")
    img, depth = _case_args("tdo_r50")
    b = po.synth_batch((1, 1), 77, with_depth=True)
    x0bar = b["x0bar"].cuda()
    before = _state_bits(model)

    def capture_all():
        for layer in EVERY_KIND:
            mu.capture_layer(model, layer, img, depth)

    with torch.no_grad():
        model.rollout = False
        out0 = model(img.unsqueeze(0), depth, x0bar).clone()
        model.rollout = True
        model.reset_initial_state(1)
        f1 = model(img.unsqueeze(0), depth, x0bar).clone()
        f2 = model(img.unsqueeze(0), depth, x0bar).clone()            # control: two frames, state carried
        model.reset_initial_state(1)
        g1 = model(img.unsqueeze(0), depth, x0bar).clone()
        carried = {k: (h.clone(), c.clone()) for k, (h, c) in model._carried.items()}
        capture_all()
        assert model.rollout and not model.training
        assert all(torch.equal(h, model._carried[k][0]) and torch.equal(c, model._carried[k][1]) for k, (h, c) in carried.items())
        g2 = model(img.unsqueeze(0), depth, x0bar).clone()
        assert torch.equal(g1, f1) and torch.equal(g2, f2)
        model.rollout = False
        capture_all()
        assert torch.equal(model(img.unsqueeze(0), depth, x0bar), out0)
        # the captured frame replays the packed weights as they stand: a capture must leave them as it found them
        model.rollout = True
        model.reset_initial_state(1)
        frame = GraphedRolloutFrame(model, img.unsqueeze(0), depth, x0bar, warmup=1, calibrate=0)
        assert frame.replaying
        model.reset_initial_state(1)
        r1 = frame(img.unsqueeze(0), depth, x0bar).clone()
        capture_all()
        model.reset_initial_state(1)
        r2 = frame(img.unsqueeze(0), depth, x0bar).clone()
        assert torch.equal(r1, r2) and torch.equal(r1, f1)
        model.rollout = False
    assert _same_state(before, _state_bits(model))
    assert not any(m._forward_hooks for m in model.modules())


def test_training_step_after_capture_has_the_same_gradients():
    """(use_depth=False: the depth head's two InstanceNorm scalars are summed with atomics)"""
    mu = _mu()
    cfg, lead, wseed, dseed = R18
    model = build("no", cfg, torch.bfloat16)
    load_values(model, "no", po.make_state("no", cfg, wseed))
    model.cuda()
    b = po.synth_batch(lead, dseed)
    img, x0bar, obj = b["img"].cuda(), b["x0bar"].cuda(), b["obj"].cuda()

    def step():
        model.train()
        model.zero_grad(set_to_none=False)
        out = model(img, None, x0bar)
        ((out - obj) ** 2).sum().backward()
        torch.cuda.synchronize()
        return [None if p.grad is None else p.grad.detach().clone() for p in model.parameters()]

    def same(a, c):
        return len(a) == len(c) and all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, c))

    g0 = step()
    g1 = step()
    assert same(g0, g1) and any(g is not None and g.abs().sum().item() > 0 for g in g1)   # the premise: the step itself is reproducible
    nbt = model.state_dict()["feature_net.module.bn1.num_batches_tracked"].item()
    for layer in ("f0", "f9", "f3", "a0"):
        mu.capture_layer(model, layer, img[0])
    assert not model.training
    assert model.state_dict()["feature_net.module.bn1.num_batches_tracked"].item() == nbt
    g2 = step()
    assert same(g1, g2)


# ---------------------------------------------------------------------------------------------------------------- every model class
def _any_model(kind, depth):
    from rgb_proprioceptive_pose_estimator_amd import models as M
    dt = torch.bfloat16
    if kind == "n":
        return M.NaiveEndEffectorStateEstimator([32], [32], depth, 64, False, compute_dtype=dt)
    if kind == "no":   # with proprioception: the reference's visualize_layer cannot run this one
        return M.NaiveObjectStateEstimator("cube", [32], depth, 64, False, (9,), True, False, False, compute_dtype=dt)
    if kind == "td":
        return M.TemporallyDependentStateEstimator(32, 32, depth, 64, 2, 0.1, False, (9,), True, False, compute_dtype=dt)
    if kind == "tdo":
        return M.TemporallyDependentObjectStateEstimator("hammer", 32, depth, 64, 2, 0.1, False, (9,), True, False, False, compute_dtype=dt)
    return M.TemporallyDependentObjectStateEstimatorV2("robot1_eef", 32, 8, depth, 64, 2, 0.1, False, (9,), True, False, compute_dtype=dt)


@pytest.mark.parametrize("depth", [18, 50])
@pytest.mark.parametrize("kind", list(CASES))
def test_every_model_class_and_batches(kind, depth):
    """All five classes, both block types; a batch of 4 images == four single captures, bit for bit; sequence-shaped input is
    flattened as the models flatten it."""
    mu = _mu()
    torch.manual_seed(5)
    model = _any_model(kind, depth).cuda()
    b = po.synth_batch((2, 2), 900 + depth, with_depth=True)
    seq = kind in ("td", "tdo", "tdo_v2")
    img = b["img"].cuda() if seq else b["img"].reshape(4, 3, 224, 224).cuda()
    dep = b["depth"].cuda() if seq else b["depth"].reshape(4, 1, 224, 224).cuda()
    flat_img, flat_dep = img.reshape(4, 3, 224, 224), dep.reshape(4, 1, 224, 224)
    exp = 1 if depth == 18 else 4
    shapes = {"f9": (64, 112, 112), "f4": (512 * exp, 7, 7), "a0": (1, 56, 56), "d0": (1, 56, 56)}
    for layer in ("f9", "f4") if kind == "n" else ("f9", "f4", "a0", "d0"):
        whole = mu.capture_layer(model, layer + "m", img, dep)
        assert whole.shape == (4,) + shapes[layer] and whole.dtype == torch.float32
        for i in range(4):
            one = mu.capture_layer(model, layer, flat_img[i], flat_dep[i:i + 1])
            assert one.shape == shapes[layer]
            assert torch.equal(_bits(one), _bits(whole[i])), (kind, depth, layer, i)
    if kind == "n":
        with pytest.raises(ValueError):
            mu.capture_layer(model, "a0", img, dep)


# ---------------------------------------------------------------------------------------------------------------- the script
def test_visualize_features_script_writes_the_rendered_pngs(tmp_path):
    from PIL import Image
    from rgb_proprioceptive_pose_estimator_amd.scripts import visualize_features as vf
    from rgb_proprioceptive_pose_estimator_amd.scripts.train_model import DTYPES as SCRIPT_DTYPES, build_model
    mu = _mu()
    rng = np.random.default_rng(4)
    frames = rng.integers(0, 256, (2, 256, 256, 3), dtype=np.uint8)
    fpath, out = str(tmp_path / "frames.npy"), str(tmp_path / "out")
    np.save(fpath, frames)
    argv = ["--model", "no", "--obj_name", "cube", "--latent_dim", "64", "--hidden_dim", "32", "--dtype", "f32", "--frames", fpath, "--frame", "1",
            "--layer", "f9m", "--layer", "a0s", "--out", out]
    env = dict(os.environ, MPLBACKEND="Agg")
    subprocess.run([sys.executable, os.path.join(ROOT, "rgb-proprioceptive-pose-estimator_amd", "scripts", "visualize_features.py")] + argv,
                   check=True, timeout=300, env=env, cwd=str(tmp_path))
    assert sorted(os.listdir(out)) == ["a0s.png", "f9m.png"]
    # the same model in this process (the script seeds torch with 3 before it builds)
    args = vf.build_vis_parser().parse_args(argv)
    torch.manual_seed(3)
    model = build_model(args, SCRIPT_DTYPES[args.dtype]).cuda().eval()
    frame = torch.from_numpy(frames[1]).cuda()
    for layer, size in (("f9m", (8 * 113 - 1, 8 * 113 - 1)), ("a0s", (56, 56))):
        png = np.asarray(Image.open(os.path.join(out, layer + ".png")).convert("RGB"))
        assert png.shape == size + (3,)
        assert np.array_equal(png, mu.render_layer(model, layer, frame))
