"""The compact data gradient of a 1x1 / stride-2 projection shortcut (rpe_conv1x1s2_dgrad_compact) and the subsampled addend that
reads it back (rpe_conv2d_dgrad_sub, rpe_conv2d_dgrad_bn_sub, rpe_conv1x1_dgrad_kcat_y_sub), through the C ABI on seeded inputs.

Shapes (B, H, W): (3, 6, 6) = 108 output rows, one partial 128-row tile with image boundaries inside it; (5, 10, 6) = 300 rows, three
tiles with a tail and H != W (a swapped division shows).  Channels: Cin 128 (a whole column tile) and 72 (a multiple of 8 only),
Cout 64 and 128.

1. compact == the rows (b, 2h', 2w') of the zero-filled gradient: both within the fp64 bound of tests/_bounds.py, every other row of
   the zero-filled one exactly zero; whether the two are bit-identical is printed (BITS ...), not asserted.
2. every epilogue form the engine uses, once with the compact addend and once, through the unchanged call, with the same values
   scattered into a zero-filled full-resolution addend: outputs and partial sums bit-identical (the same kernel adding +0 at the odd
   pixels either way; no tolerance, no excluded element).
3. engine: a ResNet-50 step by default and with all-zero dense hook gradients on layers 1-3 (which force the zero-filled path and add
   nothing): every gradient tensor bit-identical if the compact GEMMs are at the three shortcut shapes of that step, within the path's
   bar otherwise.  fp32 on 4 images of 64 x 64, and fp32 / bf16 on 16 images of 256 x 256, the smallest step at which the engine takes
   the compact path in all three entry blocks (it keeps the zero-filled launch while that has fewer workgroups than the chip has CUs).
4. odd dims: the zero-filled call still runs and is right; the compact entry points refuse them with the shape error."""
import ctypes

import pytest
import torch

import _bounds as B

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from rgb_proprioceptive_pose_estimator_amd import ops
    from rgb_proprioceptive_pose_estimator_amd._lib import RpeError, lib

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
SHAPES = [(3, 6, 6), (5, 10, 6)]
CHANNELS = [(128, 64), (72, 128)]   # (Cin, Cout)


def bits(t):
    """the stored bit patterns (so that -0 != +0 and NaNs compare)"""
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def operands(shape, ci, co, dtype, seed):
    """dy [B, H/2, W/2, Co] and the data-gradient weight copy [Ci, 1, 1, Co] of a 1x1 / stride-2 conv over [B, H, W, Ci]"""
    b, h, w = shape
    g = torch.Generator().manual_seed(seed)
    dy = (torch.randn(b, h // 2, w // 2, co, generator=g) + 0.1).to(dtype).to(DEV)
    wd = (torch.randn(ci, 1, 1, co, generator=g) / co ** 0.5).to(dtype).to(DEV)
    return dy, wd


def scatter(compact, shape):
    """the compact tensor's values at the even pixels of a zero-filled [B, H, W, C]"""
    b, h, w = shape
    full = torch.zeros(b, h, w, compact.shape[-1], dtype=compact.dtype, device=compact.device)
    full[:, ::2, ::2] = compact
    return full


def compact_pair(shape, ci, co, dtype, seed):
    """-> (compact, zero-filled, fp64 reference) of the shortcut's data gradient"""
    b, h, w = shape
    dy, wd = operands(shape, ci, co, dtype, seed)
    comp = ops.conv1x1s2_dgrad_compact(dy, wd, (b, h, w, ci))
    full = ops.conv2d_dgrad(dy, wd, (b, h, w, ci), 2, 0)
    ref = B.gemm_ref(dy.reshape(-1, co), wd.reshape(ci, co))
    return comp, full, ref


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("ci,co", CHANNELS)
def test_compact_dgrad_is_the_even_rows_of_the_zero_filled_one(dtype, shape, ci, co):
    b, h, w = shape
    comp, full, ref = compact_pair(shape, ci, co, dtype, 7 * sum(shape) + ci + co)
    assert comp.shape == (b, h // 2, w // 2, ci)
    bnd = B.bound(ref, dtype)
    label = "compact dgrad %s %s ci%d co%d" % (str(dtype).split(".")[-1], shape, ci, co)
    B.assert_within(comp.reshape(-1, ci), ref.acc, bnd, label, layout="rc")
    B.assert_rounds_once(comp.reshape(-1, ci), ref.acc, dtype, label, bnd)
    kept = full[:, ::2, ::2].contiguous()
    B.assert_within(kept.reshape(-1, ci), ref.acc, bnd, label + " (zero-filled, even pixels)", layout="rc")
    rest = full.clone()
    rest[:, ::2, ::2] = 0
    assert int((bits(rest) != 0).sum()) == 0, "the zero-filled gradient is not exactly +0 off the even pixels"
    print("BITS  %-48s %s" % (label, "identical" if same_bits(comp, kept) else "DIFFERENT (max |d| %.3g)" % float((comp.float() - kept.float()).abs().max())))


FORMS = ["plain", "bn_mask_y", "bn_aout_y", "bn_mask_noy", "kcat_y_bn", "kcat_y"]   # BN-backward modes 0, 4, 1, 5, 4, 0


def run_form(form, sub, shape, ci, co, dtype, seed):
    """one conv1 data gradient of the entry block: dy [B, H, W, Co] of the 1x1 / stride-1 conv, the shortcut gradient as its addend
    (compact with sub, scattered into zeros without) -> the tensors the launch leaves behind"""
    b, h, w = shape
    rows = b * h * w
    g = torch.Generator().manual_seed(seed)
    dy = (torch.randn(b, h, w, co, generator=g) + 0.1).to(dtype).to(DEV)
    wd = (torch.randn(ci, 1, 1, co, generator=g) / co ** 0.5).to(dtype).to(DEV)
    compact = torch.randn(b, h // 2, w // 2, ci, generator=g).to(dtype).to(DEV)
    addend = compact if sub else scatter(compact, shape)
    y = (torch.randn(b, h, w, ci, generator=g) * 1.2).to(dtype).to(DEV)
    mean = (torch.randn(ci, generator=g) * 0.1).to(DEV)
    invstd = (0.5 + torch.rand(ci, generator=g)).to(DEV)
    mask = torch.randint(0, 256, (rows, ci // 8), generator=g, dtype=torch.uint8).to(DEV)
    if form == "plain":
        return (ops.conv2d_dgrad(dy, wd, (b, h, w, ci), 1, 0, addend=addend, sub_addend=sub),)
    if form == "bn_mask_y":
        return ops.conv2d_dgrad_bn(dy, wd, (b, h, w, ci), 1, 0, y, mean, invstd, addend=addend, a_mask=mask, sub_addend=sub)
    if form == "bn_aout_y":   # (the ReLU mask from the layer's output itself: the engines without packed masks)
        a_out = torch.randn(b, h, w, ci, generator=g).to(dtype).to(DEV)
        return ops.conv2d_dgrad_bn(dy, wd, (b, h, w, ci), 1, 0, y, mean, invstd, a_out=a_out, addend=addend, sub_addend=sub)
    if form == "bn_mask_noy":
        return ops.conv2d_dgrad_bn(dy, wd, (b, h, w, ci), 1, 0, None, None, None, addend=addend, a_mask=mask, sub_addend=sub)
    y1 = torch.randn(b, h, w, co, generator=g).to(dtype).to(DEV)
    wk = (torch.randn(ci, 2 * co, generator=g) / co ** 0.5).to(dtype).to(DEV)
    bias = torch.randn(ci, generator=g).to(DEV)
    if form == "kcat_y":
        return (ops.conv1x1_dgrad_kcat_y(dy, y1, wk, bias, ci, addend=addend, sub_addend=sub),)
    return ops.conv1x1_dgrad_kcat_y(dy, y1, wk, bias, ci, addend=addend, bn=dict(y=y, mean=mean, invstd=invstd, a_mask=mask), sub_addend=sub)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("ci,co", CHANNELS)
@pytest.mark.parametrize("form", FORMS)
def test_subsampled_addend_is_bitwise_the_scattered_one(form, dtype, shape, ci, co):
    if form == "bn_mask_noy" and dtype == torch.float32:
        # (rpe_conv2d_dgrad_bn refuses y = NULL for fp32 in both forms: the sum-dz-only epilogue exists for the 16-bit types alone)
        with pytest.raises(RpeError):
            run_form(form, False, shape, ci, co, dtype, 5)
        with pytest.raises(RpeError):
            run_form(form, True, shape, ci, co, dtype, 5)
        return
    seed = 11 * sum(shape) + ci + co
    got = run_form(form, True, shape, ci, co, dtype, seed)
    want = run_form(form, False, shape, ci, co, dtype, seed)
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for name, a, c in zip(("output", "stats_part"), got, want):
        assert torch.isfinite(c.float()).all(), name
        assert same_bits(a, c), "%s of %s differs: %d of %d elements" % (name, form, int((bits(a) != bits(c)).sum()), a.numel())


LATENT = 32


def engine_step(zero_hooks, dtype, batch, side):
    from rgb_proprioceptive_pose_estimator_amd.engine import ResNet50Trunk
    from rgb_proprioceptive_pose_estimator_amd.params import ParamArena

    torch.manual_seed(4321)
    trunk = ResNet50Trunk(LATENT, compute_dtype=dtype, depth=50).cuda().train()
    trunk.ensure_layout()
    arena = ParamArena(trunk)
    g = torch.Generator().manual_seed(77)
    img = torch.randn(batch, 3, side, side, generator=g).cuda()
    d_feat = (torch.randn(batch, ops.pad4(LATENT), generator=g) / batch).cuda()
    feat = torch.zeros(batch, ops.pad4(LATENT), device="cuda")
    plan = trunk.run(img, feat, True, pre_forward=lambda p: lib.rpe_resnet50_profile(p.handle, 1))
    hooks = []
    if zero_hooks:
        for layer in (1, 2, 3):
            hooks.append(torch.zeros_like(plan.hooked_feature(layer)))
            plan.set_hook_grad(layer, hooks[-1])
    plan.backward(d_feat, False)
    torch.cuda.synchronize()
    # zero-filled shortcut gradients of this step: the data-gradient launches (role 1) in conv mode (MODE 1) without a BN epilogue;
    # launches with a compact addend carry ",sub" in their symbol
    buf = ctypes.create_string_buffer(1 << 16)
    nbytes = lib.rpe_resnet50_profile_kernels(plan.handle, buf, len(buf))
    launches = {}
    for line in buf.raw[:nbytes].decode().splitlines():
        name, cnt = line.split(";")[:2]
        launches[name] = launches.get(name, 0) + int(cnt)
    zero_filled = sub = 0
    for name, cnt in launches.items():
        f = name.rstrip(">").split(",")
        if name.startswith("nt_kernel<") and f[4] == "1" and f[6] == "1" and f[7] == "0":
            zero_filled += cnt
        if name.startswith("nt_kernel<") and f[-1] == "sub":
            sub += cnt
    lib.rpe_resnet50_profile(plan.handle, 0)
    _, params, _, _ = trunk._ordered()
    names = {id(p): n for n, p in trunk.named_parameters()}
    census = {"workspace_bytes": int(lib.rpe_resnet50_workspace_bytes(plan.handle)), "launches": dict(sorted(launches.items()))}
    return feat.clone(), [(names[id(p)], p._rpe_grad.clone()) for p in params], (zero_filled, sub), census


# (dtype, images, image side, bar where the GEMMs are not bit-identical).  4 images of 64 x 64: the step the issue names -- there the
# engine keeps the zero-filled launches by default (fewer workgroups than CUs, engine.hip compact_min_tiles), so both runs take one path.
# 16 images of 256 x 256: the zero-filled shortcut gradients of layers 2 / 3 / 4 are 1024 / 512 / 256 workgroups, all three entry
# blocks take the compact path by default -- once through the fp32 epilogues, once through the 16-bit ones (mask bits, sum dz only).
ENGINE_CASES = [(torch.float32, 4, 64, 1e-4), (torch.float32, 16, 256, 1e-4), (torch.bfloat16, 16, 256, 2e-2)]


@pytest.mark.parametrize("dtype,batch,side,bar", ENGINE_CASES, ids=lambda v: str(v))
def test_engine_gradients_do_not_depend_on_the_shortcut_form(dtype, batch, side, bar):
    exact = True
    for div, ci, co in ((4, 256, 512), (8, 512, 1024), (16, 1024, 2048)):   # the entry blocks' shortcuts: input side, Cin, Cout
        comp, full, _ = compact_pair((batch, side // div, side // div), ci, co, dtype, side + ci)
        exact = exact and same_bits(comp, full[:, ::2, ::2].contiguous())
    print("BITS  engine shortcut GEMMs (%s, %d x %d^2): %s" % (str(dtype).split(".")[-1], batch, side, "identical" if exact else "different"))
    feat_a, grads_a, zf_a, _ = engine_step(False, dtype, batch, side)
    feat_b, grads_b, zf_b, _ = engine_step(True, dtype, batch, side)
    # (zero-filled shortcut gradients, conv1 data gradients with a compact addend): the two runs really took the two forms
    assert zf_b == (3, 0) and zf_a == ((0, 3) if batch * side >= 16 * 256 else (3, 0)), (zf_a, zf_b)
    assert same_bits(feat_a, feat_b)
    worst = 0.0
    for (name, a), (_, c) in zip(grads_a, grads_b):
        assert torch.isfinite(a).all() and torch.isfinite(c).all(), name
        rel = float((a - c).abs().max() / c.abs().max().clamp_min(1e-30))
        worst = max(worst, rel)
        if exact:
            assert same_bits(a, c), "%s: compact and zero-filled paths differ (rel %.3g)" % (name, rel)
        else:
            assert rel < bar, "%s: rel %.3g" % (name, rel)
    print("ENGINE worst relative difference over %d gradient tensors: %.3g" % (len(grads_a), worst))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_odd_dims_keep_the_zero_filled_path(dtype):
    b, h, w, ci, co = 2, 7, 6, 72, 64
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    g = torch.Generator().manual_seed(31)
    dy = (torch.randn(b, ho, wo, co, generator=g) + 0.1).to(dtype).to(DEV)
    wd = (torch.randn(ci, 1, 1, co, generator=g) / co ** 0.5).to(dtype).to(DEV)
    full = ops.conv2d_dgrad(dy, wd, (b, h, w, ci), 2, 0)
    ref = B.gemm_ref(dy.reshape(-1, co), wd.reshape(ci, co))
    kept = full[:, ::2, ::2].contiguous()
    assert kept.shape == (b, ho, wo, ci)
    B.assert_within(kept.reshape(-1, ci), ref.acc, B.bound(ref, dtype), "zero-filled dgrad, odd dims %s" % str(dtype).split(".")[-1], layout="rc")
    rest = full.clone()
    rest[:, ::2, ::2] = 0
    assert int((bits(rest) != 0).sum()) == 0
    with pytest.raises(RpeError, match=r"failed \(1\)"):   # RPE_ERR_SHAPE
        ops.conv1x1s2_dgrad_compact(dy, wd, (b, h, w, ci))
    # ... and a compact addend over odd dims has no row map
    dy1 = torch.zeros(b, h, w, co, dtype=dtype, device=DEV)
    with pytest.raises(RpeError, match=r"failed \(1\)"):
        ops.conv2d_dgrad(dy1, wd, (b, h, w, ci), 1, 0, addend=torch.zeros(b, ho, wo, ci, dtype=dtype, device=DEV), sub_addend=True)
    # ... nor is there a compact addend for the epilogues no entry block runs (mask recomputed from y: scale / shift; no mask)
    y6 = torch.zeros(b, 6, 6, ci, dtype=dtype, device=DEV)
    vec = torch.ones(ci, device=DEV)
    for kw in (dict(scale=vec, shift=vec), dict()):
        with pytest.raises(RpeError, match=r"failed \(1\)"):
            ops.conv2d_dgrad_bn(torch.zeros(b, 6, 6, co, dtype=dtype, device=DEV), wd, (b, 6, 6, ci), 1, 0, y6, vec, vec,
                                addend=torch.zeros(b, 3, 3, ci, dtype=dtype, device=DEV), sub_addend=True, **kw)
    # nor does a stride-1 conv have a compact gradient
    with pytest.raises(RpeError, match=r"failed \(1\)"):
        d = ops.conv_desc((b, 6, 6, ci), co, 1, 1, 0)
        dy6, dx3 = torch.zeros(b, 6, 6, co, dtype=dtype, device=DEV), torch.zeros(b, 3, 3, ci, dtype=dtype, device=DEV)
        ops.lib.rpe_conv1x1s2_dgrad_compact(ctypes.byref(d), ops.dtype_code(dy6), ops._p(dy6), ops._p(wd), ops._p(dx3), ops._stream())
