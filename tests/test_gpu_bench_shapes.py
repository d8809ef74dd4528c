"""Every distinct conv of the benchmarked ResNet-50 train step (256 images at 224 x 224) and the ResNet-18 BasicBlock convs that
ResNet-50 lacks, through the entry points the engine uses, checked element by element against fp64 (tests/_bounds.py): forward
with the BN partial sums, data gradient with addend, deterministic weight gradient (the halo form for the 3x3 / stride-1 convs of
layers 1-2 in the 16-bit types), Gram + BN statistics + the fused 1x1 forward for conv3 of layers 1-2, and the stem.  These are
the launch configurations of the benchmark itself: split plans that depend on M, XCD remap over thousands of tiles, halo tiles
crossing 256 image borders, ring wrap-around on 56-wide maps.  bf16 at batch 256; fp16 and fp32 at 32.

The table comes from the model's own conv modules (channels, kernel, stride, padding), spatial sizes tracked from 224."""
import pytest
import torch
import torch.nn.functional as F

import _bounds as B

DEV = "cuda"
RUNS = [(torch.bfloat16, 256), (torch.float16, 32), (torch.float32, 32)]


def conv_table(depth):
    """[(name, Ci, Co, k, stride, pad, H_in)] of the trunk's convs after the stem (first occurrence of each distinct one)."""
    from rgb_proprioceptive_pose_estimator_amd.engine import ResNet50Trunk
    t = ResNet50Trunk(10, depth=depth)
    out, seen = [], set()
    h = 224 // 4                                                    # stem (stride 2) + max pool (stride 2)
    for li in range(1, 5):
        for bi, blk in enumerate(getattr(t, "layer%d" % li)):
            hin = h
            convs = [("conv1", blk.conv1), ("conv2", blk.conv2)] + ([("conv3", blk.conv3)] if hasattr(blk, "conv3") else [])
            if hasattr(blk, "downsample"):
                convs.append(("downsample", blk.downsample[0]))
            cur = hin
            for name, c in convs:
                hi = hin if name == "downsample" else cur
                key = (c.in_channels, c.out_channels, c.kernel_size[0], c.stride[0], c.padding[0], hi)
                if key not in seen:
                    seen.add(key)
                    out.append(("r%d.layer%d.%d.%s" % (depth, li, bi, name),) + key)
                if name != "downsample":
                    cur = (hi + 2 * c.padding[0] - c.kernel_size[0]) // c.stride[0] + 1
            h = cur
    return out


R50 = conv_table(50)
R18_EXTRA = [c for c in conv_table(18) if c[1:] not in {r[1:] for r in R50}]
TABLE = R50 + R18_EXTRA


def test_table_covers_every_trunk_conv():
    """CPU: every trunk conv weight shape of ResNet-50 and ResNet-18 (stem aside) appears in the table, with its own stride and
    padding; ~23 + 6 entries."""
    from rgb_proprioceptive_pose_estimator_amd.engine import ResNet50Trunk
    shapes = {(c[2], c[1], c[3], c[3]) for c in TABLE}
    for depth in (50, 18):
        t = ResNet50Trunk(10, depth=depth)
        for name, m in t.named_modules():
            if isinstance(m, torch.nn.Conv2d) and name != "conv1":
                assert tuple(m.weight.shape) in shapes, (depth, name)
                assert any(c[1:6] == (m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], m.padding[0]) for c in TABLE), name
    assert 20 <= len(R50) <= 26 and 4 <= len(R18_EXTRA) <= 8, (len(R50), len(R18_EXTRA))


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _record(label, ops):
    k = ops.last_kernel_name()
    print("KERNEL %-52s %s" % (label, k))
    return k


def _within(got, r, dtype, label, out=None, gain=1.0, epi=None, layout=None):
    ref = r.acc if out is None else out
    bnd = B.bound(r, dtype, out=ref, gain=gain, epi=epi)
    B.assert_within(got, ref, bnd, label, layout)
    B.assert_unbiased(got, ref, dtype, label, bnd)
    B.assert_rounds_once(got, ref, dtype, label, bnd)


def _stats(st, r, label):
    B.assert_stats(st, r, label)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,batch", RUNS, ids=["bf16x256", "f16x32", "f32x32"])
@pytest.mark.parametrize("cfg", TABLE, ids=[c[0] for c in TABLE])
def test_bench_conv(cfg, dtype, batch):
    from rgb_proprioceptive_pose_estimator_amd import ops
    name, ci, co, k, s, p, h = cfg
    tag = "%s %s x%d" % (name, str(dtype)[6:], batch)
    g = torch.Generator(device=DEV).manual_seed(ci * 7 + co + k * 13 + s + h)
    x = torch.randn(batch, ci, h, h, generator=g, device=DEV).to(dtype)
    w = (torch.randn(co, ci, k, k, generator=g, device=DEV) / (ci * k * k) ** 0.5).to(dtype)
    ho = (h + 2 * p - k) // s + 1
    dy = torch.randn(batch, co, ho, ho, generator=g, device=DEV).to(dtype)
    add = torch.randn(batch, ci, h, h, generator=g, device=DEV).to(dtype)
    xd, dyd, addd = _nhwc(x).contiguous(), _nhwc(dy).contiguous(), _nhwc(add).contiguous()
    # forward + BN partial sums
    y, st = ops.conv2d_fwd(xd, w.permute(0, 2, 3, 1).contiguous(), s, p, want_stats=True)
    _record(tag + " fwd", ops)
    r = B.conv_fwd_ref(x, w, s, p)
    _within(y, r, dtype, tag + " fwd")
    _stats(st, r, tag + " fwd stats")
    del y, st, r
    # data gradient + addend
    dx = ops.conv2d_dgrad(dyd, w.permute(1, 2, 3, 0).contiguous(), (batch, h, h, ci), s, p, addend=addd)
    _record(tag + " dgrad", ops)
    r = B.conv_dgrad_ref(dy, w, (h, h), s, p)
    a64 = addd.double()
    _within(dx, r, dtype, tag + " dgrad", out=r.acc + a64, epi=r.acc.abs() + a64.abs())
    del dx, r, a64
    # deterministic weight gradient
    dw = ops.conv2d_wgrad(xd, dyd, k, s, p)
    kn = _record(tag + " wgrad", ops)
    if batch == 256 and k == 3 and s == 1 and h >= 28:            # layers 1-2 at the benchmark size: the halo form
        assert kn.startswith("wgrad_halo"), kn
    _within(dw, B.conv_wgrad_ref(x, dy, k, s, p), torch.float32, tag + " wgrad", layout="krsc")


BN1X1 = [c for c in R50 if c[3] == 1 and c[4] == 1 and c[0].endswith("conv3") and c[1] in (64, 128)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,batch", RUNS[:2], ids=["bf16x256", "f16x32"])
@pytest.mark.parametrize("cfg", BN1X1, ids=[c[0] for c in BN1X1])
def test_bench_conv3_bn_from_gram(cfg, dtype, batch):
    """conv3 of layers 1-2 as the engine runs it at the benchmark size: Gram of the input, BN statistics from it, and the fused
    1x1 forward + BN apply + identity + ReLU (the row-streaming kernel), against fp64 with the kernel's own scale / shift."""
    from rgb_proprioceptive_pose_estimator_amd import ops
    name, ci, co, k, s, p, h = cfg
    tag = "%s %s x%d" % (name, str(dtype)[6:], batch)
    rows = batch * h * h
    g = torch.Generator(device=DEV).manual_seed(ci + co + h)
    x = F.relu(torch.randn(batch, h, h, ci, generator=g, device=DEV) * 1.2 + 0.3).to(dtype)
    w = (torch.randn(co, ci, generator=g, device=DEV) / ci ** 0.5).to(dtype)
    idn = F.relu(torch.randn(batch, h, h, co, generator=g, device=DEV)).to(dtype)
    gamma, beta = torch.rand(co, generator=g, device=DEV) + 0.5, torch.randn(co, generator=g, device=DEV) * 0.3
    S, s1, buf = ops.gram(x)
    _record(tag + " gram", ops)
    x64 = x.reshape(rows, ci).double()
    rg = B.gemm_ref_tn(x64, x64)
    B.assert_within(S, rg.acc, B.bound(rg, torch.float32), tag + " gram S")
    r1 = B.Ref(x64.sum(0), (x64 * x64).sum(0).sqrt(), rows)
    B.assert_within(s1, r1.acc, B.bound(r1, torch.float32), tag + " gram s1")
    scale, shift, mean, invstd = ops.bn_stats_from_gram(w, buf, rows, gamma, beta)
    r = B.linear_ref(x64, w)
    B.assert_gram_stats((scale, shift, mean, invstd), x64, w.double(), gamma, beta, tag + " bn_stats_from_gram")
    out, mask, _ = ops.conv1x1_fwd_bn(x, w, scale, shift, idn)
    _record(tag + " fwd_bn", ops)
    sc, sh, i64 = scale.double(), shift.double(), idn.reshape(rows, co).double()
    pre = r.acc * sc + sh + i64
    _within(out.reshape(rows, co), r, dtype, tag + " fwd_bn", out=F.relu(pre), gain=sc, epi=(r.acc * sc).abs() + sh.abs() + i64.abs())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,batch", RUNS, ids=["bf16x256", "f16x32", "f32x32"])
def test_bench_stem(dtype, batch):
    """the 7x7 / stride-2 stem on 224 x 224 images: forward + partial sums (the LDS-DMA ring) and weight gradient"""
    from rgb_proprioceptive_pose_estimator_amd import ops
    tag = "stem %s x%d" % (str(dtype)[6:], batch)
    g = torch.Generator(device=DEV).manual_seed(5)
    img = torch.randn(batch, 3, 224, 224, generator=g, device=DEV).to(dtype)
    w = (torch.randn(64, 3, 7, 7, generator=g, device=DEV) / 12.0).to(dtype)
    x4 = ops.stage_image(img.float(), dtype)
    y, st = ops.stem_conv_fwd(x4, ops.pack_stem_weight(w.float(), dtype), want_stats=True)
    _record(tag + " fwd", ops)
    r = B.conv_fwd_ref(img, w, 2, 3)
    _within(y, r, dtype, tag + " fwd")
    _stats(st, r, tag + " fwd stats")
    del y, st, r
    dy = torch.randn(batch, 64, 112, 112, generator=g, device=DEV).to(dtype)
    dw = ops.stem_conv_wgrad(x4, _nhwc(dy).contiguous())
    _record(tag + " wgrad", ops)
    _within(dw.reshape(64, 3, 7, 7).permute(0, 2, 3, 1), B.conv_wgrad_ref(img, dy, 7, 2, 3), torch.float32, tag + " wgrad", layout="krsc")


@pytest.mark.gpu
def test_gpu_builder_matches_cpu_builder():
    """the fp64 references built on the device (as every bound check here does) == the same builders on the CPU"""
    g = torch.Generator().manual_seed(2)
    x, w = torch.randn(4, 128, 28, 28, generator=g).bfloat16(), (torch.randn(128, 128, 3, 3, generator=g) / 34).bfloat16()
    dy = torch.randn(4, 128, 14, 14, generator=g).bfloat16()
    for f, args in ((B.conv_fwd_ref, (x, w, 2, 1)), (B.conv_dgrad_ref, (dy, w, (28, 28), 2, 1)), (B.conv_wgrad_ref, (x, dy, 3, 2, 1))):
        c = f(*args)
        d = f(*(a.to(DEV) if torch.is_tensor(a) else a for a in args))
        assert c.K == d.K
        for a, b in ((c.acc, d.acc), (c.Q, d.Q)):
            assert float((a - b.cpu()).abs().max()) <= 1e-12 * float(a.abs().max())
