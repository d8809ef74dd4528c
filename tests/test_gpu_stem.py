"""The front end every train step and rollout frame passes before the trunk, each entry point called directly through the C ABI and held to
the fp64 references and bounds of tests/_stem_bounds.py (built on the device from the operands the kernel reads: the staged x4 and the
packed weight are read back), on the cases of tests/_stem_cases.py:

- rpe_stage_image_nhwc4, rpe_stage_frames_u8, rpe_stage_frames_u8_resized (all four pass combinations) into a sentinel-filled x4: the
  interior within the normalisation's bound and rounded once (the image form bit for bit), channel 3 +0, every border element untouched;
- rpe_pack_stem_weight and rpe_pack_conv_weights_multi (tiled and element-wise paths) bit for bit; rpe_unpack_stem_grad exact;
- rpe_stem_conv_fwd and rpe_stem_conv_fwd_affine on ragged tiles, tiles that start inside an image and span several, non-square images;
- rpe_stem_conv_wgrad_det (bit-reproducible, both walk directions, its workspace contract) and the atomic rpe_stem_conv_wgrad (it
  accumulates into dw_packed), one split of M and several;
- rpe_transpose_f32, rpe_colsum, rpe_copy2d, rpe_relu_bwd beyond the one shape of test_small_utils;
- the shapes an entry point must refuse: the documented code, the outputs untouched.

Every output is prefilled with a sentinel and sits between sentinel guards in one allocation.  The bounds and the faults they reject are
judged on the CPU by tests/test_stem_cpu.py."""
import ctypes

import pytest
import torch

import _bounds as B
import _stem_bounds as SB
import _stem_cases as C

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from rgb_proprioceptive_pose_estimator_amd import ops

DEV = "cuda"
F32 = torch.float32
SENT = -12345.5
ERR_SHAPE, ERR_WORKSPACE = 1, 5      # include/rpe_hip.h
G = C.GUARD
PAD = C.PAD


def _lib():
    from rgb_proprioceptive_pose_estimator_amd._lib import lib
    return lib


def _raw():
    from rgb_proprioceptive_pose_estimator_amd._lib import raw
    return raw


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _name(dtype):
    return str(dtype)[6:]


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _same_values(got, ref):
    """bit for bit; where the reference is a NaN, a NaN"""
    nan = torch.isnan(ref)
    return bool((torch.isnan(got) == nan).all()) and bool((_bits(got) == _bits(ref))[~nan].all())


class Out:
    """n elements for the kernel between G sentinels in front and G behind, one allocation, all prefilled"""

    def __init__(self, n, dtype=F32, fill=SENT):
        self.n, self.fill = n, fill
        self.buf = torch.full((G + n + G,), fill, dtype=dtype, device=DEV)
        self.t = self.buf[G:G + n]

    def guards_ok(self):
        g = torch.cat([self.buf[:G], self.buf[G + self.n:]])
        return _same_bits(g, torch.full_like(g, self.fill))

    def untouched(self):
        return _same_bits(self.buf, torch.full_like(self.buf, self.fill))


def _norm3(v):
    return (ctypes.c_float * 3)(*(float(x) for x in v))


def _stored(got, ref, bnd, dtype, label):
    w = B.assert_within(got, ref, bnd, label)
    B.assert_rounds_once(got, ref, dtype, label, bnd)
    B.assert_unbiased(got, ref, dtype, label, bnd)
    return w


# ------------------------------------------------------------------ staging
def _x4_out(b, h, w, dtype):
    o = Out(b * (h + 2 * PAD) * (w + 2 * PAD) * 4, dtype)
    return o, o.t.view(b, h + 2 * PAD, w + 2 * PAD, 4)


def _check_frame(o, x4, b, h, w, label):
    """channel 3 of the interior is +0, the border and the guards still hold the sentinel -> the interior's channels 0-2"""
    inner = x4[:, PAD:PAD + h, PAD:PAD + w]
    assert not bool(_bits(inner[..., 3]).any()), label + ": channel 3 is not +0"
    border = SB.x4_border(b, h, w, DEV)
    assert _same_bits(x4[border], torch.full_like(x4[border], SENT)), label + ": %d border elements were written" % int(
        (_bits(x4[border]) != _bits(torch.full_like(x4[border], SENT))).sum())
    assert o.guards_ok(), label + ": wrote outside x4"
    return inner[..., :3]


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
@pytest.mark.parametrize("shape", C.IMAGE_SHAPES, ids=str)
def test_stage_image(dtype, shape):
    """rpe_stage_image_nhwc4 into a sentinel-filled x4: the interior is torch's .to(dtype) bit for bit (ties, subnormals, overflow to inf,
    signed zeros; a NaN for a NaN), channel 3 +0, the border untouched"""
    b, h, w = shape
    img = C.image_case(shape).to(DEV)
    o, x4 = _x4_out(b, h, w, dtype)
    _lib().rpe_stage_image_nhwc4(ops.dtype_code(dtype), _P(img), _P(o.t), b, h, w, _S())
    got = _check_frame(o, x4, b, h, w, "stage_image %s %s" % (_name(dtype), shape))
    ref = img.permute(0, 2, 3, 1).to(dtype)
    assert _same_values(got, ref), "stage_image %s %s: %d interior elements differ from .to(dtype)" % (_name(dtype), shape, int((_bits(got) != _bits(ref)).sum()))


def _normalised(got, src, mean, std, dtype, label):
    ref, bnd = SB.normalise_ref(src, C.f32(mean), C.f32(std), dtype)
    return _stored(got, ref, bnd, dtype, label)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
@pytest.mark.parametrize("geom", C.FRAME_GEOMS, ids=str)
def test_stage_frames_u8(dtype, geom):
    """rpe_stage_frames_u8: the floored centre crop, ((p / 255) - mean) / std from the fp32 mean / std within the bound of the kernel's
    statement and rounded once; channel 3 +0; border untouched.  The gross mean / std make a swapped channel a large error."""
    b, hs, ws, h, w = geom
    fr = C.frames_case(geom).to(DEV)
    src = SB.window(fr, (hs - h) // 2, (ws - w) // 2, h, w)
    if geom == C.ALL_BYTES:
        for c in range(3):
            assert torch.unique(src[..., c]).numel() == 256
    for name, mean, std in C.NORMS:
        label = "stage_frames_u8 %s %s %s" % (_name(dtype), geom, name)
        o, x4 = _x4_out(b, h, w, dtype)
        _lib().rpe_stage_frames_u8(ops.dtype_code(dtype), _P(fr), _P(o.t), b, hs, ws, h, w, _norm3(mean), _norm3(std), _S())
        _normalised(_check_frame(o, x4, b, h, w, label), src, mean, std, dtype, label)


def _tables(i, o):
    from rgb_proprioceptive_pose_estimator_amd.util.data_utils import pil_bilinear_tables
    if i == o:
        return None, None, 0
    bounds, kk = pil_bilinear_tables(i, o)
    return torch.from_numpy(bounds).to(DEV), torch.from_numpy(kk).contiguous().to(DEV), kk.shape[1]


def _stage_resized(call, dtype, fr, hr, wr, top, left, h, w, mean, std, tabs=None, tmp="auto"):
    """-> (status, Out of x4, x4 view, Out of tmp or None)"""
    b, hs, ws, _ = fr.shape
    (xb, xk, ksx), (yb, yk, ksy) = tabs if tabs is not None else (_tables(ws, wr), _tables(hs, hr))
    t = Out(b * hs * wr * 3, torch.uint8, 0xA5) if (tmp == "auto" and ws != wr) else None
    o, x4 = _x4_out(b, h, w, dtype)
    rc = call.rpe_stage_frames_u8_resized(ops.dtype_code(dtype), _P(fr), _P(o.t), b, hs, ws, hr, wr, top, left, h, w, _P(xb), _P(xk), ksx, _P(yb), _P(yk),
                                          ksy, None if t is None else _P(t.t), _norm3(mean), _norm3(std), _S())
    return rc, o, x4, t


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
@pytest.mark.parametrize("case", C.RESIZE_CASES, ids=lambda c: c[0])
def test_stage_frames_u8_resized(dtype, case):
    """rpe_stage_frames_u8_resized in each of its four modes: the integer part is oracle.pil_resize.resize_bilinear_u8 (Pillow, bit for
    bit), then the window and the normalisation's bound"""
    name, b, hs, ws, hr, wr, h, w, windows = case
    fr = C.resize_frames(b, hs, ws).to(DEV)
    assert not torch.equal(fr[0], fr[1])
    res = SB.resize_u8(fr, hr, wr)
    for top, left in windows:
        for nname, mean, std in C.NORMS[:1] if (top, left) != windows[0] else C.NORMS:
            label = "stage_frames_u8_resized %s %s (%d, %d) %s" % (_name(dtype), name, top, left, nname)
            rc, o, x4, t = _stage_resized(_lib(), dtype, fr, hr, wr, top, left, h, w, mean, std)
            assert t is None or t.guards_ok(), label + ": wrote outside tmp"
            _normalised(_check_frame(o, x4, b, h, w, label), SB.window(res, top, left, h, w), mean, std, dtype, label)


@pytest.mark.parametrize("geom", C.ODD_CROPS, ids=str)
def test_stage_frames_odd_crop_routes_to_the_window(geom):
    """ops.stage_frames on an odd crop difference: the window form at crop_origin's half-to-even offsets, bit for bit the direct call;
    the plain kernel floors there (test_stage_frames_u8, the geometry with odd differences) and is never sent such a case"""
    hs, ws, h, w = geom
    fr = C.resize_frames(2, hs, ws).to(DEV)
    route = ops.frames_route(hs, ws, h, w, min(hs, ws))
    top, left = int(round((hs - h) / 2.0)), int(round((ws - w) / 2.0))
    assert route == ("window", hs, ws, top, left)
    mean, std = C.IMAGENET_MEAN, C.IMAGENET_STD
    for dtype in C.DTYPES:
        got = ops.stage_frames(fr, dtype, (h, w), min(hs, ws), mean, std)
        rc, o, x4, _ = _stage_resized(_lib(), dtype, fr, hs, ws, top, left, h, w, mean, std)
        assert _same_bits(got[:, PAD:PAD + h, PAD:PAD + w], x4[:, PAD:PAD + h, PAD:PAD + w]) and not bool(got[SB.x4_border(2, h, w, DEV)].any())
        label = "stage_frames odd crop %s %s" % (_name(dtype), geom)
        _normalised(_check_frame(o, x4, 2, h, w, label), SB.window(fr, top, left, h, w), mean, std, dtype, label)


def test_staging_refusals():
    """bad geometry or missing operands: RPE_ERR_SHAPE, and x4 still all sentinel"""
    raw, mean, std = _raw(), _norm3(C.IMAGENET_MEAN), _norm3(C.IMAGENET_STD)
    fr = C.frames_case((2, 12, 16, 8, 10)).to(DEV)
    for dtype in C.DTYPES:
        code = ops.dtype_code(dtype)
        for hs, ws, m, s in ((7, 16, mean, std), (12, 9, mean, std), (12, 16, None, std), (12, 16, mean, None)):
            o, _ = _x4_out(2, 8, 10, dtype)
            assert raw.rpe_stage_frames_u8(code, _P(fr), _P(o.t), 2, hs, ws, 8, 10, m, s, _S()) == ERR_SHAPE
            assert o.untouched()
        fr2 = C.resize_frames(2, 12, 20).to(DEV)
        full = (_tables(20, 26), _tables(12, 16))
        # a window that leaves the resized frame, a negative top / left, missing tables, a missing tmp for a horizontal pass
        for top, left, tabs, tmp in ((9, 0, full, "auto"), (0, 17, full, "auto"), (-1, 0, full, "auto"), (0, -1, full, "auto"),
                                     (0, 0, ((None, None, 0), full[1]), "auto"), (0, 0, (full[0], (None, None, 0)), "auto"),
                                     (0, 0, ((full[0][0], full[0][1], 0), full[1]), "auto"), (0, 0, full, None)):
            rc, o, _, t = _stage_resized(raw, dtype, fr2, 16, 26, top, left, 8, 10, C.IMAGENET_MEAN, C.IMAGENET_STD, tabs, tmp)
            assert rc == ERR_SHAPE, (top, left, tmp)
            assert o.untouched() and (t is None or t.untouched())


# ------------------------------------------------------------------ stem conv
def _stage(img, dtype):
    """the zero-bordered x4 of an fp32 image, through the staging kernel"""
    b, _, h, w = img.shape
    x4 = torch.zeros(b, h + 2 * PAD, w + 2 * PAD, 4, dtype=dtype, device=DEV)
    _lib().rpe_stage_image_nhwc4(ops.dtype_code(dtype), _P(img), _P(x4), b, h, w, _S())
    return x4


def _pack_stem(w, scale, dtype, label):
    """rpe_pack_stem_weight, checked bit for bit -> [64, 8, 8, 4]"""
    o = Out(64 * 256, dtype)
    _lib().rpe_pack_stem_weight(ops.dtype_code(dtype), _P(w), _P(scale), _P(o.t), _S())
    assert o.guards_ok(), label + ": wrote outside the packed weight"
    wp = o.t.view(64, 8, 8, 4)
    assert _same_bits(wp, SB.pack_stem_ref(w, scale, dtype)), label + ": not (w * scale) in fp32 rounded once"
    assert not bool(wp[:, 7].float().abs().sum()) and not bool(wp[:, :, 7].float().abs().sum()) and not bool(wp[..., 3].float().abs().sum()), \
        label + ": tap row 7, tap column 7 or channel 3 is not zero"
    return wp


def _fwd(dtype, x4, wp, b, h, w, stats=True, bias=None, relu=0, affine=False):
    ho, wo = C.out_hw(h, w)
    m = b * ho * wo
    y = Out(m * 64, dtype)
    st = Out(((m + 127) // 128) * 2 * 64) if stats else None
    if affine:
        _lib().rpe_stem_conv_fwd_affine(ops.dtype_code(dtype), _P(x4), _P(wp), _P(y.t), _P(bias), relu, b, h, w, _S())
    else:
        _lib().rpe_stem_conv_fwd(ops.dtype_code(dtype), _P(x4), _P(wp), _P(y.t), None if st is None else _P(st.t), b, h, w, _S())
    assert y.guards_ok() and (st is None or st.guards_ok()), "stem forward wrote outside an output"
    return y.t.view(b, ho, wo, 64), None if st is None else st.t.view(-1, 2, 64)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
@pytest.mark.parametrize("shape", C.STEM_SHAPES, ids=str)
def test_stem_forward(dtype, shape):
    """rpe_stem_conv_fwd (y and the BN partial sums) and rpe_stem_conv_fwd_affine (with and without ReLU) against the fp64 conv of the
    staged image and the packed weight; rpe_pack_stem_weight bit for bit; x4 between NaN guards gives the same bits"""
    b, h, w = shape
    tag = "%s %s" % (_name(dtype), shape)
    d = {k: v.to(DEV) for k, v in C.stem_case(dtype, shape).items()}
    x4 = _stage(d["img"], dtype)
    wp = _pack_stem(d["w"], None, dtype, "pack_stem_weight " + tag)
    y, st = _fwd(dtype, x4, wp, b, h, w)
    r = SB.stem_fwd_ref(x4, wp, h, w)
    _stored(y, r.acc, B.bound(r, dtype), dtype, "stem_fwd y " + tag)
    assert st.shape[0] == len(C.fwd_tiles(b, h, w)[1])
    B.assert_stats(st, r, "stem_fwd stats " + tag)
    # without the statistics, and with tap row 7 of the packed weight poisoned (K = 224: the row is never read): the same bits
    assert _same_bits(_fwd(dtype, x4, wp, b, h, w, stats=False)[0], y), tag + ": y depends on stats_part"
    poisoned = wp.clone()
    poisoned[:, 7] = C.NAN
    assert _same_bits(_fwd(dtype, x4, poisoned, b, h, w)[0], y), tag + ": tap row 7 of the packed weight is read"
    # x4 between NaN guards in one allocation, at a 16-byte-aligned offset that is no multiple of 32 bytes
    off = 8 * 5
    big = torch.full((off + x4.numel() + 4096,), C.NAN, dtype=dtype, device=DEV)
    inner = big[off:off + x4.numel()]
    inner.copy_(x4.view(-1))
    assert inner.data_ptr() % 16 == 0
    y2, st2 = _fwd(dtype, inner, wp, b, h, w)
    assert bool(torch.isfinite(y2).all()) and bool(torch.isfinite(st2).all()) and _same_bits(y2, y) and _same_bits(st2, st), tag + ": a read outside x4"
    # the affine form on the scale-folded weight
    wps = _pack_stem(d["w"], d["scale"], dtype, "pack_stem_weight scaled " + tag)
    r2 = SB.stem_fwd_ref(x4, wps, h, w)
    for relu in (0, 1):
        out, _ = _fwd(dtype, x4, wps, b, h, w, stats=False, bias=d["bias"], relu=relu, affine=True)
        ref, bnd = SB.affine_ref(r2, d["bias"], relu, dtype)
        _stored(out, ref, bnd, dtype, "stem_fwd_affine relu=%d %s" % (relu, tag))
        if relu:
            zeros = float((ref == 0).double().mean())
            assert 0.2 < zeros < 0.8, "the case does not exercise the ReLU's zero: %.2f" % zeros
            assert bool((out >= 0).all())


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
@pytest.mark.parametrize("shape", C.STEM_SHAPES, ids=str)
def test_stem_wgrad(dtype, shape):
    """rpe_stem_conv_wgrad_det and the atomic rpe_stem_conv_wgrad against the fp64 weight gradient of the staged image: within the bound;
    the deterministic form bit-reproducible under every walk direction and refusing a short workspace; the atomic form accumulating into
    dw_packed; channel 3 exactly zero"""
    b, h, w = shape
    tag = "%s %s" % (_name(dtype), shape)
    lib, code = _lib(), ops.dtype_code(dtype)
    d = {k: v.to(DEV) for k, v in C.stem_case(dtype, shape).items()}
    x4, dy = _stage(d["img"], dtype), d["dy"].contiguous()
    plan = C.wgrad_plan(b, h, w, dtype)
    need = lib.rpe_stem_conv_wgrad_workspace_bytes(code, b, h, w)
    assert need == plan["slab_bytes"], "the restated split of M (%r) is not the launcher's: %d bytes" % (plan, need)
    ws = Out(need, torch.uint8, 0xA5)
    r = SB.stem_wgrad_ref(x4, dy, h, w)
    bnd = B.bound(r, F32)

    def det(nbytes=need, call=lib):
        o = Out(64 * 256)
        rc = call.rpe_stem_conv_wgrad_det(code, _P(x4), _P(dy), _P(o.t), b, h, w, _P(ws.t), nbytes, _S())
        assert o.guards_ok() and ws.guards_ok(), tag + ": wrote outside dw_packed or the workspace"
        return rc, o

    _, o = det()
    B.assert_within(SB.packed_grad(o.t), r.acc, bnd, "stem_wgrad_det " + tag, layout="krsc")
    assert not bool(_bits(o.t.view(64, 8, 8, 4)[..., 3]).any()), tag + ": channel 3 of dw_packed is not +0"
    try:
        for mode in (0, 1, 2, 2):
            ops.set_walk_direction(mode)
            assert _same_bits(det()[1].t, o.t), "%s: the deterministic form differs under walk direction %d" % (tag, mode)
    finally:
        ops.set_walk_direction(0)
    rc, short = det(need - 1, _raw())
    assert rc == ERR_WORKSPACE and short.untouched(), tag + ": a workspace one byte short"
    # the atomic form accumulates: zero prefill, and a prefill of the gradient's own size
    g = torch.Generator(device=DEV).manual_seed(7)
    for name, pre in (("zero", torch.zeros(64 * 256, device=DEV)), ("nonzero", torch.randn(64 * 256, generator=g, device=DEV) * float(r.acc.abs().mean()))):
        o = Out(64 * 256)
        o.t.copy_(pre)
        lib.rpe_stem_conv_wgrad(code, _P(x4), _P(dy), _P(o.t), b, h, w, _S())
        assert o.guards_ok(), tag + ": the atomic form wrote outside dw_packed"
        p = SB.packed_grad(pre).double()
        ref = p + r.acc
        B.assert_within(SB.packed_grad(o.t), ref, B.bound(r, F32, out=ref, epi=r.acc.abs() + p.abs()), "stem_wgrad atomic %s %s" % (name, tag), layout="krsc")
        assert _same_bits(o.t.view(64, 8, 8, 4)[..., 3], pre.view(64, 8, 8, 4)[..., 3]), tag + ": channel 3 of dw_packed moved"


def test_unpack_stem_grad():
    """a pure permutation: exact; tap row 7, tap column 7 and channel 3 of the packed input are NaN and none reaches the output"""
    dp = torch.randn(64, 8, 8, 4, generator=torch.Generator().manual_seed(11)).to(DEV)
    dp[:, 7], dp[:, :, 7], dp[..., 3] = C.NAN, C.NAN, C.NAN
    o = Out(64 * 147)
    _lib().rpe_unpack_stem_grad(_P(dp), _P(o.t), _S())
    assert o.guards_ok()
    got = o.t.view(64, 3, 7, 7)
    assert not bool(torch.isnan(got).any()) and _same_bits(got, SB.unpack_stem_ref(dp))


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
def test_stem_refusals(dtype):
    """odd H or W, H or W below 7, B <= 0: RPE_ERR_SHAPE from every stem entry point, the outputs still all sentinel"""
    raw, code = _raw(), ops.dtype_code(dtype)
    x4 = torch.zeros(2 * 16 * 16 * 4, dtype=dtype, device=DEV)
    wp = torch.zeros(64 * 256, dtype=dtype, device=DEV)
    dy = torch.zeros(2 * 8 * 8 * 64, dtype=dtype, device=DEV)
    bias = torch.zeros(64, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    for b, h, w in C.STEM_REFUSED:
        y, st, dwp = Out(2 * 8 * 8 * 64, dtype), Out(2 * 64), Out(64 * 256)
        assert raw.rpe_stem_conv_fwd(code, _P(x4), _P(wp), _P(y.t), _P(st.t), b, h, w, _S()) == ERR_SHAPE
        assert raw.rpe_stem_conv_fwd_affine(code, _P(x4), _P(wp), _P(y.t), _P(bias), 1, b, h, w, _S()) == ERR_SHAPE
        assert raw.rpe_stem_conv_wgrad(code, _P(x4), _P(dy), _P(dwp.t), b, h, w, _S()) == ERR_SHAPE
        assert raw.rpe_stem_conv_wgrad_det(code, _P(x4), _P(dy), _P(dwp.t), b, h, w, _P(ws), ws.numel(), _S()) == ERR_SHAPE
        assert raw.rpe_stem_conv_wgrad_workspace_bytes(code, b, h, w) == -1
        assert y.untouched() and st.untouched() and dwp.untouched(), (b, h, w)


# ------------------------------------------------------------------ rpe_pack_conv_weights_multi
def _pack_multi(table, dtype, nlayers=None, total=None, call=None):
    """-> (status, [(src, scale, Out wf or None, Out wd or None)])"""
    from rgb_proprioceptive_pose_estimator_amd._lib import PackDesc
    case = C.pack_case(table)
    starts, tot = C.pack_starts(table)
    tab, layers = (PackDesc * len(table))(), []
    for d, (co, rs, ci, _, has_wf, has_wd), c, s in zip(tab, table, case, starts):
        src, scale = c["src"].to(DEV), None if c["scale"] is None else c["scale"].to(DEV)
        wf, wd = (Out(co * rs * ci, dtype) if has_wf else None), (Out(co * rs * ci, dtype) if has_wd else None)
        d.src, d.Co, d.RS, d.Ci, d.start = src.data_ptr(), co, rs, ci, s
        d.wf, d.wd = (None if wf is None else wf.t.data_ptr()), (None if wd is None else wd.t.data_ptr())
        d.scale = None if scale is None else scale.data_ptr()
        layers.append((src, scale, wf, wd))
    dev_tab = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(DEV)
    rc = (call or _lib()).rpe_pack_conv_weights_multi(ops.dtype_code(dtype), _P(dev_tab), len(table) if nlayers is None else nlayers,
                                                      tot if total is None else total, _S())
    torch.cuda.synchronize()
    return rc, layers


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
@pytest.mark.parametrize("table", [C.PACK_TABLE, C.PACK_TABLE_TILED], ids=["mixed", "tiled"])
def test_pack_conv_weights_multi(dtype, table):
    """every wf / wd bit for bit rpe_pack_conv_weight of that layer (wf of a scaled layer: fp32 w * scale[co] rounded once, wd unscaled);
    null outputs are skipped; the guards between the layers' buffers hold.  `mixed` takes the element-wise path from its third layer on
    (a chunk straddles two layers), `tiled` the 64 x 64 tiles throughout."""
    _, layers = _pack_multi(table, dtype)
    for i, ((co, rs, ci, _, _, _), (src, scale, wf, wd)) in enumerate(zip(table, layers)):
        label = "pack_conv_weights_multi %s layer %d %s" % (_name(dtype), i, (co, rs, ci))
        one_f, one_d = Out(src.numel(), dtype), Out(src.numel(), dtype)
        _lib().rpe_pack_conv_weight(ops.dtype_code(dtype), _P(src), _P(one_f.t), _P(one_d.t), co, rs, 1, ci, _S())
        assert one_f.guards_ok() and one_d.guards_ok()
        ref_f, ref_d = SB.pack_ref(src, scale, dtype)
        assert _same_bits(one_d.t, ref_d.view(-1)) and _same_bits(one_f.t, SB.pack_ref(src, None, dtype)[0].view(-1)), label + ": rpe_pack_conv_weight"
        if wf is not None:
            assert wf.guards_ok(), label + ": wrote outside wf"
            assert _same_bits(wf.t, ref_f.view(-1)), label + ": %d elements of wf differ" % int((_bits(wf.t) != _bits(ref_f.view(-1))).sum())
        if wd is not None:
            assert wd.guards_ok(), label + ": wrote outside wd"
            assert _same_bits(wd.t, one_d.t), label + ": %d elements of wd differ" % int((_bits(wd.t) != _bits(one_d.t)).sum())


def test_pack_conv_weights_multi_refusals():
    """nlayers of 0 and 256, total <= 0: RPE_ERR_SHAPE, nothing written"""
    for nlayers, total in ((0, None), (256, None), (None, 0), (None, -4096)):
        rc, layers = _pack_multi(C.PACK_TABLE_TILED, torch.bfloat16, nlayers, total, _raw())
        assert rc == ERR_SHAPE, (nlayers, total)
        assert all(o is None or o.untouched() for _, _, wf, wd in layers for o in (wf, wd))


# ------------------------------------------------------------------ small fp32 utilities
@pytest.mark.parametrize("case", C.TRANSPOSE_CASES, ids=str)
def test_transpose_f32(case):
    """out[c][r] = in[r][c], the pad columns rows .. ldo zero, exact; the columns of `in` past cols are never read (NaN)"""
    rows, cols, ldi, ldo = case
    x = torch.randn(rows, ldi, generator=torch.Generator().manual_seed(rows)).to(DEV)
    x[:, cols:] = C.NAN
    o = Out(cols * ldo)
    _lib().rpe_transpose_f32(_P(x), _P(o.t), rows, cols, ldi, ldo, _S())
    assert o.guards_ok()
    got = o.t.view(cols, ldo)
    assert _same_bits(got[:, :rows], x[:, :cols].t().contiguous()) and not bool(_bits(got[:, rows:]).any())


@pytest.mark.parametrize("case", C.COLSUM_CASES, ids=str)
def test_colsum(case):
    """the fp32 column sums within the GEMM bound of a K = rows reduction; accumulate = 1 adds to what `out` held"""
    rows, cols, ld = case
    x, old = (t.to(DEV) for t in C.colsum_case(rows, cols, ld))
    for acc in (0, 1):
        o = Out(cols)
        if acc:
            o.t.copy_(old)
        _lib().rpe_colsum(_P(x), rows, cols, ld, _P(o.t), acc, _S())
        assert o.guards_ok()
        ref, bnd = SB.colsum_ref(x, cols, old if acc else None)
        B.assert_within(o.t, ref, bnd, "colsum %s accumulate=%d" % (case, acc), layout="c")


@pytest.mark.parametrize("case", C.COPY2D_CASES, ids=str)
def test_copy2d(case):
    """strided on both sides: exact, nothing written outside the copied columns"""
    rows, cols, lds, ldd = case
    src = torch.randn(rows, lds, generator=torch.Generator().manual_seed(cols)).to(DEV)
    src[:, cols:] = C.NAN
    o = Out(rows * ldd)
    _lib().rpe_copy2d(_P(src), lds, _P(o.t), ldd, rows, cols, _S())
    got = o.t.view(rows, ldd)
    assert o.guards_ok() and _same_bits(got[:, :cols], src[:, :cols].contiguous())
    assert _same_bits(got[:, cols:], torch.full_like(got[:, cols:], SENT))


def test_relu_bwd():
    """dx = out > 0 ? dy : 0, exact: zeros of either sign and NaN give +0"""
    out = torch.tensor(C.RELU_OUT * 40, dtype=F32)
    dy = torch.randn(out.numel(), generator=torch.Generator().manual_seed(5))
    dy[::7] = -0.0
    o = Out(out.numel())
    out_d, dy_d = out.to(DEV), dy.to(DEV)
    _lib().rpe_relu_bwd(_P(out_d), _P(dy_d), _P(o.t), out.numel(), _S())
    assert o.guards_ok() and _same_bits(o.t.cpu(), torch.where(out > 0, dy, torch.zeros_like(dy)))


# ------------------------------------------------------------------ the thin wrappers of ops.py
@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
def test_wrappers_equal_the_direct_calls(dtype):
    """ops.stage_frames (both routes), pack_stem_weight(scale), stem_conv_fwd_affine, stem_conv_wgrad(deterministic) and
    pack_conv_weights_multi return, bit for bit, what the direct calls above were held to"""
    shape = (3, 10, 14)
    b, h, w = shape
    d = {k: v.to(DEV) for k, v in C.stem_case(dtype, shape).items()}
    x4 = ops.stage_image(d["img"], dtype)
    assert _same_bits(x4, _stage(d["img"], dtype))
    for scale in (None, d["scale"]):
        assert _same_bits(ops.pack_stem_weight(d["w"], dtype, scale), SB.pack_stem_ref(d["w"], scale, dtype))
    wps = ops.pack_stem_weight(d["w"], dtype, d["scale"])
    for relu in (False, True):
        assert _same_bits(ops.stem_conv_fwd_affine(x4, wps, d["bias"], relu), _fwd(dtype, x4, wps, b, h, w, stats=False, bias=d["bias"], relu=int(relu), affine=True)[0])
    r = SB.stem_wgrad_ref(x4, d["dy"], h, w)
    det = ops.stem_conv_wgrad(x4, d["dy"])
    assert _same_bits(det, ops.stem_conv_wgrad(x4, d["dy"], deterministic=True))
    for dw in (det, ops.stem_conv_wgrad(x4, d["dy"], deterministic=False)):
        B.assert_within(dw.permute(0, 2, 3, 1), r.acc, B.bound(r, F32), "ops.stem_conv_wgrad %s" % _name(dtype), layout="krsc")
    # frames: the plain route (even differences, nothing resized) and the window route (a resize)
    geom = (2, 12, 16, 8, 10)
    fr = C.frames_case(geom).to(DEV)
    assert ops.frames_route(12, 16, 8, 10, 12) == ("plain",)
    o, direct = _x4_out(2, 8, 10, dtype)
    _lib().rpe_stage_frames_u8(ops.dtype_code(dtype), _P(fr), _P(o.t), 2, 12, 16, 8, 10, _norm3(C.GROSS_MEAN), _norm3(C.GROSS_STD), _S())
    got = ops.stage_frames(fr, dtype, (8, 10), 12, C.GROSS_MEAN, C.GROSS_STD)
    assert _same_bits(got[:, PAD:PAD + 8, PAD:PAD + 10], direct[:, PAD:PAD + 8, PAD:PAD + 10]) and not bool(got[SB.x4_border(2, 8, 10, DEV)].any())
    route = ops.frames_route(12, 16, 8, 10, 16)
    assert route[0] == "window" and route[1:3] == (16, 21)
    _, o, direct, _ = _stage_resized(_lib(), dtype, fr, 16, 21, route[3], route[4], 8, 10, C.GROSS_MEAN, C.GROSS_STD)
    got = ops.stage_frames(fr, dtype, (8, 10), 16, C.GROSS_MEAN, C.GROSS_STD)
    assert _same_bits(got[:, PAD:PAD + 8, PAD:PAD + 10], direct[:, PAD:PAD + 8, PAD:PAD + 10]) and not bool(got[SB.x4_border(2, 8, 10, DEV)].any())
    # the one-launch packing
    case = C.pack_case(C.PACK_TABLE)
    layers = [(c["src"].view(co, 3, 3, ci).to(DEV) if rs == 9 else c["src"].view(co, 1, 1, ci).to(DEV), None if c["scale"] is None else c["scale"].to(DEV))
              for (co, rs, ci, _, _, _), c in zip(C.PACK_TABLE, case)]
    for (wsrc, scale), (wf, wd) in zip(layers, ops.pack_conv_weights_multi(layers, dtype)):
        ref_f, ref_d = SB.pack_ref(wsrc.view(wsrc.shape[0], -1, wsrc.shape[3]), scale, dtype)
        assert _same_bits(wf.view(-1), ref_f.view(-1)) and _same_bits(wd.view(-1), ref_d.view(-1))
        assert _same_bits(wd, ops.pack_conv_weight(wsrc, dtype)[1])
