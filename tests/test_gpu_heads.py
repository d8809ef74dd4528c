"""The head kernels of csrc/heads.hip, each entry point called directly and held element by element to the fp64 references and bounds of
tests/_head_bounds.py (built on the device from the operands the kernel reads), on the cases of tests/_head_cases.py: the aux head
forward / backward in its three C = 64 forms and its any-channel form, the winner taps, the aux head fused into the stem's apply + pool
pass and the det_y backward (both bit for bit against the calls they replace), the depth heads and their backward, tensor_add, and the
argument checks.  The bounds and the mutants they reject are judged on the CPU by tests/test_heads_cpu.py."""
import ctypes

import pytest
import torch

import _bounds as B
import _head_bounds as HB
import _head_cases as C

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from rgb_proprioceptive_pose_estimator_amd import ops

DEV = "cuda"
F32 = torch.float32
SENT = -12345.5                      # outputs are prefilled with it: columns / elements a kernel must not touch keep it
ERR_SHAPE, ERR_WORKSPACE = 1, 5      # include/rpe_hip.h


def _lib():
    from rgb_proprioceptive_pose_estimator_amd._lib import lib
    return lib


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _name(dtype):
    return str(dtype)[6:]


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _dev(case):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in case.items()}


def _within(got, ref, bnd, label, mask=None):
    if mask is not None:
        got, ref, bnd = got[mask], ref[mask], bnd[mask]
    if ref.numel() == 0:
        return 0.0
    return B.assert_within(got, ref, bnd, label, layout="i" if ref.dim() == 1 else None)


# ------------------------------------------------------------------ aux head
def aux_fwd(dtype, d, form):
    """-> out [b, ld] (ld = windows + 5, prefilled), raw [b, n], idx [b, n]"""
    lib, code = _lib(), ops.dtype_code(dtype)
    b, h, wd, c = d["x"].shape
    n = C.windows(h, wd)
    ld = n + 5
    out = torch.full((b, ld), SENT, device=DEV)
    raw = torch.full((b, n), SENT, device=DEV)
    idx = torch.full((b, n), 9, dtype=torch.uint8, device=DEV)
    if form == "c":
        lib.rpe_aux_head_fwd_c(code, _P(d["x"]), c, _P(d["w"]), _P(d["bias"]), _P(d["depth_feat"]), _P(out), ld, _P(raw), _P(idx), b, h, wd, _S())
    else:
        assert c == 64
        lib.rpe_aux_head_fwd(code, _P(d["x"]), _P(d["w"]), _P(d["bias"]), _P(d["depth_feat"]), _P(out), ld, _P(raw), _P(idx), b, h, wd, _S())
    return out, raw, idx


def check_aux_fwd(label, d, out, raw, idx):
    """raw and out within their bounds, the columns behind the feature untouched, idx the fp64 argmax in decided windows and a
    defensible tap elsewhere, the constructed windows exactly by the scan-order rule, a NaN window NaN with idx 2"""
    b, h, wd, c = d["x"].shape
    n, wo = C.windows(h, wd), wd // 2
    ref = HB.aux_fwd_ref(d["x"], d["w"], d["bias"], d["depth_feat"])
    fin = ref["finite"]
    _within(raw, ref["raw"], ref["braw"], label + " raw", fin)
    _within(out[:, :n], ref["out"], ref["bout"], label + " out", fin)
    assert bool((out[:, n:] == SENT).all()), "%s: wrote behind the %d feature columns of a row" % (label, n)
    bad = HB.idx_errors(idx, ref)
    assert bad == 0, "%s: %d winner taps no correct kernel can choose" % (label, bad)
    und = int((~ref["decided"] & fin).sum())
    assert und <= 1e-3 * b * n, "%s: %d undecided windows" % (label, und)
    for (i, oh, ow) in d["slots"]:
        p = oh * wo + ow
        if bool(fin[i, p]):
            assert int(idx[i, p]) == int(ref["idx"][i, p]), "%s: constructed window (%d, %d, %d): tap %d, the scan order gives %d" % (
                label, i, oh, ow, int(idx[i, p]), int(ref["idx"][i, p]))
        else:
            assert bool(raw[i, p].isnan()) and bool(out[i, p].isnan()) and int(idx[i, p]) == 2, "%s: NaN window (%d, %d, %d)" % (label, i, oh, ow)
    return ref


def aux_bwd(dtype, d, raw, idx, form, start=(0.5, -0.25)):
    """form atomic / det / c -> d_depth_feat, d_x, dw, dbias.  d_x, d_depth_feat prefilled with poison; dw / dbias start at `start`
    (the det form must overwrite them)"""
    lib, code = _lib(), ops.dtype_code(dtype)
    b, h, wd, c = d["x"].shape
    n = C.windows(h, wd)
    dout = torch.full((b, n + 5), SENT, device=DEV)
    dout[:, :n] = d["dout"]
    d_x = torch.full(d["x"].shape, 3.0, dtype=dtype, device=DEV)
    dw, db = torch.full((c,), start[0], device=DEV), torch.full((1,), start[1], device=DEV)
    ddf = None if d["depth_feat"] is None else torch.full((b, n), SENT, device=DEV)
    head = (code, _P(dout), n + 5, _P(d["x"]))
    tail = (_P(d["w"]), _P(d["depth_feat"]), _P(raw), _P(idx), _P(d_x), _P(dw), _P(db), _P(ddf), b, h, wd)
    if form == "c":
        lib.rpe_aux_head_bwd_c(*head, c, *tail, _S())
    elif form == "atomic":
        lib.rpe_aux_head_bwd(*head, *tail, _S())
    else:
        ws = torch.full((lib.rpe_aux_head_bwd_workspace_floats(code, b, h, wd),), float("nan"), device=DEV)
        lib.rpe_aux_head_bwd_det(*head, *tail, _P(ws), ws.numel(), _S())
        first = (dw.clone(), db.clone(), d_x.clone())
        dw.fill_(7.0), db.fill_(-7.0)
        lib.rpe_aux_head_bwd_det(*head, *tail, _P(ws), ws.numel(), _S())
        assert _same_bits(dw, first[0]) and _same_bits(db, first[1]) and _same_bits(d_x, first[2]), "aux_head_bwd_det does not repeat bit for bit"
        dw.fill_(7.0), db.fill_(-7.0)          # the compact form (no feature gradient): the same sums
        lib.rpe_aux_head_bwd_det(*head, *tail[:4], None, *tail[5:], _P(ws), ws.numel(), _S())
        assert _same_bits(dw, first[0]) and _same_bits(db, first[1]), "aux_head_bwd_det: the compact form sums differently"
    return ddf, d_x, dw, db


def check_aux_bwd(label, dtype, d, raw, idx, got, start, steps):
    ddf, d_x, dw, db = got
    b, h, wd, c = d["x"].shape
    rb = HB.aux_bwd_ref(d["dout"], d["x"], d["w"], d["depth_feat"], raw, idx, dtype, start, steps)
    if ddf is not None:
        _within(ddf, *rb["ddf"], label + " d_depth_feat")
    img, ih, iw = rb["winner"]
    gw = d_x[img, ih, iw]
    _within(gw, *rb["gx"], label + " d_x (winners)")
    B.assert_rounds_once(gw, rb["gx"][0], dtype, label + " d_x (winners)", rb["gx"][1])
    lose = torch.ones(b, h, wd, dtype=torch.bool, device=DEV)
    lose[img, ih, iw] = False
    nz = int((_bits(d_x)[lose] != 0).sum())
    assert nz == 0, "%s: %d elements outside the winner pixels are not +0" % (label, nz)
    _within(dw, *rb["dw"], label + " dw")
    _within(db, *rb["db"], label + " dbias")


def _atomic_steps(dtype, total, form):
    return C.ew_grid(total, 32) if form == "c" else min(1024, C.ew_grid(total, (16 if dtype == F32 else 32) * 4))


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
@pytest.mark.parametrize("shape", C.AUX_SHAPES, ids=str)
def test_aux_head_c64(dtype, shape):
    """rpe_aux_head_fwd, rpe_aux_head_bwd (atomic, onto a non-zero start) and rpe_aux_head_bwd_det (overwriting, repeating bit for bit):
    post-ReLU and signed features, with and without the depth feature, plain and with each constructed window"""
    b, h, w = shape
    for kind in C.KINDS:
        for use_depth in (False, True):
            for con in C.CONSTRUCTS:
                label = "aux64 %s %s %s depth=%d %s" % (_name(dtype), shape, kind, use_depth, con)
                d = _dev(C.aux_case(dtype, b, h, w, 64, kind, use_depth, con))
                out, raw, idx = aux_fwd(dtype, d, "64")
                check_aux_fwd(label, d, out, raw, idx)
                if con == "nan":
                    continue
                start = (0.5, -0.25)
                check_aux_bwd(label + " bwd", dtype, d, raw, idx, aux_bwd(dtype, d, raw, idx, "atomic", start), start,
                              _atomic_steps(dtype, b * C.windows(h, w), "64"))
                check_aux_bwd(label + " det", dtype, d, raw, idx, aux_bwd(dtype, d, raw, idx, "det", start), (0.0, 0.0), 0)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
def test_aux_head_c64_second_grid_trip(dtype):
    """forward only: more windows than 4096 blocks take in one trip (16 per block in fp32, 32 in 16-bit)"""
    b, h, w = C.AUX_BIG[dtype]
    assert b * C.windows(h, w) > 4096 * (16 if dtype == F32 else 32)
    d = _dev(C.aux_case(dtype, b, h, w, 64, "relu", True, "tie"))
    out, raw, idx = aux_fwd(dtype, d, "64")
    check_aux_fwd("aux64 %s %s" % (_name(dtype), (b, h, w)), d, out, raw, idx)


@pytest.mark.parametrize("dtype,c", [(t, c) for t in C.DTYPES for c in C.AUXC_C[t]], ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_aux_head_any_c(dtype, c):
    """rpe_aux_head_fwd_c / rpe_aux_head_bwd_c: one lane per pixel (C = one chunk) up to 64 lanes walking two (16-bit) or four (fp32)
    chunks each at C = 1024; even, odd (the last row and column belong to no window: their gradient is +0) and 14 x 14 maps"""
    for (h, w) in C.AUXC_HW:
        for b in C.AUXC_B:
            for k, con in enumerate(C.CONSTRUCTS):
                kind, use_depth = C.KINDS[(k + b) % 2], bool((k + h) % 2)
                label = "auxc %s C=%d %s %s depth=%d %s" % (_name(dtype), c, (b, h, w), kind, use_depth, con)
                d = _dev(C.aux_case(dtype, b, h, w, c, kind, use_depth, con))
                out, raw, idx = aux_fwd(dtype, d, "c")
                check_aux_fwd(label, d, out, raw, idx)
                if con == "nan":
                    continue
                start = (0.5, -0.25)
                check_aux_bwd(label + " bwd", dtype, d, raw, idx, aux_bwd(dtype, d, raw, idx, "c", start), start,
                              _atomic_steps(dtype, b * C.windows(h, w), "c"))


def test_aux_head_any_c_second_grid_trip():
    """forward only: 64 lanes per pixel leave 4 windows per block; more than 4096 x 4 windows"""
    dtype, c, (b, h, w) = C.AUXC_BIG
    assert b * C.windows(h, w) > 4096 * 4 and c // C.CE[dtype] >= 64
    d = _dev(C.aux_case(dtype, b, h, w, c, "relu", True, "zero"))
    out, raw, idx = aux_fwd(dtype, d, "c")
    check_aux_fwd("auxc %s C=%d %s" % (_name(dtype), c, (b, h, w)), d, out, raw, idx)


# ------------------------------------------------------------------ the aux head inside the stem's apply + pool pass; det_y
def _stem_shapes():
    return C.AUX_SHAPES + ["big"]


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
@pytest.mark.parametrize("shape", _stem_shapes(), ids=str)
def test_fused_stem_aux_is_the_two_calls_bit_for_bit(dtype, shape):
    """rpe_bn_apply_maxpool3x3s2_aux: a, out, idx as rpe_bn_apply_maxpool3x3s2 writes them, and aux_out / aux_raw / aux_idx as
    rpe_aux_head_fwd computes them from that a -- bit for bit, with and without the depth feature, with ld_aux_out > n (the columns
    behind stay untouched), and with a = NULL"""
    lib, code = _lib(), ops.dtype_code(dtype)
    b, h, w = C.AUX_BIG[dtype] if shape == "big" else shape
    n, ho, wo = C.windows(h, w), h // 2, w // 2
    for kind in (C.KINDS if shape != "big" else C.KINDS[:1]):
        for use_depth in (False, True):
            d = _dev(C.stem_case(dtype, b, h, w, kind, use_depth))
            y = d["x"]
            a = torch.full_like(y, 3.0)
            pool, pidx = torch.full((b, ho, wo, 64), 3.0, dtype=dtype, device=DEV), torch.full((b, ho, wo, 64), 99, dtype=torch.uint8, device=DEV)
            lib.rpe_bn_apply_maxpool3x3s2(code, _P(y), _P(d["scale"]), _P(d["shift"]), _P(a), _P(pool), _P(pidx), b, h, w, 64, _S())
            want = aux_fwd(dtype, dict(d, x=a), "64")
            for with_a in (True, False):
                a2 = torch.full_like(y, 3.0) if with_a else None
                pool2, pidx2 = torch.full_like(pool, 5.0), torch.full_like(pidx, 98)
                ld = n + 5
                out = torch.full((b, ld), SENT, device=DEV)
                raw, idx = torch.full((b, n), SENT, device=DEV), torch.full((b, n), 9, dtype=torch.uint8, device=DEV)
                lib.rpe_bn_apply_maxpool3x3s2_aux(code, _P(y), _P(d["scale"]), _P(d["shift"]), _P(a2), _P(pool2), _P(pidx2), b, h, w, _P(d["w"]),
                                                  _P(d["bias"]), _P(d["depth_feat"]), _P(out), ld, _P(raw), _P(idx), _S())
                label = "stem aux %s %s %s depth=%d a=%s" % (_name(dtype), (b, h, w), kind, use_depth, "tensor" if with_a else "NULL")
                if with_a:
                    assert _same_bits(a2, a), label + ": a"
                assert _same_bits(pool2, pool) and _same_bits(pidx2, pidx), label + ": pooled output / winner taps"
                diff = int((_bits(raw) != _bits(want[1])).sum())
                assert diff == 0, "%s: aux_raw differs from rpe_aux_head_fwd in %d of %d windows (max %g)" % (
                    label, diff, raw.numel(), float((raw - want[1]).abs().max()))
                assert _same_bits(idx, want[2]), label + ": aux_idx"
                assert _same_bits(out, want[0]), label + ": aux_out (or the columns behind it)"


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
@pytest.mark.parametrize("shape", C.AUX_SHAPES, ids=str)
def test_aux_head_bwd_det_y_is_det_on_the_activated_tensor(dtype, shape):
    """rpe_aux_head_bwd_det_y(y, scale, shift) against rpe_aux_head_bwd_det(a1 = rpe_bn_apply(y, scale, shift, relu), d_a1 = NULL):
    dw, dbias and d_depth_feat bit for bit; dw and dbias, besides, within their bounds"""
    lib, code = _lib(), ops.dtype_code(dtype)
    b, h, w = shape
    n = C.windows(h, w)
    for kind in C.KINDS:
        for use_depth in (False, True):
            d = _dev(C.stem_case(dtype, b, h, w, kind, use_depth))
            a1 = torch.empty_like(d["x"])
            lib.rpe_bn_apply(code, _P(d["x"]), None, _P(a1), _P(d["scale"]), _P(d["shift"]), b * h * w, 64, 1, _S())
            da = dict(d, x=a1)
            out, raw, idx = aux_fwd(dtype, da, "64")
            assert int(idx.max()) <= 3
            dout = d["dout"].contiguous()
            ws = torch.full((lib.rpe_aux_head_bwd_workspace_floats(code, b, h, w),), float("nan"), device=DEV)
            res = []
            for form in ("det", "det_y"):
                dw, db = torch.full((64,), 7.0, device=DEV), torch.full((1,), 7.0, device=DEV)
                ddf = torch.full((b, n), SENT, device=DEV) if use_depth else None
                tail = (_P(d["w"]), _P(d["depth_feat"]), _P(raw), _P(idx))
                if form == "det":
                    lib.rpe_aux_head_bwd_det(code, _P(dout), n, _P(a1), *tail, None, _P(dw), _P(db), _P(ddf), b, h, w, _P(ws), ws.numel(), _S())
                else:
                    lib.rpe_aux_head_bwd_det_y(code, _P(dout), n, _P(d["x"]), _P(d["scale"]), _P(d["shift"]), *tail, _P(dw), _P(db), _P(ddf), b, h, w,
                                               _P(ws), ws.numel(), _S())
                res.append((dw, db, ddf))
            label = "det_y %s %s %s depth=%d" % (_name(dtype), shape, kind, use_depth)
            assert _same_bits(res[1][0], res[0][0]), "%s: dw differs from det on a1 (max %g)" % (label, float((res[1][0] - res[0][0]).abs().max()))
            assert _same_bits(res[1][1], res[0][1]), label + ": dbias"
            if use_depth:
                assert _same_bits(res[1][2], res[0][2]), label + ": d_depth_feat"
            rb = HB.aux_bwd_ref(dout, a1, d["w"], d["depth_feat"], raw, idx, dtype)
            _within(res[1][0], *rb["dw"], label + " dw")
            _within(res[1][1], *rb["db"], label + " dbias")


# ------------------------------------------------------------------ depth heads
def _depth_run(d, pools, entry):
    lib = _lib()
    b, h, w = d["depth"].shape
    n = (h >> pools) * (w >> pools)
    feat, xhat = torch.full((b * n + 8,), SENT, device=DEV), torch.full((b * n + 8,), SENT, device=DEV)
    if entry == "fwd":
        lib.rpe_depth_head_fwd(_P(d["depth"]), _P(d["w"]), _P(d["b"]), _P(feat), _P(xhat), b, h, w, _S())
    else:
        lib.rpe_depth_head_fwd_pools(_P(d["depth"]), _P(d["w"]), _P(d["b"]), _P(feat), _P(xhat), b, h, w, pools, _S())
    assert bool((feat[b * n:] == SENT).all()) and bool((xhat[b * n:] == SENT).all()), "depth head wrote behind its outputs"
    return feat[:b * n].view(b, n), xhat[:b * n].view(b, n)


def _check_depth(label, d, pools, kind, feat, xhat):
    r = HB.depth_fwd_ref(d["depth"], d["w"], d["b"], pools)
    _within(xhat, *r["xhat"], label + " xhat")
    _within(feat, *r["feat"], label + " feat")
    if kind == "const" or xhat.shape[1] == 1:      # zero variance: xhat exactly 0, feat exactly b
        assert bool((xhat == 0).all()) and bool((feat == d["b"]).all()), label + ": zero variance is not exact"


@pytest.mark.parametrize("hw", C.DEPTH_HW, ids=str)
@pytest.mark.parametrize("b", C.DEPTH_B)
def test_depth_head_fwd(hw, b):
    """rpe_depth_head_fwd and rpe_depth_head_fwd_pools(pools = 2) associate their window sums differently: both are held to the same
    fp64 reference, not to each other"""
    for kind in C.DEPTH_KINDS:
        d = _dev(C.depth_case(b, hw[0], hw[1], kind))
        for entry in ("fwd", "pools"):
            feat, xhat = _depth_run(d, 2, entry)
            _check_depth("depth %s %s b=%d %s" % (entry, hw, b, kind), d, 2, kind, feat, xhat)


@pytest.mark.parametrize("h,w,pools", C.DEPTH_POOLS)
def test_depth_head_fwd_pools(h, w, pools):
    for kind in C.DEPTH_KINDS:
        d = _dev(C.depth_case(2, h, w, kind))
        feat, xhat = _depth_run(d, pools, "pools")
        _check_depth("depth pools=%d %s %s" % (pools, (h, w), kind), d, pools, kind, feat, xhat)


@pytest.mark.parametrize("n", C.DEPTH_BWD_NS)
def test_depth_head_bwd(n):
    """rpe_depth_head_bwd accumulates onto non-zero dw / db"""
    d = _dev(C.depth_bwd_case(n))
    dw, db = torch.full((1,), C.DEPTH_BWD_START[0], device=DEV), torch.full((1,), C.DEPTH_BWD_START[1], device=DEV)
    _lib().rpe_depth_head_bwd(_P(d["d_feat"]), _P(d["xhat"]), n, _P(dw), _P(db), _S())
    r = HB.depth_bwd_ref(d["d_feat"], d["xhat"], C.DEPTH_BWD_START, C.depth_bwd_blocks(n))
    _within(dw, *r["dw"], "depth bwd n=%d dw" % n)
    _within(db, *r["db"], "depth bwd n=%d db" % n)


# ------------------------------------------------------------------ tensor_add
@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
@pytest.mark.parametrize("k", range(3))
def test_tensor_add(dtype, k):
    """dst += src is (dst.float() + src.float()).to(dtype) bit for bit; the elements after n stay as they were"""
    n, guard = C.tensor_add_ns(dtype)[k], 16
    dst, src = (t.to(DEV) for t in C.tensor_add_case(dtype, n, guard))
    want = dst.clone()
    want[:n] = (dst[:n].float() + src[:n].float()).to(dtype)
    _lib().rpe_tensor_add(ops.dtype_code(dtype), _P(dst), _P(src), n, _S())
    diff = int((_bits(dst) != _bits(want)).sum())
    assert diff == 0, "tensor_add %s n=%d: %d elements differ (the last %d are guards)" % (_name(dtype), n, diff, guard)


# ------------------------------------------------------------------ argument checks
def test_argument_checks_return_their_code_and_launch_nothing():
    from rgb_proprioceptive_pose_estimator_amd._lib import raw
    buf = torch.full((4096,), SENT, device=DEV)           # every pointer: a kernel that ran would read or write it
    p, s = _P(buf), _S()
    f32, bf16 = ops.dtype_code(F32), ops.dtype_code(torch.bfloat16)
    assert raw.rpe_aux_head_fwd(f32, p, p, p, None, p, 8, p, p, 1, 3, 4, s) == ERR_SHAPE                   # odd H
    assert raw.rpe_aux_head_fwd(f32, p, p, p, None, p, 8, p, p, 1, 4, 3, s) == ERR_SHAPE                   # odd W
    for c in (96, 2048):                                                                                   # 12 chunks; past 1024
        assert raw.rpe_aux_head_fwd_c(bf16, p, c, p, p, None, p, 8, p, p, 1, 2, 2, s) == ERR_SHAPE
        assert raw.rpe_aux_head_bwd_c(bf16, p, 8, p, c, p, None, p, p, p, p, p, None, 1, 2, 2, s) == ERR_SHAPE
    assert raw.rpe_aux_head_bwd_c(bf16, p, 8, p, 64, p, None, p, p, None, p, p, None, 1, 2, 2, s) == ERR_SHAPE       # null d_x
    for (h, w, pools) in ((8, 8, 0), (8, 8, 7), (3, 8, 2), (8, 3, 2)):                                     # pools; H >> pools == 0
        assert raw.rpe_depth_head_fwd_pools(p, p, p, p, p, 1, h, w, pools, s) == ERR_SHAPE
    assert b"depth_head_fwd_pools" in raw.rpe_last_error()
    assert raw.rpe_tensor_add(bf16, p, p, 12, s) == ERR_SHAPE and raw.rpe_tensor_add(f32, p, p, 6, s) == ERR_SHAPE
    need = raw.rpe_aux_head_bwd_workspace_floats(f32, 1, 4, 4)
    assert need >= 65
    assert raw.rpe_aux_head_bwd_det(f32, p, 4, p, p, None, p, p, None, p, p, None, 1, 4, 4, p, need - 1, s) == ERR_WORKSPACE
    assert raw.rpe_aux_head_bwd_det(f32, p, 4, p, p, None, p, p, None, p, p, None, 1, 4, 4, None, need, s) == ERR_WORKSPACE
    assert raw.rpe_aux_head_bwd_det_y(f32, p, 4, p, p, p, p, None, p, p, p, p, None, 1, 4, 4, p, need - 1, s) == ERR_WORKSPACE
    assert b"aux_head_bwd_det_y" in raw.rpe_last_error()
    torch.cuda.synchronize()
    assert bool((buf == SENT).all()), "a refused call launched a kernel"
