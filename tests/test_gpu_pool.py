"""The pooling and stem-backward kernels of csrc/norm.hip, each entry point called directly through the C ABI and held element by element
to the fp64 references and bounds of tests/_pool_bounds.py (built on the device from the operands the kernel reads), on the cases of
tests/_pool_cases.py: rpe_maxpool3x3s2_fwd (value bit for bit, every winner tap; ties, NaN and -inf windows, odd sizes), its backward
(with and without the addend, rounded once, unnamed pixels exact), rpe_bn_apply_maxpool3x3s2 (bit for bit the two passes, both walk
directions), rpe_stem_bwd (every row-pass count, block shape and slice count of its launcher, the three aux forms, the dpart contract),
rpe_avgpool_fwd / _bwd (both kernels, on either side of the switch) and the shapes an entry point must refuse.  Every output is
prefilled with a sentinel and carries sentinels behind it.  The bounds and the faults they reject are judged on the CPU by
tests/test_pool_cpu.py.

Deliberately not tested: the grid-stride tail behind ew_grid's cap of 2^20 blocks, which needs 2^28 chunks (4 GiB per tensor)."""
import ctypes

import pytest
import torch

import _bounds as B
import _pool_bounds as PB
import _pool_cases as C

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from rgb_proprioceptive_pose_estimator_amd import ops

DEV = "cuda"
F32 = torch.float32
SENT = -12345.5
IDX_SENT = 0xA5
ERR_SHAPE, ERR_WORKSPACE = 1, 5      # include/rpe_hip.h
G = C.GUARD


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


def _dev(case):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in case.items()}


def _out(n, dtype=F32):
    """n elements for the kernel and G sentinels behind them, all prefilled"""
    return torch.full((n + G,), SENT, dtype=dtype, device=DEV)


def _idx_out(n):
    return torch.full((n + G,), IDX_SENT, dtype=torch.uint8, device=DEV)


def _untouched(t, n=0):
    """the elements of t from n on still hold the sentinel"""
    fill = IDX_SENT if t.dtype == torch.uint8 else SENT
    return _same_bits(t[n:], torch.full_like(t[n:], fill))


def _stored(got, ref, bnd, dtype, label):
    """an output in the compute type: within its bound, rounded once, unbiased (where the case is large enough to tell)"""
    B.assert_within(got, ref, bnd, label)
    B.assert_rounds_once(got, ref, dtype, label, bnd)
    B.assert_unbiased(got, ref, dtype, label, bnd)


def _same_values(got, ref):
    """bit for bit; where the reference is a NaN, a NaN"""
    nan = torch.isnan(ref)
    return bool((torch.isnan(got) == nan).all()) and bool((_bits(got) == _bits(ref))[~nan].all())


# ------------------------------------------------------------------ max pool
def _maxpool_fwd(dtype, x):
    b, h, w, c = x.shape
    n = b * C.pooled(h) * C.pooled(w) * c
    out, idx = _out(n, dtype), _idx_out(n)
    _lib().rpe_maxpool3x3s2_fwd(ops.dtype_code(dtype), _P(x), _P(out), _P(idx), b, h, w, c, _S())
    assert _untouched(out, n) and _untouched(idx, n), "maxpool_fwd wrote behind an output"
    shape = (b, C.pooled(h), C.pooled(w), c)
    return out[:n].view(shape), idx[:n].view(shape)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
@pytest.mark.parametrize("k", range(6))
def test_maxpool_forward(dtype, k):
    """rpe_maxpool3x3s2_fwd: the value bit for bit, the winner tap on every element (torch's rule: test_pool_cpu.py)"""
    shape = C.maxpool_shapes(dtype)[k]
    for kind in C.MAXPOOL_KINDS:
        label = "%s %s %s" % (_name(dtype), shape, kind)
        d = C.maxpool_case(dtype, shape, kind)
        x = d["x"].to(DEV)
        out, idx = _maxpool_fwd(dtype, x)
        ref_out, ref_idx = PB.maxpool_ref(x)
        assert _same_values(out, ref_out), "%s: %d pooled values differ" % (label, int((_bits(out) != _bits(ref_out)).sum()))
        bad = int((idx != ref_idx).sum())
        assert bad == 0, "%s: %d of %d winner taps differ, first at %s" % (label, bad, idx.numel(), torch.nonzero(idx != ref_idx)[0].tolist())
        for (bb, oh, ow, ch), tap in d["expect"].items():
            assert int(idx[bb, oh, ow, ch]) == tap, "%s: constructed window %s names tap %d, not %d" % (label, (bb, oh, ow, ch), int(idx[bb, oh, ow, ch]), tap)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
@pytest.mark.parametrize("k", range(6))
def test_maxpool_backward(dtype, k):
    """rpe_maxpool3x3s2_bwd on the reference forward's winners, with and without the addend: within the bound of its fp32 sum, rounded
    once; a pixel no window names holds the addend (or +0) bit for bit"""
    shape = C.maxpool_shapes(dtype)[k]
    b, h, w, c = shape
    n = b * h * w * c
    for kind in C.MAXPOOL_KINDS:
        d = _dev(C.maxpool_case(dtype, shape, kind))
        idx = PB.maxpool_ref(d["x"])[1].contiguous()
        for addend in (None, d["addend"]):
            label = "%s %s %s addend=%d" % (_name(dtype), shape, kind, addend is not None)
            dx = _out(n, dtype)
            _lib().rpe_maxpool3x3s2_bwd(ops.dtype_code(dtype), _P(d["dout"]), _P(idx), _P(addend), _P(dx), b, h, w, c, _S())
            assert _untouched(dx, n), label + ": wrote behind dx"
            got = dx[:n].view(b, h, w, c)
            ref, bnd, named = PB.maxpool_bwd_ref(d["dout"], idx, addend, (h, w), dtype)
            _stored(got, ref, bnd, dtype, "pool bwd " + label)
            base = torch.zeros_like(got) if addend is None else addend
            bad = int((_bits(got) != _bits(base))[~named].sum())
            assert bad == 0, "%s: %d pixels that no window names differ from the addend" % (label, bad)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
def test_fused_bn_apply_maxpool(dtype):
    """rpe_bn_apply_maxpool3x3s2: a, out and idx are bit for bit rpe_bn_apply followed by rpe_maxpool3x3s2_fwd, out and idx are the
    reference forward of that a, and both walk directions give the same bits"""
    lib, code = _lib(), ops.dtype_code(dtype)
    for shape in C.fused_shapes(dtype):
        label = "%s %s" % (_name(dtype), shape)
        b, h, w, c = shape
        d = _dev(C.fused_case(dtype, shape))
        n, no = b * h * w * c, b * (h // 2) * (w // 2) * c
        a2 = _out(n, dtype)
        lib.rpe_bn_apply(code, _P(d["y"]), None, _P(a2), _P(d["scale"]), _P(d["shift"]), b * h * w, c, 1, _S())
        assert _untouched(a2, n), label + ": bn_apply wrote behind its output"
        a2 = a2[:n].view(b, h, w, c)
        out2, idx2 = _maxpool_fwd(dtype, a2)
        ref_out, ref_idx = PB.maxpool_ref(a2)
        got = []
        for mode in (0, 1):
            a, out, idx = _out(n, dtype), _out(no, dtype), _idx_out(no)
            ops.set_walk_direction(mode)
            try:
                lib.rpe_bn_apply_maxpool3x3s2(code, _P(d["y"]), _P(d["scale"]), _P(d["shift"]), _P(a), _P(out), _P(idx), b, h, w, c, _S())
            finally:
                ops.set_walk_direction(0)
            assert _untouched(a, n) and _untouched(out, no) and _untouched(idx, no), "%s walk %d: wrote behind an output" % (label, mode)
            got.append((a[:n].view(b, h, w, c), out[:no].view(out2.shape), idx[:no].view(idx2.shape)))
        a, out, idx = got[0]
        assert _same_bits(a, a2) and _same_bits(out, out2) and torch.equal(idx, idx2), label + ": the fused pass is not bitwise the two passes"
        assert _same_bits(out, ref_out) and torch.equal(idx, ref_idx), label + ": the fused pass is not the reference forward of its a"
        assert all(_same_bits(p, q) for p, q in zip(got[0], got[1])), label + ": walking downwards changes the result"


# ------------------------------------------------------------------ stem backward
def _stem_bwd(dtype, d, shape, lib, part_floats=None, **override):
    """-> (status, dict of the prefilled outputs, part, dpart); override replaces operands / extents (the refusals)"""
    b, h, w, pf = shape
    pf = pf if part_floats is None else part_floats
    n = b * h * w * 64
    o = dict(dgamma=_out(64), dbeta=_out(64), c1c2=_out(128), dy=_out(n, dtype))
    part = torch.full((shape[3] + G,), float("nan"), device=DEV)       # a block partial read before it is written shows
    part[shape[3]:] = SENT
    dpart = torch.full((C.DPART_DOUBLES,), float("nan"), dtype=torch.float64, device=DEV)
    dpart[:64] = 0.0
    a = dict(d, B=b, H=h, W=w)
    a.update(override)
    rc = lib.rpe_stem_bwd(ops.dtype_code(dtype), _P(a["dpool"]), _P(a["pool_idx"]), _P(a["y"]), _P(a["scale"]), _P(a["shift"]), _P(a["mean"]),
                          _P(a["invstd"]), _P(a["gamma"]), _P(a["aux_dout"]), a["aux_ld"], _P(a["depth_feat"]), _P(a["aux_idx"]), _P(a["aux_w"]),
                          _P(o["dgamma"]), _P(o["dbeta"]), _P(o["dy"]), a["B"], a["H"], a["W"], _P(part), pf, _P(o["c1c2"]), _P(dpart), _S())
    return rc, o, part, dpart


def _stem_again(dtype, d, shape, o, dpart):
    """a second call on the same dpart -> its outputs"""
    b, h, w, pf = shape
    o2 = dict(dgamma=_out(64), dbeta=_out(64), c1c2=_out(128), dy=_out(b * h * w * 64, dtype))
    part = torch.full((pf,), float("nan"), device=DEV)
    _lib().rpe_stem_bwd(ops.dtype_code(dtype), _P(d["dpool"]), _P(d["pool_idx"]), _P(d["y"]), _P(d["scale"]), _P(d["shift"]), _P(d["mean"]),
                        _P(d["invstd"]), _P(d["gamma"]), _P(d["aux_dout"]), d["aux_ld"], _P(d["depth_feat"]), _P(d["aux_idx"]), _P(d["aux_w"]),
                        _P(o2["dgamma"]), _P(o2["dbeta"]), _P(o2["dy"]), b, h, w, _P(part), pf, _P(o2["c1c2"]), _P(dpart), _S())
    return o2


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
@pytest.mark.parametrize("aux", C.STEM_AUX)
@pytest.mark.parametrize("k", range(5))
def test_stem_backward(dtype, aux, k):
    """rpe_stem_bwd: dbeta, dgamma, c1, c2 within the bounds of their block sums, dy within its bound and rounded once (round_T(k1 +
    k2 y) wherever the mask or the winners leave no gradient), nothing written behind an output or the partial sums, the arrival
    counters left zero, a second call on the same dpart giving the same bits"""
    shape = C.STEM_SHAPES[k]
    b, h, w, pf = shape
    n = b * h * w * 64
    label = "%s %s %s" % (_name(dtype), shape, aux)
    d = _dev(C.stem_case(dtype, shape, aux))
    geo = C.stem_geometry(b, h, w, pf, dtype)
    rc, o, part, dpart = _stem_bwd(dtype, d, shape, _lib())
    assert _untouched(part, pf), label + ": wrote behind the partial-sum workspace"
    assert bool(torch.isnan(part[geo["nb"] * 128:pf]).all()) and bool(torch.isfinite(part[:geo["nb"] * 128]).all()), \
        label + ": the reduce pass did not write exactly its %d blocks' partial sums" % geo["nb"]
    assert bool((_bits(dpart[:64]) == 0).all()), label + ": the first 64 doubles of dpart are not left zero"
    for name, t in o.items():
        assert _untouched(t, n if name == "dy" else 128 if name == "c1c2" else 64), "%s: wrote behind %s" % (label, name)
    o2 = _stem_again(dtype, d, shape, o, dpart)
    assert bool((_bits(dpart[:64]) == 0).all()), label + ": the first 64 doubles of dpart are not left zero (second call)"
    for name in o:
        assert _same_bits(o[name], o2[name]), "%s: %s differs between two calls on one dpart" % (label, name)
    r = PB.stem_ref(d, geo["rpb"], dtype)
    und = int(r["undecided"].sum())
    print("UNDECIDED %-40s %d of %d" % (label, und, n))
    assert und <= 1e-3 * n, "%s: %d undecided elements" % (label, und)
    lay = "i"
    B.assert_within(o["dbeta"][:64], *r["dbeta"].out(), "stem dbeta " + label, lay)
    B.assert_within(o["dgamma"][:64], *r["dgamma"].out(), "stem dgamma " + label, lay)
    B.assert_within(o["c1c2"][:64], *r["c1"].out(), "stem c1 " + label, lay)
    B.assert_within(o["c1c2"][64:128], *r["c2"].out(), "stem c2 " + label, lay)
    dy = o["dy"][:n].view(b, h, w, 64)
    ref, bnd = r["dy"]
    if und == 0:
        _stored(dy, ref, bnd, dtype, "stem dy " + label)
    else:
        dec = ~r["undecided"]
        B.assert_within(dy[dec], ref[dec], bnd[dec], "stem dy (decided) " + label, lay)
        B.assert_rounds_once(dy[dec], ref[dec], dtype, "stem dy (decided) " + label, bnd[dec])
    off = r["off"]
    zb, zh, zw, zc = d["zero"]
    assert bool(off[zb, zh, zw, zc]), label + ": the constructed +0 is not off"
    B.assert_within(dy[off], r["plain"][0][off], r["plain"][1][off], "stem dy off " + label, lay)


# ------------------------------------------------------------------ average pool
@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
@pytest.mark.parametrize("k", range(9))
def test_average_pool(dtype, k):
    """rpe_avgpool_fwd (both kernels: (32, 16, 2048) and (33, 16, 2048) lie on either side of the switch) and rpe_avgpool_bwd"""
    shape = C.avgpool_bwd_shapes(dtype)[k]
    b, hw, c = shape
    label = "%s %s" % (_name(dtype), shape)
    d = _dev(C.avgpool_case(dtype, shape))
    code = ops.dtype_code(dtype)
    if shape in C.avgpool_shapes(dtype):
        out = _out(b * c)
        _lib().rpe_avgpool_fwd(code, _P(d["x"]), _P(out), b, hw, c, _S())
        assert _untouched(out, b * c), label + ": avgpool_fwd wrote behind its output"
        B.assert_within(out[:b * c].view(b, c), *PB.avgpool_ref(d["x"]), "avgpool fwd %s few=%d" % (label, C.avgpool_few(b, hw, c)), "rc")
    n = b * hw * c
    dx = _out(n, dtype)
    _lib().rpe_avgpool_bwd(code, _P(d["dout"]), _P(dx), b, hw, c, _S())
    assert _untouched(dx, n), label + ": avgpool_bwd wrote behind dx"
    ref, bnd = PB.avgpool_bwd_ref(d["dout"], hw, dtype)
    _stored(dx[:n].view(b, hw, c), ref, bnd, dtype, "avgpool bwd " + label)


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
def test_pool_entry_points_refuse_malformed_shapes(dtype):
    """B = 0, HW = 0 and a channel count that is no whole number of 16-byte chunks: RPE_ERR_SHAPE from all four pool entry points,
    nothing written.  The empty batch goes first: it is harmless on any library, and a library that accepts it has no argument checks
    -- the test stops there and never launches a kernel on a truncated channel count.  Buffers are sized for the next whole chunk
    count."""
    raw, code = _raw(), ops.dtype_code(dtype)
    ce = C.CE[dtype]
    bad_c = C.refused_channels(dtype)
    cw = (bad_c + ce - 1) // ce * ce
    b, h, w = 2, 4, 4
    x = torch.full((b * h * w * cw + G,), SENT, dtype=dtype, device=DEV)
    o = torch.full((b * h * w * cw + G,), SENT, dtype=dtype, device=DEV)
    of = _out(b * cw)
    idx = _idx_out(b * h * w * cw)

    def calls(bb, hh, ww, cc):
        return [("maxpool_fwd", lambda: raw.rpe_maxpool3x3s2_fwd(code, _P(x), _P(o), _P(idx), bb, hh, ww, cc, _S())),
                ("maxpool_bwd", lambda: raw.rpe_maxpool3x3s2_bwd(code, _P(x), _P(idx), None, _P(o), bb, hh, ww, cc, _S())),
                ("avgpool_fwd", lambda: raw.rpe_avgpool_fwd(code, _P(x), _P(of), bb, hh * ww, cc, _S())),
                ("avgpool_bwd", lambda: raw.rpe_avgpool_bwd(code, _P(of), _P(o), bb, hh * ww, cc, _S()))]
    for what, (bb, hh, ww, cc) in (("B = 0", (0, h, w, cw)), ("HW = 0", (b, 0, 0, cw)), ("C = %d" % bad_c, (b, h, w, bad_c)), ("C = 0", (b, h, w, 0))):
        for name, call in calls(bb, hh, ww, cc):
            rc = call()
            assert rc == ERR_SHAPE, "%s %s %s: status %d, not RPE_ERR_SHAPE (%s)" % (_name(dtype), name, what, rc, raw.rpe_last_error())
    torch.cuda.synchronize()
    assert _untouched(o) and _untouched(of) and _untouched(idx), "a refused call wrote to an output"


@pytest.mark.parametrize("dtype", C.DTYPES, ids=_name)
def test_stem_backward_refusals(dtype):
    """odd H, aux_dout without aux_idx: RPE_ERR_SHAPE; 127 floats of partial sums: RPE_ERR_WORKSPACE; nothing written"""
    shape = C.STEM_SHAPES[4]
    d = _dev(C.stem_case(dtype, shape, "aux"))
    for what, want, kw in (("odd H", ERR_SHAPE, dict(override=dict(H=shape[1] - 1))),
                           ("aux_dout without aux_idx", ERR_SHAPE, dict(override=dict(aux_idx=None))),
                           ("127 floats of partial sums", ERR_WORKSPACE, dict(part_floats=127))):
        rc, o, part, dpart = _stem_bwd(dtype, d, shape, _raw(), kw.get("part_floats"), **kw.get("override", {}))
        torch.cuda.synchronize()
        assert rc == want, "%s %s: status %d, not %d" % (_name(dtype), what, rc, want)
        assert all(_untouched(t) for t in o.values()), "%s %s: a refused call wrote to an output" % (_name(dtype), what)
        assert bool(torch.isnan(part[:shape[3]]).all()) and _untouched(part, shape[3]) and bool(torch.isnan(dpart[64:]).all()) \
            and bool((_bits(dpart[:64]) == 0).all()), "%s %s: a refused call wrote to a workspace" % (_name(dtype), what)
