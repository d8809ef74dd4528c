"""The fused BN-backward epilogue of the conv data gradient (rpe_conv2d_dgrad_bn, bn_mode 1 .. 5 of nt_kernel), called directly through
the C ABI into buffers the test owns and held to the fp64 references and bounds of tests/_dgrad_bn_bounds.py (built on the device from
the operands the kernel reads), on the cases of tests/_dgrad_bn_cases.py.  Per case and mode:

- dz element by element, the column totals of both partial sums, and on the 1x1 / stride-1 shapes every partial row against its own
  128 rows;
- dz and the partial sums are prefilled with NaN, the partial sums carry 4 guard rows: every row rpe_conv2d_dgrad_stats_tiles promises
  is finite in every column, every guard row is still NaN, no NaN is left in dz;
- modes 1 (no residual), 2 and 4 of one forward give the same bits; mode 3's dz is bitwise rpe_conv2d_dgrad's; mode 5's dz is bitwise
  mode 4's, its first halves are the sums of the stored dz and its second halves compare equal to 0;
- a second call and a call under the other walk direction reproduce every bit;
- rpe_last_kernel_name shows the form the shape is here for (dense / gathered / halo, and the mode), so that a shape that falls back
  fails loudly instead of testing another kernel.

The bounds and the faults they reject are judged on the CPU by tests/test_dgrad_bn_cpu.py."""
import ctypes

import pytest
import torch

import _bounds as B
import _dgrad_bn_bounds as DB
import _dgrad_bn_cases as C

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from rgb_proprioceptive_pose_estimator_amd import ops

DEV = "cuda"
GUARD_ROWS = 4
ERR_ALIGN = 3                        # include/rpe_hip.h
MODE_DENSE, MODE_CONV, MODE_HALO = 0, 1, 3          # csrc/igemm.h


def _L():
    from rgb_proprioceptive_pose_estimator_amd import _lib
    return _lib


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _device_case(c):
    """the case's tensors on the device, in the layouts the ABI reads: dy NHWC, w [in_c][k][k][out_c]"""
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()}
    d["dy_nhwc"] = d["dy"].permute(0, 2, 3, 1).contiguous()
    d["w_crsk"] = d["w"].permute(1, 2, 3, 0).contiguous()
    return d


def _desc(shape):
    b, h, w, ci, co, k, s, p = shape
    return _L().ConvDesc(b, h, w, ci, co, k, k, s, p)


def _launch(d, mode, fwd, raw=False):
    """one rpe_conv2d_dgrad_bn call -> (dz [rows, in_c], stats_part with its guard rows [T + 4, 2, in_c], T, kernel name | status)"""
    lib = _L()
    shape, ci = d["shape"], d["y"].shape[1]
    desc = _desc(shape)
    code = ops.dtype_code(d["dtype"])
    tiles = int(lib.lib.rpe_conv2d_dgrad_stats_tiles(ctypes.byref(desc), code))
    st = torch.full((tiles + GUARD_ROWS, 2, ci), float("nan"), dtype=torch.float32, device=DEV)
    dz = torch.full((d["rows"], ci), float("nan"), dtype=d["dtype"], device=DEV)
    y = None if mode == 5 else d["y"]
    stat = (None, None) if mode == 5 else (d["mean"], d["invstd"])
    a_out = fwd["a_out"] if mode == 1 else None
    sc, sh = (d["scale"], d["shift"]) if mode == 2 else (None, None)
    mask = fwd["mask"] if mode in (4, 5) else None
    ep = lib.BnBwdEpilogue(*(None if t is None else t.data_ptr() for t in (y, a_out, stat[0], stat[1], sc, sh, st, mask)))
    fn = (lib.raw if raw else lib.lib).rpe_conv2d_dgrad_bn
    rc = fn(ctypes.byref(desc), code, _P(d["dy_nhwc"]), _P(d["w_crsk"]), _P(dz), _P(d["addend"]), ctypes.byref(ep), _S())
    torch.cuda.synchronize()
    return dz, st, tiles, (rc if raw else ops.last_kernel_name())


def _kernel_fields(name):
    """nt_kernel<type, WAVES_M, BN, KCH, MODE, NST, ROLE, bn_mode> -> (MODE, bn_mode)"""
    assert name.startswith("nt_kernel<"), name
    f = name[name.index("<") + 1:name.rindex(">")].split(",")
    return int(f[4]), int(f[7])


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.name)
@pytest.mark.parametrize("path,shape", C.SHAPES, ids=["%s-%s" % (p, "x".join(map(str, s))) for p, s in C.SHAPES])
def test_fused_epilogue_within_fp64_bounds(path, shape, dtype):
    c = C.case(shape, dtype)
    d = _device_case(c)
    ci = shape[3]
    fwds = {res: C.forward(d, res, ops) for res in (False, True)}
    r = DB.conv_ref(d, DEV)                                  # the fp64 data gradient: once per case, shared by every mode
    want_mode = MODE_DENSE if C.is_dense(shape) else MODE_HALO if C.is_halo(shape, dtype) else MODE_CONV
    results = {}
    for mode, res in C.variants(shape, dtype):
        label = "dgrad_bn | %s | mode %d%s | %s | %s" % (path, mode, "r" if res else "", C.name(dtype), "x".join(map(str, shape)))
        fwd = fwds[res]
        dz, st, tiles, kname = _launch(d, mode, fwd)
        results[(mode, res)] = (dz, st)
        # the kernel form this row of the table is here for
        assert _kernel_fields(kname) == (want_mode, mode), "%s: launched %s, expected staging mode %d, bn_mode %d" % (label, kname, want_mode, mode)
        if C.is_parity(shape) and not C.is_dense(shape):
            assert tiles == C.parity_rows(shape), "%s: %d partial rows, the parity-class form has %d" % (label, tiles, C.parity_rows(shape))
        # rows written
        assert bool(torch.isfinite(st[:tiles]).all()), "%s: a promised partial row was not written (rows %s)" % (
            label, sorted(set((~torch.isfinite(st[:tiles])).nonzero()[:, 0].tolist())))
        assert bool(torch.isnan(st[tiles:]).all()), "%s: a guard row behind the %d promised partial rows was written" % (label, tiles)
        assert not bool(torch.isnan(dz.float()).any()), "%s: dz has elements the kernel never wrote" % label
        # bounds
        part = st[:tiles]
        checks, und = DB.judge(d, mode, fwd, dz, part, r=r, dev=DEV)
        if mode == 2:
            print("UNDECIDED %-60s %.3g" % (label, und))
            assert und <= C.UNDECIDED_CAP
        for qn, got, ref, bnd, layout in checks:
            B.assert_within(got, ref, bnd, "%s | %s" % (label, qn), layout)
        if mode == 5:
            assert DB.exact_zero(part), "%s: the second half of a partial row is not 0" % label
        # determinism, walk direction
        dz2, st2, _, _ = _launch(d, mode, fwd)
        assert _same(dz, dz2) and _same(st, st2), "%s: a second call does not reproduce the bits" % label
        try:
            ops.set_walk_direction(1)
            dz3, st3, _, _ = _launch(d, mode, fwd)
        finally:
            ops.set_walk_direction(0)
        assert _same(dz, dz3) and _same(st, st3), "%s: the walk direction changed a result" % label
    # mode agreement: one forward, three ways to its gate
    ref_dz, ref_st = results[(1, False)]
    for m in (2, 4):
        if (m, False) in results:
            assert _same(results[(m, False)][0], ref_dz), "%s %s %s: mode %d's dz differs from mode 1's" % (path, shape, dtype, m)
            assert _same(results[(m, False)][1], ref_st), "%s %s %s: mode %d's partial sums differ from mode 1's" % (path, shape, dtype, m)
    if (4, True) in results:
        assert _same(results[(4, True)][0], results[(1, True)][0]) and _same(results[(4, True)][1], results[(1, True)][1])
    for res in (False, True):
        if (5, res) in results:
            assert _same(results[(5, res)][0], results[(4, res)][0]), "%s %s %s: mode 5's dz differs from mode 4's" % (path, shape, dtype)
    b, h, w = shape[:3]
    plain = ops.conv2d_dgrad(d["dy_nhwc"], d["w_crsk"], (b, h, w, ci), shape[6], shape[7], addend=None if d["addend"] is None else d["addend"].view(b, h, w, ci))
    assert _same(results[(3, False)][0], plain.view(-1, ci)), "%s %s %s: mode 3's dz is not rpe_conv2d_dgrad's" % (path, shape, dtype)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.name)
def test_in_c_not_a_multiple_of_8_is_refused(dtype):
    """the epilogue moves whole 8-channel chunks: a width that would need its element-wise tail is refused before any launch, and
    nothing is written"""
    c = C.case(C.TAIL_SHAPE[1], dtype)
    d = _device_case(c)
    fwd = {"a_out": C.forward(c, False)["a_out"].to(DEV)}     # (a torch statement: the BN kernels need whole chunks as well)
    for mode in (1, 2, 3):
        dz, st, tiles, rc = _launch(d, mode, fwd, raw=True)
        assert rc == ERR_ALIGN, "mode %d: status %d" % (mode, rc)
        assert bool(torch.isnan(dz.float()).all()) and bool(torch.isnan(st).all())
