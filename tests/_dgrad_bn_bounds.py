"""fp64 reference, with element-wise bounds, of the fused BN-backward epilogue of the conv data gradient (rpe_conv2d_dgrad_bn:
bn_mode 1 .. 5 of nt_kernel, csrc/igemm_impl.h).

Everything is computed from the operands the kernel reads, on their device, and built from tests/_bounds.py and tests/_norm_bounds.py
as they stand -- bound (LAM, EPI), sum_bound, Fx (EW), U_OUT, FLOOR -- with no further constant:

- dz = (acc + addend) gate, acc the fp64 data gradient (conv_dgrad_ref): bound(r, dtype, out = dz, epi = |acc| + |addend|), the form
  test_y3_free_bottleneck_backward uses for mode 5.  A gated-off element has reference 0 and must be within the ungated value's
  accumulation share of it: the kernel writes +0 there;
- gate: a_out > 0 on the stored values (mode 1), the mask bits as given (4, 5), all ones (3).  Mode 2 recomputes it as
  fmaf(y, scale, shift) > 0, so the sign of the fp64 pre-activation decides wherever |pre| exceeds the fp32 evaluation's slack
  (_norm_bounds.apply_ref); the few elements inside it (expected share ~1e-6, at most _dgrad_bn_cases.UNDECIDED_CAP) may fall either
  way and take the gate the judged dz itself shows (dz != 0);
- sum dz (the first half of a partial row): the kernel adds the UNROUNDED fp32 values, so the elements carry eb, the fp32 form of
  their bound (bound(r, float32, ...)), where the gate is open and nothing where it is closed: sum_bound(dz, eb gate);
- sum dz xhat (the second half): the kernel's expression is fmaf(dz, fmaf(y, inv, -(mean inv)), .).  The term is carried as
  Fx(dz, eb gate) (Fx(y) Fx(inv) + (-(Fx(mean) Fx(inv)))), so |y inv| and |mean inv| enter the error separately (where the mean is
  many sigma the two cancel in xhat and the error does not): sum_bound(term.v, term.e).  This is _norm_bounds.reduce_ref's construction
  with the cancellation made explicit;
- mode 5 has no y: the first half is the sum of dz AS STORED (rounded to the type), so the stored tensor summed in fp64 is the
  reference and the elements carry no error of their own, sum_bound(stored, 0); the second half is exactly +0;
- the checks are on the column totals over all partial rows (added in fp64 from the fp32 rows).  Which rows a partial row covers is a
  contract for the 1x1 / stride-1 form only ("per-128-row-tile partial sums", include/rpe_hip.h): there row t is also held against
  rows [128 t, 128 t + 128) alone, sum_bound on that slice -- a half written to the wrong row does not change the total.

tests/test_dgrad_bn_cpu.py holds a torch-fp32 restatement of the epilogue to <= 0.5 of each of these, and shows the faults they reject."""
import torch

import _bounds as B
import _dgrad_bn_cases as C
import _norm_bounds as NB
from _bounds import Fx

ROWS = C.STATS_ROWS


def conv_ref(c, dev):
    """the fp64 data gradient of case c as rows: Ref with acc, Q [rows, in_c]"""
    b, h, w, ci, co, k, s, p = c["shape"]
    d64 = lambda t: t.to(dev).double()
    if C.is_dense(c["shape"]):
        return B.gemm_ref(d64(c["dy"]).permute(0, 2, 3, 1).reshape(-1, co), d64(c["w"]).reshape(co, ci).t())
    r = B.conv_dgrad_ref(d64(c["dy"]), d64(c["w"]), (h, w), s, p)
    return B.Ref(r.acc.reshape(-1, ci), r.Q.reshape(-1, ci), r.K)


def gate_ref(c, mode, fwd, dz_got, dev):
    """-> (gate [rows, in_c] bool, share of undecided elements).  dz_got: the judged dz (only mode 2's undecided elements look at it)"""
    y = c["y"].to(dev)
    if mode == 1:
        return fwd["a_out"].to(dev).double() > 0, 0.0
    if mode in (4, 5):
        return fwd["bits"].to(dev), 0.0
    if mode == 3:
        return torch.ones(y.shape, dtype=torch.bool, device=dev), 0.0
    a = NB.apply_ref(y, c["scale"].to(dev), c["shift"].to(dev), None, None, None, True, c["dtype"])
    und = a["pre"].abs() <= a["slack"]
    gate = a["pre"] > 0
    if dz_got is not None:
        gate = torch.where(und, dz_got.to(dev).double().reshape(gate.shape) != 0, gate)
    return gate, float(und.double().mean())


def dz_ref(c, r, gate, dev):
    """-> dict(ref, bnd (in the compute type), eb (the fp32 form, zero where the gate is closed))"""
    add = 0.0 if c["addend"] is None else c["addend"].to(dev).double()
    g = gate.double()
    ref = (r.acc + add) * g
    epi = r.acc.abs() + (add.abs() if torch.is_tensor(add) else 0.0)
    return dict(ref=ref, bnd=B.bound(r, c["dtype"], out=ref, epi=epi), eb=B.bound(r, torch.float32, out=ref, epi=epi) * g)


def _tiles(v, e):
    """per-128-row slices: (sums [T, C], sum_bound of each slice [T, C])"""
    n = v.shape[0]
    sl = [slice(i, min(i + ROWS, n)) for i in range(0, n, ROWS)]
    return torch.stack([v[s].sum(0) for s in sl]), torch.stack([B.sum_bound(v[s], e[s]) for s in sl])


def sums_ref(c, d, dev, tiles=False):
    """-> {s1, s2: (reference [C], bound [C])} of the column totals of dz and dz xhat; with tiles also {t1, t2: ([T, C], [T, C])}"""
    y, mean, inv = c["y"].to(dev).double(), c["mean"].to(dev).double(), c["invstd"].to(dev).double()
    term = Fx(d["ref"], d["eb"]) * (Fx(y) * Fx(inv) + (-(Fx(mean) * Fx(inv))))
    out = dict(s1=(d["ref"].sum(0), B.sum_bound(d["ref"], d["eb"])), s2=(term.v.sum(0), B.sum_bound(term.v, term.e)))
    if tiles:
        out.update(t1=_tiles(d["ref"], d["eb"]), t2=_tiles(term.v, term.e))
    return out


def stored_sums_ref(dz_stored, dev, tiles=False):
    """mode 5: the stored dz summed in fp64, no element error"""
    v = dz_stored.to(dev).double().reshape(-1, dz_stored.shape[-1])
    z = torch.zeros_like(v)
    out = dict(s1=(v.sum(0), B.sum_bound(v, z)))
    if tiles:
        out["t1"] = _tiles(v, z)
    return out


def judge(c, mode, fwd, dz, part, r=None, dev="cpu", plain_rows=None):
    """Every bound check of one launch's results as a list of (quantity, got, ref, bnd, layout), and the undecided share.
    dz [rows, in_c] as stored, part [T, 2, in_c] fp32 (the promised rows only).  plain_rows: whether partial row t covers rows
    [128 t, 128 t + 128) (default: the 1x1 / stride-1 shapes).  Mode 5's second half is not a bound: see exact_zero."""
    ci = c["y"].shape[1]
    plain = C.is_dense(c["shape"]) if plain_rows is None else plain_rows
    r = conv_ref(c, dev) if r is None else r
    dz = dz.to(dev).reshape(-1, ci)
    p64 = part.to(dev).double()
    gate, und = gate_ref(c, mode, fwd, dz, dev)
    d = dz_ref(c, r, gate, dev)
    out = [("dz", dz, d["ref"], d["bnd"], "rc")]
    if mode == 5:
        s = stored_sums_ref(dz, dev, plain)
        out.append(("sum dz", p64[:, 0].sum(0), s["s1"][0], s["s1"][1], "c"))
        if plain:
            out.append(("tile sum dz", p64[:, 0], s["t1"][0], s["t1"][1], "tc"))
        return out, und
    s = sums_ref(c, d, dev, plain)
    out.append(("sum dz", p64[:, 0].sum(0), s["s1"][0], s["s1"][1], "c"))
    out.append(("sum dz xhat", p64[:, 1].sum(0), s["s2"][0], s["s2"][1], "c"))
    if plain:
        out.append(("tile sum dz", p64[:, 0], s["t1"][0], s["t1"][1], "tc"))
        out.append(("tile sum dz xhat", p64[:, 1], s["t2"][0], s["t2"][1], "tc"))
    return out, und


def exact_zero(part):
    """mode 5: the second half of every partial row compares equal to 0"""
    return bool((part[:, 1] == 0).all())
