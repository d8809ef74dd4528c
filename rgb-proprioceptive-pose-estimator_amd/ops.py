"""Thin tensor-level wrappers over the C ABI (include/rpe_hip.h).

PyTorch is used for device memory and streams only: every function here allocates its
outputs with torch.empty on the input's device, passes raw device pointers plus the
current HIP stream to librpe_hip.so, and returns the output tensors.  Activations of the
conv trunk are NHWC tensors ([B, H, W, C], contiguous) in fp32 or bf16.
"""
import ctypes
import math
import os

import torch

from ._lib import PARAM_STATS_COLS, PARAM_STATS_PART_COLS, RPE_BF16, RPE_F16, RPE_F32, BnBwdEpilogue, ConvDesc, lib

_DT = {torch.float32: RPE_F32, torch.bfloat16: RPE_BF16, torch.float16: RPE_F16}


def dtype_code(t):
    try:
        return _DT[t if isinstance(t, torch.dtype) else t.dtype]
    except KeyError:
        raise TypeError("unsupported compute dtype %r (fp32, bf16 or fp16)" % (t,))


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("librpe_hip ops need device tensors (got a CPU tensor): the HIP path has no CPU fallback")
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, name):
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def pad4(n):
    return (n + 3) // 4 * 4


def conv_desc(x_shape, out_c, k, stride, pad):
    b, h, w, c = x_shape
    return ConvDesc(b, h, w, c, out_c, k, k, stride, pad)


def conv_out_hw(d):
    return (d.in_h + 2 * d.pad - d.kh) // d.stride + 1, (d.in_w + 2 * d.pad - d.kw) // d.stride + 1


def stats_tiles(rows):
    return (rows + 127) // 128


def conv2d_fwd(x, w_krsc, stride, pad, want_stats=False):
    """x [B,H,W,Ci], w_krsc [Co,kh,kw,Ci] (same dtype) -> y [B,Ho,Wo,Co] (+ stats partials [tiles,2,Co] fp32)."""
    _chk(x, "x"), _chk(w_krsc, "w")
    co, k = w_krsc.shape[0], w_krsc.shape[1]
    d = conv_desc(x.shape, co, k, stride, pad)
    ho, wo = conv_out_hw(d)
    y = torch.empty((x.shape[0], ho, wo, co), dtype=x.dtype, device=x.device)
    st = None
    if want_stats:
        st = torch.empty((lib.rpe_conv2d_fwd_stats_tiles(ctypes.byref(d), dtype_code(x)), 2, co), dtype=torch.float32, device=x.device)
    lib.rpe_conv2d_fwd(ctypes.byref(d), dtype_code(x), _p(x), _p(w_krsc), _p(y), _p(st), _stream())
    return (y, st) if want_stats else y


def conv2d_fwd_affine(x, w_krsc, stride, pad, bias, addend=None, relu=True, split_k=True):
    """Inference form: relu(conv(x, w) + bias (+ addend)) in one launch (BatchNorm folded: w = weight * scale, bias = shift)."""
    _chk(x, "x"), _chk(w_krsc, "w")
    co, k = w_krsc.shape[0], w_krsc.shape[1]
    d = conv_desc(x.shape, co, k, stride, pad)
    ho, wo = conv_out_hw(d)
    out = torch.empty((x.shape[0], ho, wo, co), dtype=x.dtype, device=x.device)
    need = lib.rpe_conv2d_fwd_affine_workspace_bytes(ctypes.byref(d), dtype_code(x)) if split_k else 0
    if need > 0:   # few output tiles, long K (a rollout frame): split-K through a workspace
        ws = scratch(need, x.device)
        lib.rpe_conv2d_fwd_affine_ws(ctypes.byref(d), dtype_code(x), _p(x), _p(w_krsc), _p(out), _p(bias), _p(addend), int(relu), _p(ws), ws.numel(),
                                     _stream())
    else:
        lib.rpe_conv2d_fwd_affine(ctypes.byref(d), dtype_code(x), _p(x), _p(w_krsc), _p(out), _p(bias), _p(addend), int(relu), _stream())
    return out


def conv2d_dgrad(dy, w_crsk, x_shape, stride, pad, addend=None, sub_addend=False):
    """dy [B,Ho,Wo,Co], w_crsk [Ci,kh,kw,Co] -> dx [B,H,W,Ci] (+ addend).
    sub_addend: `addend` is a compact shortcut gradient [B,H/2,W/2,Ci] (conv1x1s2_dgrad_compact), added at the even pixels."""
    _chk(dy, "dy"), _chk(w_crsk, "w")
    ci, k, co = w_crsk.shape[0], w_crsk.shape[1], w_crsk.shape[3]
    d = conv_desc(x_shape, co, k, stride, pad)
    dx = torch.empty(tuple(x_shape), dtype=dy.dtype, device=dy.device)
    fn = lib.rpe_conv2d_dgrad_sub if sub_addend else lib.rpe_conv2d_dgrad
    fn(ctypes.byref(d), dtype_code(dy), _p(dy), _p(w_crsk), _p(dx), _p(addend), _stream())
    return dx


def conv1x1s2_dgrad_compact(dy, w_crsk, x_shape):
    """Data gradient of a 1x1 / stride-2 / pad-0 conv over even dims, on the pixels it reads alone: dy [B,H/2,W/2,Co], w_crsk [Ci,1,1,Co]
    -> [B,H/2,W/2,Ci] = rows (b, 2h', 2w') of conv2d_dgrad's dx (every other row of it is zero)."""
    _chk(dy, "dy"), _chk(w_crsk, "w")
    ci, k, co = w_crsk.shape[0], w_crsk.shape[1], w_crsk.shape[3]
    d = conv_desc(x_shape, co, k, 2, 0)
    dx = torch.empty((x_shape[0], x_shape[1] // 2, x_shape[2] // 2, ci), dtype=dy.dtype, device=dy.device)
    lib.rpe_conv1x1s2_dgrad_compact(ctypes.byref(d), dtype_code(dy), _p(dy), _p(w_crsk), _p(dx), _stream())
    return dx


def conv2d_dgrad_bn(dy, w_crsk, x_shape, stride, pad, y, mean, invstd, a_out=None, scale=None, shift=None, addend=None, a_mask=None, sub_addend=False):
    """Data gradient with the producing layer's ReLU mask and BN-backward partial sums fused into the epilogue.
    Returns (dz [B,H,W,Ci], stats partials [tiles,2,Ci]).  sub_addend: as conv2d_dgrad."""
    _chk(dy, "dy"), _chk(w_crsk, "w")
    if y is not None:   # (y = None with a_mask: the producing layer's raw output was never written -- only sum dz is emitted)
        _chk(y, "y")
    ci, k, co = w_crsk.shape[0], w_crsk.shape[1], w_crsk.shape[3]
    d = conv_desc(x_shape, co, k, stride, pad)
    dz = torch.empty(tuple(x_shape), dtype=dy.dtype, device=dy.device)
    st = torch.empty((lib.rpe_conv2d_dgrad_stats_tiles(ctypes.byref(d), dtype_code(dy)), 2, ci), dtype=torch.float32, device=dy.device)
    ep = BnBwdEpilogue(*(None if t is None else t.data_ptr() for t in (y, a_out, mean, invstd, scale, shift, st, a_mask)))
    fn = lib.rpe_conv2d_dgrad_bn_sub if sub_addend else lib.rpe_conv2d_dgrad_bn
    fn(ctypes.byref(d), dtype_code(dy), _p(dy), _p(w_crsk), _p(dz), _p(addend), ctypes.byref(ep), _stream())
    return dz, st


def conv1x1_dgrad_bn_t(dy, w_crsk, x_shape, a_prev, a_mask, addend=None):
    """The fused 1x1 data gradient with the producing layer's packed ReLU mask (sum dz only) that also leaves T = dz^T a_prev behind.
    Returns (dz [B,H,W,Ci], stats partials [tiles,2,Ci], T [Ci, P] fp32)."""
    _chk(dy, "dy"), _chk(w_crsk, "w"), _chk(a_prev, "a_prev")
    ci, co = w_crsk.shape[0], w_crsk.shape[3]
    pch = a_prev.shape[-1]
    d = conv_desc(x_shape, co, 1, 1, 0)
    dz = torch.empty(tuple(x_shape), dtype=dy.dtype, device=dy.device)
    st = torch.empty((lib.rpe_conv2d_dgrad_stats_tiles(ctypes.byref(d), dtype_code(dy)), 2, ci), dtype=torch.float32, device=dy.device)
    t_out = torch.empty((ci, pch), dtype=torch.float32, device=dy.device)
    ws = scratch(lib.rpe_conv1x1_dgrad_bn_t_workspace_bytes(ctypes.byref(d), pch), dy.device)
    ep = BnBwdEpilogue(*(None if t is None else t.data_ptr() for t in (None, None, None, None, None, None, st, a_mask)))
    lib.rpe_conv1x1_dgrad_bn_t(ctypes.byref(d), dtype_code(dy), _p(dy), _p(w_crsk), _p(dz), _p(addend), ctypes.byref(ep), _p(a_prev), pch, _p(t_out),
                               _p(ws), ws.numel(), _stream())
    return dz, st, t_out


def bn_backward_from_dz(dz, y, mean, invstd, gamma, stats_part):
    c = y.shape[-1]
    dev = y.device
    dgamma = torch.empty(c, dtype=torch.float32, device=dev)
    dbeta = torch.empty(c, dtype=torch.float32, device=dev)
    dy = torch.empty_like(y)
    c1c2 = torch.empty(2 * c, dtype=torch.float32, device=dev)
    dpart = torch.zeros(256 * 2 * c + 64, dtype=torch.float64, device=dev)  # RPE_BN_DPART_DOUBLES(c); counters start at zero
    lib.rpe_bn_backward_from_dz(dtype_code(y), _p(dz), _p(y), _p(mean), _p(invstd), _p(gamma), _p(stats_part), stats_part.shape[0], _p(dgamma),
                                _p(dbeta), _p(dy), y.numel() // c, c, _p(c1c2), _p(dpart), _stream())
    return dy, dgamma, dbeta


_SCRATCH = {}


def last_kernel_name():
    """Symbol (with its configuration) of the kernel the last implicit-GEMM / BN entry point launched from this thread."""
    return lib.rpe_last_kernel_name().decode()


def set_walk_direction(mode):
    """Walk direction of this thread's next launches of the direction-aware kernels (rpe_set_walk_direction): 0 every XCD walks its
    share of the row tiles upwards (default), 1 downwards, 2 alternating launch by launch.  Scheduling only: results do not depend on it."""
    lib.rpe_set_walk_direction(int(mode))


def scratch(nbytes, device):
    """Per-device workspace for the deterministic weight-gradient calls (per-workgroup fp32 tiles, summed in a fixed order).
    One buffer that only ever grows: consecutive calls on one stream are ordered, so they can share it -- and its address stays
    fixed, which a captured hipGraph needs.  Use one stream per device for these ops (the models do)."""
    key = (device.type, device.index)
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _SCRATCH[key] = buf
    return buf


def bn_backward_coeffs(stats_part, rows):
    """per-tile partial sums [tiles, 2, C] of (dz, dz*xhat) -> (dgamma, dbeta, c1c2 [2, C] = their means)"""
    tiles, _, c = stats_part.shape
    dev = stats_part.device
    dgamma = torch.empty(c, dtype=torch.float32, device=dev)
    dbeta = torch.empty(c, dtype=torch.float32, device=dev)
    c1c2 = torch.empty((2, c), dtype=torch.float32, device=dev)
    dpart = torch.zeros(256 * 2 * c + 64, dtype=torch.float64, device=dev)
    lib.rpe_bn_backward_coeffs(_p(stats_part), tiles, c, rows, _p(dgamma), _p(dbeta), _p(c1c2), _p(dpart), _stream())
    return dgamma, dbeta, c1c2


def bn_backward_coeffs_t(stats_part, rows, dzt_a, w, mean, invstd):
    """y3-free block: partial sums [tiles, 2, C] whose first half is sum dz, T = dz^T a_in [C, Ci] fp32 and the compute-dtype weight
    [C, Ci] -> (dgamma, dbeta, c1c2): sum dz*xhat = invstd (rowdot(T, w) - mean sum dz)"""
    tiles, _, c = stats_part.shape
    ci = w.shape[1]
    dev = stats_part.device
    dgamma = torch.empty(c, dtype=torch.float32, device=dev)
    dbeta = torch.empty(c, dtype=torch.float32, device=dev)
    c1c2 = torch.empty((2, c), dtype=torch.float32, device=dev)
    dpart = torch.zeros(256 * 2 * c + 64, dtype=torch.float64, device=dev)
    lib.rpe_bn_backward_coeffs_t(dtype_code(w), _p(stats_part), tiles, c, rows, _p(_chk(dzt_a, "dzt_a")), _p(_chk(w, "w")), ci, _p(mean), _p(invstd), _p(dgamma),
                                 _p(dbeta), _p(c1c2), _p(dpart), _stream())
    return dgamma, dbeta, c1c2


def conv1x1_wgrad_combine(dzt_a, gram_buf, w_master, gamma, invstd, mean, c1c2):
    """dW [Co, Ci] fp32 of a y3-free block's conv3: A o (T - c1 s1^T) + C' o (W S - mean s1^T), S / s1 from the forward's Gram buffer"""
    co, ci = dzt_a.shape
    d = conv_desc((1, 1, 1, ci), co, 1, 1, 0)
    dw = torch.empty((co, ci), dtype=torch.float32, device=dzt_a.device)
    lib.rpe_conv1x1_wgrad_combine(ctypes.byref(d), _p(_chk(dzt_a, "dzt_a")), _p(gram_buf), _p(_chk(w_master, "w")), _p(gamma), _p(invstd), _p(mean), _p(c1c2),
                                  _p(dw), _stream())
    return dw


def bn_backward_apply_dz(dz, y, mean, invstd, gamma, c1c2):
    dy = torch.empty_like(y)
    c = y.shape[-1]
    lib.rpe_bn_backward_apply_dz(dtype_code(y), _p(dz), _p(y), _p(mean), _p(invstd), _p(gamma), _p(c1c2), _p(dy), y.numel() // c, c, _stream())
    return dy


def bn_bwd_fold_conv1x1(w_fwd, w_dgrad, gamma, invstd, mean, c1c2):
    """w_fwd [Co, Ci], w_dgrad [Ci, Co] (compute dtype) -> (w_kcat [Ci, Co + Ci], bias [Ci] fp32): the BN backward of the conv's
    output folded into its data gradient (see include/rpe_hip.h)."""
    co, ci = w_fwd.shape
    dev = w_fwd.device
    wk = torch.empty((ci, co + ci), dtype=w_fwd.dtype, device=dev)
    bias = torch.empty(ci, dtype=torch.float32, device=dev)
    ws = scratch(lib.rpe_bn_bwd_fold_scratch_bytes(dtype_code(w_fwd), co, ci), dev)
    lib.rpe_bn_bwd_fold_conv1x1(dtype_code(w_fwd), co, ci, _p(_chk(w_fwd, "w_fwd")), _p(_chk(w_dgrad, "w_dgrad")), _p(gamma), _p(invstd), _p(mean), _p(c1c2),
                                _p(wk), _p(bias), _p(ws), ws.numel(), _stream())
    return wk, bias


def bn_bwd_fold_y_conv1x1(w_dgrad, gamma, invstd, mean, c1c2):
    """w_dgrad [Ci, Co] (compute dtype) -> (w_kcat [Ci, 2 Co], bias [Ci] fp32): the backward of the BatchNorm BEHIND a 1x1 conv whose
    output is narrow (a Bottleneck's conv1), folded into its data gradient with y itself as the second K-concatenated operand."""
    ci, co = w_dgrad.shape
    dev = w_dgrad.device
    wk = torch.empty((ci, 2 * co), dtype=w_dgrad.dtype, device=dev)
    bias = torch.empty(ci, dtype=torch.float32, device=dev)
    lib.rpe_bn_bwd_fold_y_conv1x1(dtype_code(w_dgrad), co, ci, _p(_chk(w_dgrad, "w_dgrad")), _p(gamma), _p(invstd), _p(mean), _p(c1c2), _p(wk), _p(bias), _stream())
    return wk, bias


def conv1x1_dgrad_kcat_y(dz, y, w_kcat, bias, ci, addend=None, bn=None, sub_addend=False):
    """dz, y [B,H,W,Co] -> dx [B,H,W,Ci] = [dz | y] w_kcat^T + bias (+ addend).  bn: optional dict(y, mean, invstd, a_out / a_mask, scale,
    shift) of the layer BEHIND dx (fused ReLU mask + BN-backward partial sums); then returns (dz_in, stats).  sub_addend: as conv2d_dgrad."""
    _chk(dz, "dz"), _chk(y, "y")
    b, h, w, co = dz.shape
    d = conv_desc((b, h, w, ci), co, 1, 1, 0)
    dx = torch.empty((b, h, w, ci), dtype=dz.dtype, device=dz.device)
    fn = lib.rpe_conv1x1_dgrad_kcat_y_sub if sub_addend else lib.rpe_conv1x1_dgrad_kcat_y
    if bn is None:
        fn(ctypes.byref(d), dtype_code(dz), _p(dz), _p(y), _p(w_kcat), _p(bias), _p(dx), _p(addend), None, _stream())
        return dx
    st = torch.empty((lib.rpe_conv2d_dgrad_stats_tiles(ctypes.byref(d), dtype_code(dz)), 2, ci), dtype=torch.float32, device=dz.device)
    ep = BnBwdEpilogue(*(None if t is None else t.data_ptr() for t in (bn["y"], bn.get("a_out"), bn["mean"], bn["invstd"], bn.get("scale"), bn.get("shift"), st,
                                                                      bn.get("a_mask"))))
    fn(ctypes.byref(d), dtype_code(dz), _p(dz), _p(y), _p(w_kcat), _p(bias), _p(dx), _p(addend), ctypes.byref(ep), _stream())
    return dx, st


def conv1x1_wgrad_folded_y(dz, y, x, gamma, invstd, mean, c1c2):
    """dW [Co, Ci] fp32 of a 1x1 conv with the backward of the BatchNorm behind it folded in: reads dz, y (both [.., Co]) and x ([.., Ci])."""
    _chk(dz, "dz"), _chk(y, "y"), _chk(x, "x")
    b, h, w, co = dz.shape
    ci = x.shape[3]
    d = conv_desc((b, h, w, ci), co, 1, 1, 0)
    dw = torch.empty((co, ci), dtype=torch.float32, device=dz.device)
    ws = scratch(lib.rpe_conv1x1_wgrad_folded_y_scratch_bytes(ctypes.byref(d), dtype_code(dz)), dz.device)
    lib.rpe_conv1x1_wgrad_folded_y(ctypes.byref(d), dtype_code(dz), _p(dz), _p(y), _p(x), _p(gamma), _p(invstd), _p(mean), _p(c1c2), _p(dw), _p(ws), ws.numel(),
                                   _stream())
    return dw


def conv1x1_wgrad_folded(dz, a_in, w_master, gamma, invstd, mean, c1c2):
    """dW [Co, Ci] fp32 of a 1x1 conv with its output BN's backward folded in: reads dz and the conv input only."""
    _chk(dz, "dz"), _chk(a_in, "a_in")
    b, h, w, co = dz.shape
    ci = a_in.shape[3]
    d = conv_desc((b, h, w, ci), co, 1, 1, 0)
    dw = torch.empty((co, ci), dtype=torch.float32, device=dz.device)
    ws = scratch(lib.rpe_conv1x1_wgrad_folded_scratch_bytes(ctypes.byref(d), dtype_code(dz)), dz.device)
    lib.rpe_conv1x1_wgrad_folded(ctypes.byref(d), dtype_code(dz), _p(dz), _p(a_in), _p(_chk(w_master, "w")), _p(gamma), _p(invstd), _p(mean), _p(c1c2), _p(dw),
                                 _p(ws), ws.numel(), _stream())
    return dw


def conv1x1_dgrad_kcat(dz, a_in, w_kcat, bias, bn=None):
    """dz [B,H,W,Co], a_in [B,H,W,Ci] -> dx [B,H,W,Ci].  bn: optional dict(y, mean, invstd, scale, shift, a_out, a_mask) of the
    layer BEHIND a_in (fused ReLU mask + BN-backward partial sums, as conv2d_dgrad_bn); then returns (dz_in, stats)."""
    _chk(dz, "dz"), _chk(a_in, "a_in")
    b, h, w, co = dz.shape
    ci = a_in.shape[3]
    d = conv_desc((b, h, w, ci), co, 1, 1, 0)
    dx = torch.empty_like(a_in)
    if bn is None:
        lib.rpe_conv1x1_dgrad_kcat(ctypes.byref(d), dtype_code(dz), _p(dz), _p(a_in), _p(w_kcat), _p(bias), _p(dx), None, _stream())
        return dx
    st = torch.empty((lib.rpe_conv2d_dgrad_stats_tiles(ctypes.byref(d), dtype_code(dz)), 2, ci), dtype=torch.float32, device=dz.device)
    ep = BnBwdEpilogue(*(None if t is None else t.data_ptr() for t in (bn["y"], bn.get("a_out"), bn["mean"], bn["invstd"], bn.get("scale"), bn.get("shift"), st,
                                                                      bn.get("a_mask"))))
    lib.rpe_conv1x1_dgrad_kcat(ctypes.byref(d), dtype_code(dz), _p(dz), _p(a_in), _p(w_kcat), _p(bias), _p(dx), ctypes.byref(ep), _stream())
    return dx, st


def conv2d_wgrad(x, dy, k, stride, pad, deterministic=True):
    """-> dw [Co,kh,kw,Ci] fp32.  deterministic: slab + fixed-order sum (bitwise reproducible); else fp32 atomics."""
    _chk(x, "x"), _chk(dy, "dy")
    co = dy.shape[3]
    d = conv_desc(x.shape, co, k, stride, pad)
    if deterministic:
        dw = torch.empty((co, k, k, x.shape[3]), dtype=torch.float32, device=x.device)
        ws = scratch(lib.rpe_conv2d_wgrad_workspace_bytes(ctypes.byref(d), dtype_code(x)), x.device)
        lib.rpe_conv2d_wgrad_det(ctypes.byref(d), dtype_code(x), _p(x), _p(dy), _p(dw), _p(ws), ws.numel(), _stream())
        return dw
    dw = torch.zeros((co, k, k, x.shape[3]), dtype=torch.float32, device=x.device)
    lib.rpe_conv2d_wgrad(ctypes.byref(d), dtype_code(x), _p(x), _p(dy), _p(dw), _stream())
    return dw


def pack_conv_weight(w_krsc_f32, dtype):
    """fp32 [Co,kh,kw,Ci] -> (forward copy in `dtype`, dgrad copy [Ci,kh,kw,Co] in `dtype`)."""
    co, kh, kw, ci = w_krsc_f32.shape
    wf = torch.empty((co, kh, kw, ci), dtype=dtype, device=w_krsc_f32.device)
    wd = torch.empty((ci, kh, kw, co), dtype=dtype, device=w_krsc_f32.device)
    lib.rpe_pack_conv_weight(dtype_code(dtype), _p(_chk(w_krsc_f32, "w")), _p(wf), _p(wd), co, kh, kw, ci, _stream())
    return wf, wd


STEM_PAD = 3   # RPE_STEM_PAD: the staged image is zero-bordered, [B, H + 6, W + 6, 4]


def stage_image(img_nchw, dtype):
    """(B, 3, H, W) fp32 -> the zero-bordered NHWC4 image [B, H + 6, W + 6, 4] the stem kernels read (interior written by the kernel)"""
    b, c, h, w = img_nchw.shape
    assert c == 3 and img_nchw.dtype == torch.float32
    out = torch.zeros((b, h + 2 * STEM_PAD, w + 2 * STEM_PAD, 4), dtype=dtype, device=img_nchw.device)
    lib.rpe_stage_image_nhwc4(dtype_code(dtype), _p(_chk(img_nchw, "img")), _p(out), b, h, w, _stream())
    return out


def pack_stem_weight(w_oihw, dtype, scale=None):
    """OIHW [64, 3, 7, 7] fp32 -> [64, 8, 8, 4] in `dtype` (tap row / column 7 and channel 3 zero); scale [64] fp32: w * scale[co] formed
    in fp32 before the rounding (inference: BatchNorm folded into the conv)"""
    out = torch.empty((64, 8, 8, 4), dtype=dtype, device=w_oihw.device)
    lib.rpe_pack_stem_weight(dtype_code(dtype), _p(_chk(w_oihw, "w")), _p(scale), _p(out), _stream())
    return out


def stem_conv_fwd(x4, w_packed, want_stats=False):
    b, h, w, _ = x4.shape
    h, w = h - 2 * STEM_PAD, w - 2 * STEM_PAD
    ho, wo = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1
    y = torch.empty((b, ho, wo, 64), dtype=x4.dtype, device=x4.device)
    st = torch.empty((stats_tiles(b * ho * wo), 2, 64), dtype=torch.float32, device=x4.device) if want_stats else None
    lib.rpe_stem_conv_fwd(dtype_code(x4), _p(x4), _p(w_packed), _p(y), _p(st), b, h, w, _stream())
    return (y, st) if want_stats else y


def stem_conv_fwd_affine(x4, w_packed, bias, relu=True):
    """Inference form of the stem: [relu](conv1(x4, w_packed) + bias) in one launch (w_packed = pack_stem_weight(w, dtype, scale))"""
    b, h, w, _ = x4.shape
    h, w = h - 2 * STEM_PAD, w - 2 * STEM_PAD
    out = torch.empty((b, (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1, 64), dtype=x4.dtype, device=x4.device)
    lib.rpe_stem_conv_fwd_affine(dtype_code(x4), _p(x4), _p(w_packed), _p(out), _p(bias), int(relu), b, h, w, _stream())
    return out


def stem_conv_wgrad(x4, dy, deterministic=True):
    """-> dw OIHW [64, 3, 7, 7] fp32.  deterministic: per-workgroup tiles through the scratch buffer, summed in a fixed order
    (rpe_stem_conv_wgrad_det); otherwise the atomic form the engine takes without a slab (it accumulates: dw_packed starts at zero)"""
    b, h, w, _ = x4.shape
    h, w = h - 2 * STEM_PAD, w - 2 * STEM_PAD
    dwp = torch.zeros((64, 8, 8, 4), dtype=torch.float32, device=x4.device)
    if deterministic:
        ws = scratch(lib.rpe_stem_conv_wgrad_workspace_bytes(dtype_code(x4), b, h, w), x4.device)
        lib.rpe_stem_conv_wgrad_det(dtype_code(x4), _p(x4), _p(dy), _p(dwp), b, h, w, _p(ws), ws.numel(), _stream())
    else:
        lib.rpe_stem_conv_wgrad(dtype_code(x4), _p(x4), _p(dy), _p(dwp), b, h, w, _stream())
    dw = torch.empty((64, 3, 7, 7), dtype=torch.float32, device=x4.device)
    lib.rpe_unpack_stem_grad(_p(dwp), _p(dw), _stream())
    return dw


def pack_conv_weights_multi(layers, dtype):
    """Every layer of `layers` = [(w_krsc fp32 [Co, kh, kw, Ci], scale [Co] fp32 or None)] packed in ONE launch (rpe_pack_conv_weights_multi)
    -> [(forward copy in `dtype`, scaled where a scale is given; dgrad copy [Ci, kh, kw, Co], unscaled)]"""
    from ._lib import PackDesc
    tab, outs, start = (PackDesc * len(layers))(), [], 0
    for d, (w, scale) in zip(tab, layers):
        co, kh, kw, ci = _chk(w, "w").shape
        wf = torch.empty((co, kh, kw, ci), dtype=dtype, device=w.device)
        wd = torch.empty((ci, kh, kw, co), dtype=dtype, device=w.device)
        d.src, d.wf, d.wd, d.Co, d.RS, d.Ci, d.start = w.data_ptr(), wf.data_ptr(), wd.data_ptr(), co, kh * kw, ci, start
        d.scale = None if scale is None else scale.data_ptr()
        start += w.numel()
        outs.append((wf, wd))
    dev = layers[0][0].device
    table = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
    lib.rpe_pack_conv_weights_multi(dtype_code(dtype), _p(table), len(layers), start, _stream())
    return outs


def bn_finalize(part, count, gamma, beta, running_mean=None, running_var=None, num_batches=None, momentum=0.1, eps=1e-5):
    tiles, _, c = part.shape
    dev = part.device
    scale, shift, mean, invstd = (torch.empty(c, dtype=torch.float32, device=dev) for _ in range(4))
    dpart = torch.zeros(256 * 2 * c + 64, dtype=torch.float64, device=dev)  # RPE_BN_DPART_DOUBLES(c); counters start at zero
    lib.rpe_bn_finalize(_p(part), tiles, c, count, _p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(num_batches),
                        momentum, eps, _p(scale), _p(shift), _p(mean), _p(invstd), _p(dpart), _stream())
    return scale, shift, mean, invstd


def bn_apply(y, scale, shift, residual=None, relu=True):
    out = torch.empty_like(y)
    c = y.shape[-1]
    lib.rpe_bn_apply(dtype_code(y), _p(_chk(y, "y")), _p(residual), _p(out), _p(scale), _p(shift), y.numel() // c, c, int(relu), _stream())
    return out


def bn_apply_mask(y, scale, shift, residual=None):
    """relu(y*scale + shift (+ residual)) and its packed ReLU mask (1 byte per 8 channels); 16-bit element types only."""
    out = torch.empty_like(y)
    c = y.shape[-1]
    mask = torch.empty(y.numel() // 8, dtype=torch.uint8, device=y.device)
    lib.rpe_bn_apply_mask(dtype_code(y), _p(_chk(y, "y")), _p(residual), _p(out), _p(scale), _p(shift), y.numel() // c, c, _p(mask), _stream())
    return out, mask


def bn_apply_res_bn(y, scale, shift, res_y, res_scale, res_shift, relu=True, want_mask=False):
    """[relu](y*scale + shift + res_y*res_scale + res_shift): the residual is a raw conv output under its own BatchNorm (the
    projection shortcut), applied on the fly; want_mask: also the packed ReLU mask (16-bit element types)."""
    out = torch.empty_like(y)
    c = y.shape[-1]
    mask = torch.empty(y.numel() // 8, dtype=torch.uint8, device=y.device) if want_mask else None
    lib.rpe_bn_apply_res_bn(dtype_code(y), _p(_chk(y, "y")), _p(res_y), _p(res_scale), _p(res_shift), _p(out), _p(scale), _p(shift), y.numel() // c, c,
                            int(relu), _p(mask), _stream())
    return (out, mask) if want_mask else out


def gram(x):
    """x [..., C] (NHWC activations) -> (x^T x [C, C], colsum(x) [C], the whole buffer) fp32, one launch + fixed-order slab sum"""
    c = x.shape[-1]
    m = x.numel() // c
    code = dtype_code(x)
    ones_row = lib.rpe_gram_ones_row(c)
    out = torch.empty((ones_row + 1, c), dtype=torch.float32, device=x.device)
    ws = scratch(lib.rpe_gram_workspace_bytes(code, m, c), x.device)
    lib.rpe_gram(code, _p(_chk(x, "x")), m, c, _p(out), _p(ws), ws.numel(), _stream())
    return out[:c], out[ones_row], out


def bn_apply_gram(y, scale, shift):
    """relu(y * scale + shift) and the Gram buffer of the result (as ops.gram) in one pass: (out, S [C, C], s1 [C], buffer)"""
    c = y.shape[-1]
    m = y.numel() // c
    code = dtype_code(y)
    ones_row = lib.rpe_gram_ones_row(c)
    buf = torch.zeros((ones_row + 1, c), dtype=torch.float32, device=y.device)
    out = torch.empty_like(y)
    ws = scratch(lib.rpe_bn_apply_gram_workspace_bytes(code, m, c), y.device)
    lib.rpe_bn_apply_gram(code, _p(_chk(y, "y")), _p(out), _p(scale), _p(shift), m, c, _p(buf), _p(ws), ws.numel(), _stream())
    return out, buf[:c], buf[ones_row], buf


def bn_stats_from_gram(w, gram_buf, count, gamma, beta, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    """BatchNorm statistics of y = x w^T from the Gram buffer of x (ops.gram): (scale, shift, mean, invstd)"""
    co, ci = w.shape
    dev = w.device
    scale, shift, mean, invstd = (torch.empty(co, dtype=torch.float32, device=dev) for _ in range(4))
    lib.rpe_bn_stats_from_gram(dtype_code(w), _p(_chk(w, "w")), co, ci, _p(gram_buf), lib.rpe_gram_ones_row(ci), int(count), _p(gamma), _p(beta),
                               _p(running_mean), _p(running_var), None, momentum, eps, _p(scale), _p(shift), _p(mean), _p(invstd), _stream())
    return scale, shift, mean, invstd


def conv1x1_fwd_bn(x, w, scale, shift, residual=None, res_scale=None, res_shift=None, want_y=False):
    """relu((x w^T) * scale + shift + residual [* res_scale + res_shift]) with the packed ReLU mask, one launch (16-bit types)"""
    co, ci = w.shape
    d = conv_desc(x.shape, co, 1, 1, 0)
    out = torch.empty(tuple(x.shape[:-1]) + (co,), dtype=x.dtype, device=x.device)
    y = torch.empty_like(out) if want_y else None
    mask = torch.empty(out.numel() // 8, dtype=torch.uint8, device=x.device)
    lib.rpe_conv1x1_fwd_bn(ctypes.byref(d), dtype_code(x), _p(_chk(x, "x")), _p(_chk(w, "w")), _p(out), _p(y), _p(scale), _p(shift), _p(residual),
                           _p(res_scale), _p(res_shift), _p(mask), _stream())
    return out, mask, y


def bn_backward(dA, a_out, y, mean, invstd, gamma, want_dz=False):
    c = y.shape[-1]
    dev = y.device
    dgamma = torch.empty(c, dtype=torch.float32, device=dev)
    dbeta = torch.empty(c, dtype=torch.float32, device=dev)
    dy = torch.empty_like(y)
    dz = torch.empty_like(y) if want_dz else None
    part = torch.empty(2 * 1024 * c, dtype=torch.float32, device=dev)
    c1c2 = torch.empty(2 * c, dtype=torch.float32, device=dev)
    dpart = torch.zeros(256 * 2 * c + 64, dtype=torch.float64, device=dev)  # RPE_BN_DPART_DOUBLES(c); counters start at zero
    lib.rpe_bn_backward(dtype_code(y), _p(dA), _p(a_out), _p(y), _p(mean), _p(invstd), _p(gamma), _p(dgamma), _p(dbeta), _p(dy), _p(dz),
                        y.numel() // c, c, _p(part), part.numel(), _p(c1c2), _p(dpart), _stream())
    return dy, dgamma, dbeta, dz


def maxpool_fwd(x):
    b, h, w, c = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = torch.empty((b, ho, wo, c), dtype=x.dtype, device=x.device)
    idx = torch.empty((b, ho, wo, c), dtype=torch.uint8, device=x.device)
    lib.rpe_maxpool3x3s2_fwd(dtype_code(x), _p(_chk(x, "x")), _p(out), _p(idx), b, h, w, c, _stream())
    return out, idx


def bn_apply_maxpool(y, scale, shift):
    """a = relu(y * scale + shift), pooled = maxpool3x3s2(a), winner taps -- one pass over y [B,H,W,C] (H, W even)"""
    b, h, w, c = y.shape
    a = torch.empty_like(y)
    out = torch.empty((b, h // 2, w // 2, c), dtype=y.dtype, device=y.device)
    idx = torch.empty((b, h // 2, w // 2, c), dtype=torch.uint8, device=y.device)
    lib.rpe_bn_apply_maxpool3x3s2(dtype_code(y), _p(_chk(y, "y")), _p(scale), _p(shift), _p(a), _p(out), _p(idx), b, h, w, c, _stream())
    return a, out, idx


def maxpool_bwd(dout, idx, x_shape, addend=None):
    b, h, w, c = x_shape
    dx = torch.empty(tuple(x_shape), dtype=dout.dtype, device=dout.device)
    lib.rpe_maxpool3x3s2_bwd(dtype_code(dout), _p(dout), _p(idx), _p(addend), _p(dx), b, h, w, c, _stream())
    return dx


def avgpool_fwd(x):
    b, h, w, c = x.shape
    out = torch.empty((b, c), dtype=torch.float32, device=x.device)
    lib.rpe_avgpool_fwd(dtype_code(x), _p(_chk(x, "x")), _p(out), b, h * w, c, _stream())
    return out


def avgpool_bwd(dout, x_shape, dtype):
    b, h, w, c = x_shape
    dx = torch.empty(tuple(x_shape), dtype=dtype, device=dout.device)
    lib.rpe_avgpool_bwd(dtype_code(dtype), _p(dout), _p(dx), b, h * w, c, _stream())
    return dx


# rows up to which rpe_linear_fwd (fp32) runs one workgroup per output column and accepts any row stride / alignment
# (csrc/conv_api.hip: linear_rows_kernel); 0 when switched off
LINEAR_ROWS_MAX = 0 if os.environ.get("RPE_NO_LINEAR_ROWS") else 8
LINEAR_SPLIT_K = not os.environ.get("RPE_NO_LINEAR_SPLITK")   # split-K for Linear launches with few tiles and long K


def linear_fwd(x, w, bias=None, relu=False, addend=None, out=None, n=None, k=None):
    """fp32 (or bf16) y[M, N] = x[M, :K] @ w[:N, :K]^T.  x, w, out, addend are 2-D with arbitrary (chunk-multiple) row strides."""
    m = x.shape[0]
    k = x.shape[1] if k is None else k
    n = w.shape[0] if n is None else n
    if out is None:
        out = torch.zeros((m, pad4(n)), dtype=x.dtype, device=x.device)[:, :n]
    need = lib.rpe_linear_fwd_workspace_bytes(dtype_code(x), m, n, k) if LINEAR_SPLIT_K else 0
    if need > 0:   # few output tiles, long K: split-K through the shared workspace (fixed-order sums)
        ws = scratch(need, x.device)
        lib.rpe_linear_fwd_ws(dtype_code(x), _p(x), x.stride(0), _p(w), w.stride(0), _p(bias), _p(out), out.stride(0), m, n, k, int(relu),
                              _p(addend), 0 if addend is None else addend.stride(0), _p(ws), ws.numel(), _stream())
        return out
    lib.rpe_linear_fwd(dtype_code(x), _p(x), x.stride(0), _p(w), w.stride(0), _p(bias), _p(out), out.stride(0), m, n, k, int(relu),
                       _p(addend), 0 if addend is None else addend.stride(0), _stream())
    return out


def linear_wgrad(dy, x, dw, n=None, k=None, deterministic=True, overwrite=False):
    """dw[:N, :K] (fp32) += dy[M, :N]^T @ x[M, :K].  deterministic: per-workgroup slabs summed in a fixed order, then ONE add
    into dw per element (bitwise reproducible); else fp32 atomics.  overwrite (deterministic form only): dw = ... instead of +=."""
    m = x.shape[0]
    n = dy.shape[1] if n is None else n
    k = x.shape[1] if k is None else k
    if deterministic:
        ws = scratch(lib.rpe_linear_wgrad_workspace_bytes(dtype_code(x), m, n, k), x.device)
        lib.rpe_linear_wgrad_det(dtype_code(x), _p(dy), dy.stride(0), _p(x), x.stride(0), _p(dw), dw.stride(0), m, n, k, 0 if overwrite else 1, _p(ws),
                                 ws.numel(), _stream())
        return dw
    if overwrite:
        dw.zero_()
    lib.rpe_linear_wgrad(dtype_code(x), _p(dy), dy.stride(0), _p(x), x.stride(0), _p(dw), dw.stride(0), m, n, k, _stream())
    return dw


def transpose_f32(w, ldo=None):
    rows, cols = w.shape
    ldo = pad4(rows) if ldo is None else ldo
    out = torch.empty((cols, ldo), dtype=torch.float32, device=w.device)
    lib.rpe_transpose_f32(_p(w), _p(out), rows, cols, w.stride(0), ldo, _stream())
    return out


def relu_bwd(out, dy):
    dx = torch.empty_like(dy)
    assert out.is_contiguous() and dy.is_contiguous()
    lib.rpe_relu_bwd(_p(out), _p(dy), _p(dx), dy.numel(), _stream())
    return dx


def colsum(x, cols=None, out=None, accumulate=False):
    rows = x.shape[0]
    cols = x.shape[1] if cols is None else cols
    if out is None:
        out = torch.empty(cols, dtype=torch.float32, device=x.device)
    lib.rpe_colsum(_p(x), rows, cols, x.stride(0), _p(out), int(accumulate), _stream())
    return out


def copy2d(src, dst, cols=None):
    cols = src.shape[1] if cols is None else cols
    lib.rpe_copy2d(_p(src), src.stride(0), _p(dst), dst.stride(0), src.shape[0], cols, _stream())
    return dst


def pose_loss(pred, truth, metric, mode, scale, alpha, eps, want_grad=True, valid=None):
    """pred/truth (..., 7) fp32 contiguous -> (out3 [loss, val_pos, val_ori], grad or None).
    valid (uint8 or bool device tensor of pred.shape[:-1], contiguous): only the rows it marks take part (rpe_pose_loss_masked) -- the
    others are never read, add nothing and get a +0 gradient row."""
    n = pred.numel() // 7
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.uint8, torch.bool) or tuple(valid.shape) != tuple(pred.shape[:-1]):
            raise ValueError("pose_loss: valid must be a uint8 or bool tensor of shape %r; got %s %r" % (
                tuple(pred.shape[:-1]), getattr(valid, "dtype", type(valid)), tuple(getattr(valid, "shape", ()))))
        if valid.device != pred.device or not valid.is_cuda:
            raise ValueError("pose_loss: valid must be on the device of pred (%s); got %s" % (pred.device, valid.device))
        if pred.dtype != torch.float32 or truth.dtype != torch.float32 or truth.device != pred.device:
            raise ValueError("pose_loss: pred and truth must be fp32 on one device")
        _chk(valid, "valid")
        if valid.dtype == torch.bool:
            valid = valid.view(torch.uint8)   # (one byte each, 0 / 1: the same memory)
    out3 = torch.empty(3, dtype=torch.float32, device=pred.device)
    grad = torch.empty_like(pred) if want_grad else None
    if valid is None:
        lib.rpe_pose_loss(_p(_chk(pred, "pred")), _p(_chk(truth, "truth")), n, metric, mode, scale, alpha, eps, _p(out3), _p(grad), _stream())
    else:
        lib.rpe_pose_loss_masked(_p(_chk(pred, "pred")), _p(_chk(truth, "truth")), _p(valid), n, metric, mode, scale, alpha, eps, _p(out3), _p(grad),
                                 _stream())
    return out3, grad


def pose_errors(pred, truth, eps, want_pose=True):
    """pred/truth (..., 7) fp32 contiguous -> (pos_err (...), ori_err (...), pose_unit (..., 7) or None): the "val" errors of every
    sample, and the prediction with its quaternion normalised (rpe_pose_errors).  Enqueued on the current stream; nothing is read back."""
    if pred.shape != truth.shape or pred.dim() < 1 or pred.shape[-1] != 7:
        raise ValueError("pose_errors: pred and truth must both be (..., 7), got %s and %s" % (tuple(pred.shape), tuple(truth.shape)))
    if pred.dtype != torch.float32 or truth.dtype != torch.float32:
        raise TypeError("pose_errors: pred and truth must be fp32")
    lead = tuple(pred.shape[:-1])
    pos = torch.empty(lead, dtype=torch.float32, device=pred.device)
    ori = torch.empty(lead, dtype=torch.float32, device=pred.device)
    pose = torch.empty_like(pred) if want_pose else None
    lib.rpe_pose_errors(_p(_chk(pred, "pred")), _p(_chk(truth, "truth")), pred.numel() // 7, eps, _p(pos), _p(ori), _p(pose), _stream())
    return pos, ori, pose


def error_stats(err, lengths=None):
    """err (E, T) fp32 contiguous -> fp64 device tensor of 3 + 2 E values: [mean, population std, max, sum[E], mean[E]]
    (rpe_error_stats: fixed-order fp64 sums, bitwise repeatable, NaN propagates).
    lengths (int32 device tensor (E,), each in [1, T]): row e holds lengths[e] values and padding behind them, which is never read
    (rpe_error_stats_ragged); the figures run over the valid values only."""
    if err.dim() != 2 or err.dtype != torch.float32:
        raise ValueError("error_stats: err must be an fp32 (E, T) tensor, got %s %s" % (err.dtype, tuple(err.shape)))
    e, t = err.shape
    if lengths is not None:
        if not isinstance(lengths, torch.Tensor) or lengths.dtype != torch.int32 or tuple(lengths.shape) != (e,):
            raise ValueError("error_stats: lengths must be an int32 tensor of shape (%d,); got %s %r" % (
                e, getattr(lengths, "dtype", type(lengths)), tuple(getattr(lengths, "shape", ()))))
        if lengths.device != err.device or not lengths.is_cuda:
            raise ValueError("error_stats: lengths must be on the device of err (%s); got %s" % (err.device, lengths.device))
        _chk(lengths, "lengths")
    out = torch.empty(3 + 2 * e, dtype=torch.float64, device=err.device)
    if lengths is None:
        lib.rpe_error_stats(_p(_chk(err, "err")), e, t, _p(out), _stream())
    else:
        lib.rpe_error_stats_ragged(_p(_chk(err, "err")), e, t, _p(lengths), _p(out), _stream())
    return out


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step):
    lib.rpe_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, step, _stream())


PARAM_STATS_COLUMNS = ("grad_sumsq", "weight_sumsq", "update_sumsq", "grad_max", "weight_max", "grad_nonfinite", "grad_zero", "weight_nonfinite",
                       "step", "first_nonfinite_step")     # the columns of rpe_param_stats_finalize's `out`


def param_stats_rows(n):
    """partial rows tensor of `n` elements takes in rpe_param_stats: a function of n alone (needs no device)"""
    return lib.rpe_param_stats_rows(int(n))


def param_stats_table(entries):
    """[(offset, numel)] in arena order -> the host copy of rpe_param_stats' table: int64 (T, 3) rows {offset, numel, first_row},
    first_row the running sum of param_stats_rows(numel).  An offset that is no multiple of 4 floats is refused here as the C ABI
    refuses it; move the result to the device with .to(device) and pass both."""
    rows, tab = 0, []
    for off, n in entries:
        off, n = int(off), int(n)
        if off < 0 or n < 0:
            raise ValueError("param_stats_table: offset and numel must not be negative, got (%d, %d)" % (off, n))
        if off % 4:
            raise ValueError("param_stats_table: offset %d is not a multiple of 4 floats (16 bytes)" % off)
        tab.append((off, n, rows))
        rows += param_stats_rows(n)
    if not tab:
        raise ValueError("param_stats_table: no tensors")
    return torch.tensor(tab, dtype=torch.int64)


def param_stats_total_rows(table_host):
    """rows of the partials buffer a table needs"""
    return int(table_host[-1, 2]) + param_stats_rows(int(table_host[-1, 1]))


def param_stats(p, g, m, v, table, table_host, partials, out, beta1, beta2, eps, state, every=1):
    """Per-tensor statistics of four fp32 arenas of one layout (rpe_param_stats + rpe_param_stats_finalize: two launches, no host
    synchronisation).  table / table_host: param_stats_table(...) on the device / on the host; partials: fp64 device buffer of at
    least param_stats_total_rows x PARAM_STATS_PART_COLS; out: fp64 (T, PARAM_STATS_COLS) device tensor, columns PARAM_STATS_COLUMNS,
    zeroed by the caller before the first call (column 9 is sticky); state: the optimizer's 8-float device state block (state[5] the
    step count, state[3] the skip flag).  Nothing is written unless (long)state[5] % every == 0."""
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        if t.dtype != torch.float32 or t.numel() != p.numel():
            raise ValueError("param_stats: %s must be fp32 with p's %d elements" % (name, p.numel()))
        _chk(t, name)
    if table_host.dtype != torch.int64 or table_host.is_cuda or table_host.dim() != 2 or table_host.shape[1] != 3 or table_host.shape[0] < 1:
        raise ValueError("param_stats: table_host must be an int64 (T, 3) CPU tensor (param_stats_table)")
    if table.dtype != torch.int64 or tuple(table.shape) != tuple(table_host.shape):
        raise ValueError("param_stats: table must be table_host on the device")
    T = table_host.shape[0]
    if int((table_host[:, 0] + table_host[:, 1]).max()) > p.numel():
        raise ValueError("param_stats: a tensor of the table ends behind the arena")
    if partials.dtype != torch.float64 or partials.numel() < param_stats_total_rows(table_host) * PARAM_STATS_PART_COLS:
        raise ValueError("param_stats: partials must be fp64 with %d rows of %d" % (param_stats_total_rows(table_host), PARAM_STATS_PART_COLS))
    if out.dtype != torch.float64 or out.numel() != T * PARAM_STATS_COLS:
        raise ValueError("param_stats: out must be fp64 (%d, %d)" % (T, PARAM_STATS_COLS))
    if state.dtype != torch.float32 or state.numel() < 8:
        raise ValueError("param_stats: state is the 8-float device state block")
    _chk(table, "table"), _chk(table_host, "table_host"), _chk(partials, "partials"), _chk(out, "out")
    s = _stream()
    lib.rpe_param_stats(_p(p), _p(g), _p(m), _p(v), _p(table), ctypes.c_void_p(table_host.data_ptr()), T, _p(partials), beta1, beta2, eps, _p(state),
                        int(every), s)
    lib.rpe_param_stats_finalize(_p(partials), _p(table), T, _p(out), _p(state), int(every), s)


def feature_planes(x_nhwc, image=None, out=None, minmax=None):
    """x [B,H,W,C] (compute dtype, contiguous) -> (planes fp32, minmax fp32): [B,C,H,W] / [B,C,2] for the whole batch, or
    [C,H,W] / [C,2] for image number `image`.  The widening is exact; minmax is each channel's range over its finite values.
    out / minmax: contiguous fp32 destinations of those shapes (e.g. one frame's slice of an episode's tensor)."""
    _chk(x_nhwc, "x")
    b, h, w, c = x_nhwc.shape
    dev = x_nhwc.device
    lead = (b,) if image is None else ()
    if image is not None and not 0 <= image < b:
        raise IndexError("feature_planes: image %d of a batch of %d" % (image, b))
    planes = torch.empty(lead + (c, h, w), dtype=torch.float32, device=dev) if out is None else _chk(out, "out")
    mm = torch.empty(lead + (c, 2), dtype=torch.float32, device=dev) if minmax is None else _chk(minmax, "minmax")
    if planes.dtype != torch.float32 or mm.dtype != torch.float32 or tuple(planes.shape) != lead + (c, h, w) or tuple(mm.shape) != lead + (c, 2):
        raise ValueError("feature_planes: out / minmax must be fp32 of shape %r / %r" % (lead + (c, h, w), lead + (c, 2)))
    if image is None:
        lib.rpe_feature_planes_batch(dtype_code(x_nhwc), _p(x_nhwc), b, h, w, c, _p(planes), _p(mm), _stream())
    else:
        lib.rpe_feature_planes(dtype_code(x_nhwc), _p(x_nhwc), image, h, w, c, _p(planes), _p(mm), _stream())
    return planes, mm


def mosaic_shape(c, h, w, cols, gutter):
    rows = (c + cols - 1) // cols
    return rows * (h + gutter) - gutter, cols * (w + gutter) - gutter


def feature_mosaic(planes, minmax, cols, gutter=1, flip_y=True):
    """planes [C,H,W] fp32 + minmax [C,2] -> uint8 colour-index image of per-channel autoscaled tiles (rpe_feature_mosaic)."""
    _chk(planes, "planes"), _chk(minmax, "minmax")
    c, h, w = planes.shape
    if planes.dtype != torch.float32 or minmax.dtype != torch.float32 or tuple(minmax.shape) != (c, 2):
        raise ValueError("feature_mosaic: planes [C,H,W] and minmax [C,2] must be fp32")
    out = torch.empty(mosaic_shape(c, h, w, cols, gutter), dtype=torch.uint8, device=planes.device)
    lib.rpe_feature_mosaic(_p(planes), _p(minmax), c, h, w, cols, gutter, int(bool(flip_y)), _p(out), _stream())
    return out


_DEPTH_TABLES = {}


def _depth_tables(hs, ws, hr, wr, device):
    """device tap tables of the Pillow-exact fp32 resize for one frame geometry (built once, kept: a captured graph replays the
    staging without a host-to-device copy)"""
    from .util.data_utils import pil_bilinear_tables_f64
    key = (hs, ws, hr, wr, device.type, device.index)
    tabs = _DEPTH_TABLES.get(key)
    if tabs is None:
        tabs = []
        for i, o in ((ws, wr), (hs, hr)):
            if i == o:
                tabs.append((None, None, 0))
            else:
                bounds, kk = pil_bilinear_tables_f64(i, o)
                tabs.append((torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device), kk.shape[1]))
        _DEPTH_TABLES[key] = tabs
    return tabs


def stage_depth_window(raw, hr, wr, top, left, h, w):
    """raw [B, Hs, Ws] fp32 -> [B, 1, h, w] fp32: the window [top, top + h) x [left, left + w) of Pillow's mode-F bilinear resize of
    every frame to hr x wr (rpe_stage_depth_f32_resized), bit for bit."""
    _chk(raw, "raw")
    if raw.dim() != 3 or raw.dtype != torch.float32:
        raise ValueError("stage_depth_window: raw must be [B, Hs, Ws] fp32; got %s %r" % (raw.dtype, tuple(raw.shape)))
    b, hs, ws = raw.shape
    if top < 0 or left < 0 or top + h > hr or left + w > wr:
        raise ValueError("stage_depth_window: the %dx%d window at (%d, %d) leaves the %dx%d resized frame" % (h, w, top, left, hr, wr))
    (xb, xk, ksx), (yb, yk, ksy) = _depth_tables(hs, ws, hr, wr, raw.device)
    out = torch.empty((b, 1, h, w), dtype=torch.float32, device=raw.device)
    lib.rpe_stage_depth_f32_resized(_p(raw), _p(out), b, hs, ws, hr, wr, top, left, h, w, _p(xb), _p(xk), ksx, _p(yb), _p(yk), ksy, _stream())
    return out


def stage_depth(raw, crop_hw=(224, 224), size=256):
    """The reference's depth_transform (ToPILImage -> Resize(size) -> CenterCrop(crop_hw) -> ToTensor, util/data_utils.py:55-60) on the
    device: raw fp32 depth frames [B, Hs, Ws] or channels-last (..., Hs, Ws, 1) -> [B, 1, H, W] fp32, bit for bit what Pillow gives."""
    from .util.data_utils import crop_origin, resized_hw
    if raw.dim() >= 4 and raw.shape[-1] == 1:
        raw = raw.reshape(-1, raw.shape[-3], raw.shape[-2])
    if raw.dim() != 3 or raw.dtype != torch.float32:
        raise ValueError("stage_depth: raw depth is fp32 [B, Hs, Ws] or (..., Hs, Ws, 1); got %s %r" % (raw.dtype, tuple(raw.shape)))
    hs, ws = raw.shape[-2:]
    h, w = crop_hw
    hr, wr = resized_hw(hs, ws, size)
    if min(hr, wr) < min(h, w) or hr < h or wr < w:
        raise ValueError("frames of %dx%d resize to %dx%d, smaller than the %dx%d crop" % (hs, ws, hr, wr, h, w))
    top, left = crop_origin(hr, wr, h, w)
    return stage_depth_window(raw.contiguous(), hr, wr, top, left, h, w)


_FRAME_TABLES = {}


def _frame_tables(hs, ws, hr, wr, device):
    """device tap tables of the Pillow-exact 8-bit resize for one frame geometry (built once, kept)"""
    from .util.data_utils import pil_bilinear_tables
    key = (hs, ws, hr, wr, device.type, device.index)
    tabs = _FRAME_TABLES.get(key)
    if tabs is None:
        tabs = []
        for i, o in ((ws, wr), (hs, hr)):
            if i == o:
                tabs.append((None, None, 0))
            else:
                bounds, kk = pil_bilinear_tables(i, o)
                tabs.append((torch.from_numpy(bounds).to(device), torch.from_numpy(kk).contiguous().to(device), kk.shape[1]))
        _FRAME_TABLES[key] = tabs
    return tabs


def _norm3(v):
    return (ctypes.c_float * 3)(*(float(x) for x in v))


def stage_frames_window(frames, dtype, hr, wr, top, left, h, w, mean, std):
    """frames uint8 [B, Hs, Ws, 3] -> the zero-bordered NHWC4 image [B, h + 6, w + 6, 4] in `dtype`: the window [top, top + h) x
    [left, left + w) of Pillow's 8-bit bilinear resize of every frame to hr x wr, normalised (rpe_stage_frames_u8_resized)."""
    _chk(frames, "frames")
    if frames.dim() != 4 or frames.shape[-1] != 3 or frames.dtype != torch.uint8:
        raise ValueError("stage_frames_window: frames must be uint8 [B, Hs, Ws, 3]; got %s %r" % (frames.dtype, tuple(frames.shape)))
    b, hs, ws, _ = frames.shape
    if top < 0 or left < 0 or top + h > hr or left + w > wr:
        raise ValueError("stage_frames_window: the %dx%d window at (%d, %d) leaves the %dx%d resized frame" % (h, w, top, left, hr, wr))
    (xb, xk, ksx), (yb, yk, ksy) = _frame_tables(hs, ws, hr, wr, frames.device)
    tmp = torch.empty(b * hs * wr * 3, dtype=torch.uint8, device=frames.device) if xb is not None else None
    out = torch.zeros((b, h + 2 * STEM_PAD, w + 2 * STEM_PAD, 4), dtype=dtype, device=frames.device)
    lib.rpe_stage_frames_u8_resized(dtype_code(dtype), _p(frames), _p(out), b, hs, ws, hr, wr, top, left, h, w, _p(xb), _p(xk), ksx, _p(yb), _p(yk), ksy,
                                    _p(tmp), _norm3(mean), _norm3(std), _stream())
    return out


def frames_route(hs, ws, h, w, size=256):
    """How frames of hs x ws reach a crop of h x w, exactly as engine.py decides it: ("plain",) -- rpe_stage_frames_u8, only when nothing
    is resized and both crop differences are even (the kernel floors its centre crop) -- or ("window", hr, wr, top, left) with
    crop_origin's offsets (torchvision's CenterCrop rounds half to even)."""
    from .util.data_utils import crop_origin, resized_hw
    hr, wr = resized_hw(hs, ws, size)
    if min(hr, wr) < min(h, w) or hr < h or wr < w:
        raise ValueError("frames of %dx%d resize to %dx%d, smaller than the %dx%d crop" % (hs, ws, hr, wr, h, w))
    if (hr, wr) == (hs, ws) and (hs - h) % 2 == 0 and (ws - w) % 2 == 0:
        return ("plain",)
    return ("window", hr, wr) + crop_origin(hr, wr, h, w)


def stage_frames(frames, dtype, crop_hw=(224, 224), size=256, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """The reference's image transform (ToPILImage -> Resize(size) -> CenterCrop(crop_hw) -> ToTensor -> Normalize) on the device:
    frames uint8 [B, Hs, Ws, 3] -> the zero-bordered NHWC4 image [B, H + 6, W + 6, 4] in `dtype`, routed as engine.py routes it."""
    _chk(frames, "frames")
    if frames.dim() != 4 or frames.shape[-1] != 3 or frames.dtype != torch.uint8:
        raise ValueError("stage_frames: frames must be uint8 [B, Hs, Ws, 3]; got %s %r" % (frames.dtype, tuple(frames.shape)))
    b, hs, ws, _ = frames.shape
    h, w = crop_hw
    route = frames_route(hs, ws, h, w, size)
    if route[0] == "plain":
        out = torch.zeros((b, h + 2 * STEM_PAD, w + 2 * STEM_PAD, 4), dtype=dtype, device=frames.device)
        lib.rpe_stage_frames_u8(dtype_code(dtype), _p(frames), _p(out), b, hs, ws, h, w, _norm3(mean), _norm3(std), _stream())
        return out
    return stage_frames_window(frames, dtype, *route[1:], h, w, mean, std)


AUGMENT_DESC_FIELDS = ("seed", "qb_lo", "qb_hi", "qc_lo", "qc_hi", "qs_lo", "qs_hi", "noise_q", "erase_thresh", "eh_lo", "eh_hi", "ew_lo", "ew_hi",
                       "fill_mode", "fill_r", "fill_g", "fill_b", "group")


def augment_desc(seed=0, qb_lo=65536, qb_hi=65536, qc_lo=65536, qc_hi=65536, qs_lo=65536, qs_hi=65536, noise_q=0, erase_thresh=0, eh_lo=1, eh_hi=1,
                 ew_lo=1, ew_hi=1, fill_mode=0, fill_r=124, fill_g=116, fill_b=104, group=0):
    """rpe_augment_desc from plain integers (the defaults are the identity settings); AUGMENT_DESC_FIELDS is the order of the flat
    list form `torch.ops.rpe.augment_frames_u8` takes"""
    from ._lib import AugmentDesc
    d = AugmentDesc()
    d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    for k, v in (("qb_lo", qb_lo), ("qb_hi", qb_hi), ("qc_lo", qc_lo), ("qc_hi", qc_hi), ("qs_lo", qs_lo), ("qs_hi", qs_hi), ("noise_q", noise_q),
                 ("erase_thresh", erase_thresh), ("eh_lo", eh_lo), ("eh_hi", eh_hi), ("ew_lo", ew_lo), ("ew_hi", ew_hi), ("fill_mode", fill_mode),
                 ("group", group)):
        setattr(d, k, int(v))
    for i, v in enumerate((fill_r, fill_g, fill_b)):
        if not 0 <= int(v) <= 255:
            raise ValueError("augment_desc: the fill colour is three bytes; got %r" % ((fill_r, fill_g, fill_b),))
        d.fill_rgb[i] = int(v)
    return d


def augment_streams(desc, b):
    """number of parameter streams of a batch of b frames"""
    return desc.group if desc.group > 0 else b


def augment_frames_u8(frames, desc, state, out=None, params=None, sums=None):
    """frames uint8 (..., Hs, Ws, 3) contiguous -> the augmented frames, uint8 of the same shape (rpe_augment_frames_u8: brightness,
    contrast, saturation, noise, erasing in integer arithmetic).  desc: augment_desc(...).  state: int32 device tensor whose element 0
    is the step counter; the launch advances it by one.  out: destination (may be `frames` itself).  params / sums: int32 (1 + 8 G,) /
    int64 (B,) device tensors receiving the parameter table and the per-frame grey sums (allocated when not given)."""
    if frames.dtype != torch.uint8 or frames.dim() < 4 or frames.shape[-1] != 3:
        raise ValueError("augment_frames_u8: frames must be uint8 (..., Hs, Ws, 3); got %s %r" % (frames.dtype, tuple(frames.shape)))
    _chk(frames, "frames")
    hs, ws = frames.shape[-3:-1]
    b = frames.numel() // (hs * ws * 3)
    if b == 0:
        raise ValueError("augment_frames_u8: empty batch")
    g = augment_streams(desc, b)
    dev = frames.device
    if state.dtype != torch.int32 or state.numel() < 1 or state.device != dev:
        raise ValueError("augment_frames_u8: state must be an int32 tensor on the frames' device")
    if out is None:
        out = torch.empty_like(frames)
    elif out.dtype != torch.uint8 or out.shape != frames.shape or out.device != dev:
        raise ValueError("augment_frames_u8: out must be uint8 of the frames' shape on their device")
    _chk(out, "out")
    if params is None:
        params = torch.empty(1 + 8 * g, dtype=torch.int32, device=dev)
    elif params.dtype != torch.int32 or params.numel() < 1 + 8 * g or params.device != dev:
        raise ValueError("augment_frames_u8: params must be int32 with at least %d elements" % (1 + 8 * g))
    if sums is None:
        sums = torch.empty(b, dtype=torch.int64, device=dev)
    elif sums.dtype != torch.int64 or sums.numel() < b or sums.device != dev:
        raise ValueError("augment_frames_u8: sums must be int64 with at least %d elements" % b)
    lib.rpe_augment_frames_u8(_p(frames), _p(out), b, hs, ws, ctypes.byref(desc), _p(state), _p(_chk(params, "params")), _p(_chk(sums, "sums")), _stream())
    return out


BLUR_MAX_LEVELS, BLUR_MAX_RADIUS, BLUR_MAX_DIRS, BLUR_TAP_SUM = 8, 8, 16, 2048
BLUR_DESC_FIELDS = ("seed", "gauss_thresh", "motion_thresh", "radius", "taps", "n_lengths", "dir_cx", "dir_cy", "group")
BLUR_DESC_NUMBERS = 4 + BLUR_MAX_LEVELS * (2 + BLUR_MAX_RADIUS) + 2 + 2 * BLUR_MAX_DIRS + 1   # the flat list of torch.ops.rpe.blur_frames_u8


def blur_desc(seed=0, gauss_thresh=0, motion_thresh=0, radius=(0,), taps=((BLUR_TAP_SUM,),), n_lengths=1, dir_cx=(256,), dir_cy=(0,), group=0):
    """rpe_blur_desc from plain integers (the defaults blur nothing): radius[s] and taps[s][0 .. radius[s]] per Gaussian level
    (n_levels = len(radius)), the Q8 components dir_cx[d], dir_cy[d] per motion direction (n_dirs = len(dir_cx)), n_lengths motion
    lengths 3, 5, ...  Counts and tables that do not fit the struct are refused here; their values by the entry point."""
    from ._lib import BlurDesc
    d = BlurDesc()
    d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    for k, v in (("gauss_thresh", gauss_thresh), ("motion_thresh", motion_thresh)):
        if not 0 <= int(v) < 2 ** 32:
            raise ValueError("blur_desc: %s is an unsigned 32-bit word; got %r" % (k, v))
        setattr(d, k, int(v))
    radius, taps, dir_cx, dir_cy = list(radius), [list(t) for t in taps], list(dir_cx), list(dir_cy)
    if not 1 <= len(radius) <= BLUR_MAX_LEVELS or len(taps) != len(radius):
        raise ValueError("blur_desc: 1 to %d levels, one row of taps each; got %d radii and %d rows" % (BLUR_MAX_LEVELS, len(radius), len(taps)))
    if not 1 <= len(dir_cx) <= BLUR_MAX_DIRS or len(dir_cy) != len(dir_cx):
        raise ValueError("blur_desc: 1 to %d directions with both components; got %d and %d" % (BLUR_MAX_DIRS, len(dir_cx), len(dir_cy)))
    d.n_levels, d.n_lengths, d.n_dirs, d.group = len(radius), int(n_lengths), len(dir_cx), int(group)
    for s, (r, row) in enumerate(zip(radius, taps)):
        if len(row) > BLUR_MAX_RADIUS + 1:
            raise ValueError("blur_desc: a level has at most %d taps; got %d" % (BLUR_MAX_RADIUS + 1, len(row)))
        d.radius[s] = int(r)
        for k, w in enumerate(row):
            d.taps[s][k] = int(w)
    for i, (cx, cy) in enumerate(zip(dir_cx, dir_cy)):
        d.dir_cx[i], d.dir_cy[i] = int(cx), int(cy)
    return d


def blur_desc_numbers(seed=0, gauss_thresh=0, motion_thresh=0, radius=(0,), taps=((BLUR_TAP_SUM,),), n_lengths=1, dir_cx=(256,), dir_cy=(0,), group=0):
    """blur_desc's arguments as the flat list of BLUR_DESC_NUMBERS integers `torch.ops.rpe.blur_frames_u8` takes: seed (as a signed
    64-bit value), gauss_thresh, motion_thresh, n_levels, 8 radii, 8 x 9 taps, n_lengths, n_dirs, 16 + 16 components, group"""
    d = blur_desc(seed, gauss_thresh, motion_thresh, radius, taps, n_lengths, dir_cx, dir_cy, group)   # (checks the counts)
    seed = d.seed - (1 << 64) if d.seed >= (1 << 63) else d.seed
    return ([seed, d.gauss_thresh, d.motion_thresh, d.n_levels] + list(d.radius) + [w for row in d.taps for w in row] + [d.n_lengths, d.n_dirs]
            + list(d.dir_cx) + list(d.dir_cy) + [d.group])


def blur_desc_from_numbers(numbers):
    """the inverse of blur_desc_numbers -> rpe_blur_desc"""
    n = [int(v) for v in numbers]
    if len(n) != BLUR_DESC_NUMBERS:
        raise ValueError("blur_frames_u8: desc has %d integers (ops.blur_desc_numbers); got %d" % (BLUR_DESC_NUMBERS, len(n)))
    levels, dirs = n[3], n[85]
    if not 1 <= levels <= BLUR_MAX_LEVELS or not 1 <= dirs <= BLUR_MAX_DIRS:
        raise ValueError("blur_frames_u8: desc names %d levels and %d directions" % (levels, dirs))
    return blur_desc(seed=n[0], gauss_thresh=n[1], motion_thresh=n[2], radius=n[4:4 + levels], taps=[n[12 + 9 * s:21 + 9 * s] for s in range(levels)],
                     n_lengths=n[84], dir_cx=n[86:86 + dirs], dir_cy=n[102:102 + dirs], group=n[118])


def blur_frames_u8(frames, desc, state, out=None, params=None):
    """frames uint8 (..., Hs, Ws, 3) contiguous -> the blurred frames, uint8 of the same shape (rpe_blur_frames_u8: per stream no
    blur, a Gaussian level or a linear motion blur, in integer arithmetic with a replicate border).  desc: blur_desc(...).  state:
    int32 device tensor whose element 0 is the step counter; the launch reads it and does NOT advance it (augment_frames_u8, which
    follows, does).  out: destination, disjoint from `frames`.  params: int32 (1 + 4 G,) device tensor receiving [0] the step used,
    then per stream kind, level, L, d (allocated when not given)."""
    if frames.dtype != torch.uint8 or frames.dim() < 4 or frames.shape[-1] != 3:
        raise ValueError("blur_frames_u8: frames must be uint8 (..., Hs, Ws, 3); got %s %r" % (frames.dtype, tuple(frames.shape)))
    _chk(frames, "frames")
    hs, ws = frames.shape[-3:-1]
    b = frames.numel() // (hs * ws * 3) if hs * ws else 0
    if b == 0:
        raise ValueError("blur_frames_u8: empty batch")
    g = augment_streams(desc, b)
    dev = frames.device
    if state.dtype != torch.int32 or state.numel() < 1 or state.device != dev:
        raise ValueError("blur_frames_u8: state must be an int32 tensor on the frames' device")
    if out is None:
        out = torch.empty_like(frames)
    elif out.dtype != torch.uint8 or out.shape != frames.shape or out.device != dev:
        raise ValueError("blur_frames_u8: out must be uint8 of the frames' shape on their device")
    _chk(out, "out")
    if params is None:
        params = torch.empty(1 + 4 * g, dtype=torch.int32, device=dev)
    elif params.dtype != torch.int32 or params.numel() < 1 + 4 * g or params.device != dev:
        raise ValueError("blur_frames_u8: params must be int32 with at least %d elements" % (1 + 4 * g))
    lib.rpe_blur_frames_u8(_p(frames), _p(out), b, hs, ws, ctypes.byref(desc), _p(_chk(state, "state")), _p(_chk(params, "params")), _stream())
    return out


DEPTH_AUGMENT_DESC_FIELDS = ("seed", "n0", "n1", "n2", "q", "inv_q", "lo", "hi", "drop_thresh", "hole_lo", "hole_hi", "hh_lo", "hh_hi", "hw_lo", "hw_hi",
                             "hole_value", "occluder_value", "group")
DEPTH_AUGMENT_DESC_NUMBERS = ("seed_lo", "seed_hi") + DEPTH_AUGMENT_DESC_FIELDS[1:]   # the flat list of torch.ops.rpe.augment_depth_f32
DEPTH_AUGMENT_ROW = 17  # ints per stream in the parameter table: count, 4 x (top, left, h, w)


def depth_augment_desc(seed=0, n0=0.0, n1=0.0, n2=0.0, q=0.0, inv_q=0.0, lo=-math.inf, hi=math.inf, drop_thresh=0, hole_lo=0, hole_hi=0, hh_lo=1, hh_hi=1,
                       hw_lo=1, hw_hi=1, hole_value=0.0, occluder_value=0.0, group=0):
    """rpe_depth_augment_desc from plain numbers (the defaults are the identity settings); DEPTH_AUGMENT_DESC_FIELDS is the order of
    the flat list form `torch.ops.rpe.augment_depth_f32` takes.  n0..n2 are the kernel's coefficients, sigma_i / sqrt(2 (2^32 - 1))
    (util.data_utils.DepthAugment converts); inv_q is 1 / q, computed by the caller in double."""
    from ._lib import DepthAugmentDesc
    d = DepthAugmentDesc()
    d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    for k, v in (("n0", n0), ("n1", n1), ("n2", n2), ("q", q), ("inv_q", inv_q), ("lo", lo), ("hi", hi), ("hole_value", hole_value),
                 ("occluder_value", occluder_value)):
        setattr(d, k, float(v))
    if not 0 <= int(drop_thresh) < 2 ** 32:
        raise ValueError("depth_augment_desc: drop_thresh is an unsigned 32-bit word; got %r" % (drop_thresh,))
    d.drop_thresh = int(drop_thresh)
    for k, v in (("hole_lo", hole_lo), ("hole_hi", hole_hi), ("hh_lo", hh_lo), ("hh_hi", hh_hi), ("hw_lo", hw_lo), ("hw_hi", hw_hi), ("group", group)):
        setattr(d, k, int(v))
    return d


def depth_frame_hw(shape):
    """(Hs, Ws) of a depth batch of `shape`: channels-last (..., Hs, Ws, 1) as recorded, or (..., 1, H, W) as the synthetic dataset
    hands it out -- both are [B][Hs][Ws] in memory.  A trailing 1 decides for channels-last."""
    shape = tuple(shape)
    if len(shape) >= 4 and shape[-1] == 1:
        return shape[-3], shape[-2]
    if len(shape) >= 4 and shape[-3] == 1:
        return shape[-2], shape[-1]
    raise ValueError("depth frames are (..., Hs, Ws, 1) or (..., 1, H, W); got %r" % (shape,))


def augment_depth_f32(depth, desc, state, out=None, params=None, rgb_params=None, rgb_group=0):
    """depth fp32 contiguous, [B][Hs][Ws] in memory: (..., Hs, Ws, 1) or (..., 1, H, W) -> the augmented depth, fp32 of the same shape
    (rpe_augment_depth_f32: range noise, quantisation, clamp, dropout, holes, shared occluder).  desc: depth_augment_desc(...).
    state: int32 device tensor whose element 0 is the step counter; the launch advances it by one.  out: destination (may be `depth`
    itself).  params: int32 (1 + 17 G,) device tensor receiving the parameter table (allocated when not given).  rgb_params: the table
    augment_frames_u8 wrote for the same batch with group `rgb_group` -- its erased rectangles become occluder_value here."""
    if depth.dtype != torch.float32:
        raise ValueError("augment_depth_f32: depth must be fp32 (..., Hs, Ws, 1) or (..., 1, H, W); got %s %r" % (depth.dtype, tuple(depth.shape)))
    hs, ws = depth_frame_hw(depth.shape)
    _chk(depth, "depth")
    if hs * ws == 0 or depth.numel() == 0:
        raise ValueError("augment_depth_f32: empty batch")
    b = depth.numel() // (hs * ws)
    g = augment_streams(desc, b)
    dev = depth.device
    if state.dtype != torch.int32 or state.numel() < 1 or state.device != dev:
        raise ValueError("augment_depth_f32: state must be an int32 tensor on the depth frames' device")
    if out is None:
        out = torch.empty_like(depth)
    elif out.dtype != torch.float32 or out.shape != depth.shape or out.device != dev:
        raise ValueError("augment_depth_f32: out must be fp32 of the depth frames' shape on their device")
    _chk(out, "out")
    n = 1 + DEPTH_AUGMENT_ROW * g
    if params is None:
        params = torch.empty(n, dtype=torch.int32, device=dev)
    elif params.dtype != torch.int32 or params.numel() < n or params.device != dev:
        raise ValueError("augment_depth_f32: params must be int32 with at least %d elements" % n)
    if rgb_params is not None:
        if int(rgb_group) != desc.group:
            raise ValueError("augment_depth_f32: the RGB table was drawn with group %d, the depth descriptor has %d" % (rgb_group, desc.group))
        if rgb_params.dtype != torch.int32 or rgb_params.numel() < 1 + 8 * g or rgb_params.device != dev:
            raise ValueError("augment_depth_f32: rgb_params must be int32 with at least %d elements on the depth frames' device" % (1 + 8 * g))
        _chk(rgb_params, "rgb_params")
    lib.rpe_augment_depth_f32(_p(depth), _p(out), b, hs, ws, ctypes.byref(desc), _p(_chk(state, "state")), _p(_chk(params, "params")),
                              None if rgb_params is None else _p(rgb_params), int(rgb_group), _stream())
    return out


SAMPLE_DESC_FIELDS = ("seed", "E", "T", "S", "stride", "N", "shuffle")


def sample_desc(seed=0, E=1, T=1, S=1, stride=1, N=1, shuffle=1):
    """rpe_sample_desc from plain integers; SAMPLE_DESC_FIELDS is the order of the flat list form `torch.ops.rpe.sample_windows` takes"""
    from ._lib import SampleDesc
    d = SampleDesc()
    d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    for k, v in (("E", E), ("T", T), ("S", S), ("stride", stride), ("N", N), ("shuffle", shuffle)):
        setattr(d, k, int(v))
    return d


def sample_windows(desc, sel, state, out=None):
    """-> index, int32 (1 + 2 N,): [0] the step used, then per window (episode number in the file, first timestep)
    (rpe_sample_windows).  desc: sample_desc(...).  sel: int32 device tensor, the file's episode numbers of the desc.E selected
    episodes.  state: int32 device tensor whose element 0 is the step counter; the launch advances it by one."""
    dev = sel.device
    if sel.dtype != torch.int32 or sel.dim() != 1 or sel.numel() < desc.E:
        raise ValueError("sample_windows: sel must be an int32 vector of at least E = %d episode numbers" % desc.E)
    if state.dtype != torch.int32 or state.numel() < 1 or state.device != dev:
        raise ValueError("sample_windows: state must be an int32 tensor on sel's device")
    n = 1 + 2 * max(int(desc.N), 0)
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=dev)
    elif out.dtype != torch.int32 or out.numel() < n or out.device != dev:
        raise ValueError("sample_windows: out must be int32 with at least %d elements on sel's device" % n)
    lib.rpe_sample_windows(ctypes.byref(desc), _p(_chk(sel, "sel")), _p(_chk(state, "state")), _p(_chk(out, "out")), _stream())
    return out


def sample_windows_ragged(desc, sel, lengths, state, out=None):
    """sample_windows over episodes of unequal length (rpe_sample_windows_ragged): lengths, an int32 device tensor with one entry per
    episode IN THE FILE, is read as lengths[sel[e]] at every launch; a window never leaves its episode's lengths[sel[e]] timesteps, and
    an episode shorter than desc.S is never drawn.  At most 8192 selected episodes.  The rest as sample_windows."""
    dev = sel.device
    if sel.dtype != torch.int32 or sel.dim() != 1 or sel.numel() < desc.E:
        raise ValueError("sample_windows_ragged: sel must be an int32 vector of at least E = %d episode numbers" % desc.E)
    if not isinstance(lengths, torch.Tensor) or lengths.dtype != torch.int32 or lengths.dim() != 1 or lengths.numel() < 1:
        raise ValueError("sample_windows_ragged: lengths must be an int32 vector, one entry per episode in the file; got %s" % (
            getattr(lengths, "dtype", type(lengths)),))
    if lengths.device != dev or not lengths.is_cuda:
        raise ValueError("sample_windows_ragged: lengths must be on sel's device (%s); got %s" % (dev, lengths.device))
    if state.dtype != torch.int32 or state.numel() < 1 or state.device != dev:
        raise ValueError("sample_windows_ragged: state must be an int32 tensor on sel's device")
    n = 1 + 2 * max(int(desc.N), 0)
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=dev)
    elif out.dtype != torch.int32 or out.numel() < n or out.device != dev:
        raise ValueError("sample_windows_ragged: out must be int32 with at least %d elements on sel's device" % n)
    lib.rpe_sample_windows_ragged(ctypes.byref(desc), _p(_chk(sel, "sel")), _p(_chk(lengths, "lengths")), _p(_chk(state, "state")), _p(_chk(out, "out")),
                                  _stream())
    return out


def gather_rows(pool, index, S, T, out=None):
    """pool (E_file, T, ...) contiguous, any dtype -> (S, N, ...) of that dtype: out[s, n] = pool[index.episode[n], index.t0[n] + s]
    (rpe_gather_rows).  index: int32 (1 + 2 N,) as sample_windows writes it; its entries are trusted (episode < E_file,
    t0 + S <= T).  out: destination, contiguous (a captured call keeps its address)."""
    if pool.dim() < 2 or pool.shape[1] != T or pool.numel() == 0:
        raise ValueError("gather_rows: pool must be (E_file, T = %d, ...); got %r" % (T, tuple(pool.shape)))
    _chk(pool, "pool")
    dev = pool.device
    if index.dtype != torch.int32 or index.dim() != 1 or index.numel() < 3 or index.numel() % 2 != 1 or index.device != dev:
        raise ValueError("gather_rows: index must be an int32 vector of 1 + 2 N elements on the pool's device")
    n = (index.numel() - 1) // 2
    if not 1 <= int(S) <= T:
        raise ValueError("gather_rows: S must lie in [1, T = %d]; got %r" % (T, S))
    shape = (int(S), n) + tuple(pool.shape[2:])
    if out is None:
        out = torch.empty(shape, dtype=pool.dtype, device=dev)
    elif out.dtype != pool.dtype or tuple(out.shape) != shape or out.device != dev:
        raise ValueError("gather_rows: out must be %s %r on the pool's device" % (pool.dtype, shape))
    row_bytes = pool[0, 0].numel() * pool.element_size()
    lib.rpe_gather_rows(_p(pool), _p(_chk(out, "out")), row_bytes, int(T), _p(_chk(index, "index")), int(S), n, _stream())
    return out


OCCLUSION_DESC_FIELDS = ("Hs", "Ws", "ph", "pw", "sy", "sx", "fill_r", "fill_g", "fill_b")


def occlusion_desc(Hs=1, Ws=1, ph=1, pw=1, sy=1, sx=1, fill_r=124, fill_g=116, fill_b=104):
    """rpe_occlusion_desc from plain integers; OCCLUSION_DESC_FIELDS is the order of the flat list form the `torch.ops.rpe` saliency
    operators take"""
    from ._lib import OcclusionDesc
    d = OcclusionDesc()
    for k, v in (("Hs", Hs), ("Ws", Ws), ("ph", ph), ("pw", pw), ("sy", sy), ("sx", sx)):
        setattr(d, k, int(v))
    for i, v in enumerate((fill_r, fill_g, fill_b)):
        if not 0 <= int(v) <= 255:
            raise ValueError("occlusion_desc: the fill colour is three bytes; got %r" % ((fill_r, fill_g, fill_b),))
        d.fill_rgb[i] = int(v)
    return d


def occlusion_grid(desc):
    """-> (Gy, Gx) of the descriptor's grid of rectangles (rpe_occlusion_grid, host only); ValueError for a refused descriptor"""
    from ._lib import raw
    gy, gx = ctypes.c_int(0), ctypes.c_int(0)
    if raw.rpe_occlusion_grid(ctypes.byref(desc), ctypes.byref(gy), ctypes.byref(gx)) < 0:
        raise ValueError(raw.rpe_last_error().decode())
    return gy.value, gx.value


def occlude_grid_u8(frame, desc, b, k0, out=None):
    """frame uint8 (Hs, Ws, 3) contiguous -> uint8 (b, Hs, Ws, 3): row 0 the frame, row r >= 1 the frame with rectangle k0 + r - 1 of
    the descriptor's grid set to its fill colour, rows past the last rectangle the frame again (rpe_occlude_grid_u8).  out: destination,
    contiguous, not overlapping the frame."""
    if frame.dtype != torch.uint8 or tuple(frame.shape) != (desc.Hs, desc.Ws, 3):
        raise ValueError("occlude_grid_u8: frame must be uint8 (%d, %d, 3); got %s %r" % (desc.Hs, desc.Ws, frame.dtype, tuple(frame.shape)))
    shape = (int(b), desc.Hs, desc.Ws, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=frame.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != frame.device:
        raise ValueError("occlude_grid_u8: out must be uint8 %r on the frame's device" % (shape,))
    lib.rpe_occlude_grid_u8(_p(_chk(frame, "frame")), _p(_chk(out, "out")), int(b), int(k0), ctypes.byref(desc), _stream())
    return out


def pose_displacement(pred, ref, pos=None, ori=None):
    """pred (..., 7) fp32 contiguous, ref (7,) fp32 on the same device -> (pos (...), ori (...)): the distance and the rotation angle
    between each pose and `ref`, computed in double and rounded once (rpe_pose_displacement); exactly (0, 0) for a row equal to ref.
    pos / ori: contiguous fp32 destinations of pred's leading shape.  Enqueued on the current stream; nothing is read back."""
    if pred.dim() < 1 or pred.shape[-1] != 7 or pred.numel() == 0 or ref.numel() != 7:
        raise ValueError("pose_displacement: pred must be (..., 7) and ref (7,); got %r and %r" % (tuple(pred.shape), tuple(ref.shape)))
    if pred.dtype != torch.float32 or ref.dtype != torch.float32 or ref.device != pred.device:
        raise TypeError("pose_displacement: pred and ref must be fp32 on one device")
    lead = tuple(pred.shape[:-1])
    outs = []
    for t, name in ((pos, "pos"), (ori, "ori")):
        if t is None:
            t = torch.empty(lead, dtype=torch.float32, device=pred.device)
        elif t.dtype != torch.float32 or tuple(t.shape) != lead or t.device != pred.device:
            raise ValueError("pose_displacement: %s must be fp32 %r on pred's device" % (name, lead))
        outs.append(_chk(t, name))
    lib.rpe_pose_displacement(_p(_chk(pred, "pred")), _p(_chk(ref, "ref")), pred.numel() // 7, _p(outs[0]), _p(outs[1]), _stream())
    return outs[0], outs[1]


def saliency_map(scores, desc):
    """scores (M, K) or (M, Gy, Gx) fp32 contiguous -> (maps (M, Hs, Ws) fp32, minmax (M, 2) fp32): every pixel the mean of the scores of
    the rectangles covering it, and each map's range over its finite values (rpe_saliency_map)."""
    gy, gx = occlusion_grid(desc)
    if scores.dtype != torch.float32 or scores.dim() not in (2, 3) or scores.numel() != scores.shape[0] * gy * gx or scores.numel() == 0:
        raise ValueError("saliency_map: scores must be fp32 (M, %d) or (M, %d, %d); got %s %r" % (gy * gx, gy, gx, scores.dtype, tuple(scores.shape)))
    m = scores.shape[0]
    maps = torch.empty((m, desc.Hs, desc.Ws), dtype=torch.float32, device=scores.device)
    minmax = torch.empty((m, 2), dtype=torch.float32, device=scores.device)
    lib.rpe_saliency_map(_p(_chk(scores, "scores")), m, ctypes.byref(desc), _p(maps), _p(minmax), _stream())
    return maps, minmax


def saliency_overlay_u8(frame, smap, minmax, table, alpha_q8, fade=False):
    """frame uint8 (Hs, Ws, 3), smap fp32 (Hs, Ws), minmax fp32 (2,), table uint8 (256, 3), all contiguous on one device -> uint8
    (Hs, Ws, 3): the map drawn over the frame through the colour table with weight alpha_q8 / 256, or, with `fade`, a weight that
    grows with the value (rpe_saliency_overlay_u8)."""
    if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[-1] != 3 or frame.numel() == 0:
        raise ValueError("saliency_overlay_u8: frame must be uint8 (Hs, Ws, 3); got %s %r" % (frame.dtype, tuple(frame.shape)))
    hs, ws = frame.shape[:2]
    dev = frame.device
    if smap.dtype != torch.float32 or tuple(smap.shape) != (hs, ws) or minmax.dtype != torch.float32 or minmax.numel() != 2:
        raise ValueError("saliency_overlay_u8: the map must be fp32 (%d, %d) and minmax fp32 (2,)" % (hs, ws))
    if table.dtype != torch.uint8 or tuple(table.shape) != (256, 3):
        raise ValueError("saliency_overlay_u8: the colour table is uint8 (256, 3)")
    if smap.device != dev or minmax.device != dev or table.device != dev:
        raise ValueError("saliency_overlay_u8: all tensors must be on the frame's device")
    out = torch.empty_like(frame)
    lib.rpe_saliency_overlay_u8(_p(_chk(frame, "frame")), _p(_chk(smap, "map")), _p(_chk(minmax, "minmax")), _p(_chk(table, "table")), hs, ws, int(alpha_q8),
                                int(bool(fade)), _p(out), _stream())
    return out


# the flat list form `torch.ops.rpe.draw_poses_u8` takes: these 17 integers per pose set
OVERLAY_STYLE_FIELDS = ("r", "g", "b", "x_r", "x_g", "x_b", "y_r", "y_g", "y_b", "z_r", "z_g", "z_b", "alpha_q8", "r_q4", "hw_q4", "trail", "trail_r_q4")
OVERLAY_AXIS_COLOURS = ((230, 40, 40), (40, 200, 40), (60, 90, 255))


def _colour(name, c):
    try:
        vals = tuple(int(v) for v in c)
    except TypeError:
        vals = ()
    if len(vals) != 3 or not all(0 <= v <= 255 for v in vals):
        raise ValueError("%s: a colour is three bytes; got %r" % (name, c))
    return vals


def overlay_style(colour=(255, 255, 255), alpha_q8=256, r_q4=64, hw_q4=24, axis_colours=OVERLAY_AXIS_COLOURS, trail=0, trail_r_q4=32):
    """rpe_overlay_style, how one pose set is drawn: the disc's and the trail's colour, opacity alpha_q8 in [0, 256], disc radius r_q4,
    half the axes' width hw_q4 and the trail's radius trail_r_q4 in sixteenths of a pixel (each at most 256), the three axes' colours
    and the trail length in frames (at most 64).  ValueError for anything rpe_draw_poses_u8 would refuse."""
    from ._lib import OVERLAY_MAX_RADIUS_Q4, OVERLAY_MAX_TRAIL, OverlayStyle
    s = OverlayStyle()
    for i, v in enumerate(_colour("overlay_style", colour)):
        s.rgb[i] = v
    axes = tuple(axis_colours)
    if len(axes) != 3:
        raise ValueError("overlay_style: axis_colours are three colours; got %r" % (axis_colours,))
    for k, c in enumerate(axes):
        for i, v in enumerate(_colour("overlay_style", c)):
            s.axis_rgb[3 * k + i] = v
    if not 0 <= int(alpha_q8) <= 256:
        raise ValueError("overlay_style: alpha_q8 lies in [0, 256]; got %r" % (alpha_q8,))
    for name, v in (("r_q4", r_q4), ("hw_q4", hw_q4), ("trail_r_q4", trail_r_q4)):
        if not 0 <= int(v) <= OVERLAY_MAX_RADIUS_Q4:
            raise ValueError("overlay_style: %s lies in [0, %d] (sixteenths of a pixel); got %r" % (name, OVERLAY_MAX_RADIUS_Q4, v))
    if not 0 <= int(trail) <= OVERLAY_MAX_TRAIL:
        raise ValueError("overlay_style: the trail length lies in [0, %d]; got %r" % (OVERLAY_MAX_TRAIL, trail))
    s.alpha_q8, s.r_q4, s.hw_q4, s.trail, s.trail_r_q4 = int(alpha_q8), int(r_q4), int(hw_q4), int(trail), int(trail_r_q4)
    return s


def overlay_style_from_list(vals):
    """the 17 integers of OVERLAY_STYLE_FIELDS -> rpe_overlay_style"""
    if len(vals) != len(OVERLAY_STYLE_FIELDS):
        raise ValueError("a pose set's style has %d integers (%s)" % (len(OVERLAY_STYLE_FIELDS), ", ".join(OVERLAY_STYLE_FIELDS)))
    v = [int(x) for x in vals]
    return overlay_style(v[0:3], v[12], v[13], v[14], (v[3:6], v[6:9], v[9:12]), v[15], v[16])


def overlay_style_to_list(s):
    return list(s.rgb) + list(s.axis_rgb) + [s.alpha_q8, s.r_q4, s.hw_q4, s.trail, s.trail_r_q4]


def project_poses(poses, cam, cam_index, axis_len=0.05, pos_err=None, ori_err=None, pos_full=0.1, ori_full=0.5, width=0):
    """poses fp32 (F, G, 7) with G <= 4, cam fp64 (C, 3, 4), cam_index int32 (F,), all contiguous on one device -> (points int32
    (F, G, 4, 2), bars int32 (F, 2)): per pose the centre and the tips of the three axes of length `axis_len` in sixteenths of a pixel
    ([u w, v w, w] = P [x, y, z, 1], fp64), _lib.OVERLAY_INVALID where there is nothing to draw; with pos_err / ori_err fp32 (F,) the
    lengths of the two error bars of a frame `width` pixels wide, full at pos_full / ori_full (rpe_project_poses)."""
    from ._lib import OVERLAY_MAX_SETS, OVERLAY_MAX_SIDE
    if poses.dtype != torch.float32 or poses.dim() != 3 or poses.shape[2] != 7 or poses.numel() == 0 or poses.shape[1] > OVERLAY_MAX_SETS:
        raise ValueError("project_poses: poses must be fp32 (F, G, 7) with 1 <= G <= %d; got %s %r" % (OVERLAY_MAX_SETS, poses.dtype, tuple(poses.shape)))
    f, g = poses.shape[:2]
    dev = poses.device
    if cam.dtype != torch.float64 or cam.dim() != 3 or tuple(cam.shape[1:]) != (3, 4) or cam.shape[0] < 1 or cam.device != dev:
        raise ValueError("project_poses: cam must be fp64 (C, 3, 4) on the poses' device; got %s %r" % (cam.dtype, tuple(cam.shape)))
    if cam_index.dtype != torch.int32 or tuple(cam_index.shape) != (f,) or cam_index.device != dev:
        raise ValueError("project_poses: cam_index must be int32 (%d,) on the poses' device" % f)
    if (pos_err is None) != (ori_err is None):
        raise ValueError("project_poses: pos_err and ori_err come together")
    for t, name in ((pos_err, "pos_err"), (ori_err, "ori_err")):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (f,) or t.device != dev):
            raise ValueError("project_poses: %s must be fp32 (%d,) on the poses' device" % (name, f))
    axis_len, pos_full, ori_full, width = float(axis_len), float(pos_full), float(ori_full), int(width)
    if not (math.isfinite(axis_len) and math.isfinite(pos_full) and math.isfinite(ori_full) and pos_full > 0 and ori_full > 0):
        raise ValueError("project_poses: axis_len must be finite, pos_full and ori_full finite and positive; got %r, %r, %r" % (axis_len, pos_full, ori_full))
    if not 0 <= width <= OVERLAY_MAX_SIDE:
        raise ValueError("project_poses: the width lies in [0, %d]; got %r" % (OVERLAY_MAX_SIDE, width))
    points = torch.empty((f, g, 4, 2), dtype=torch.int32, device=dev)
    bars = torch.empty((f, 2), dtype=torch.int32, device=dev)
    lib.rpe_project_poses(_p(_chk(poses, "poses")), _p(_chk(cam, "cam")), _p(_chk(cam_index, "cam_index")), f, g, cam.shape[0], axis_len,
                          _p(None if pos_err is None else _chk(pos_err, "pos_err")), _p(None if ori_err is None else _chk(ori_err, "ori_err")), pos_full,
                          ori_full, width, _p(points), _p(bars), _stream())
    return points, bars


OVERLAY_BAR_COLOURS = ((255, 255, 255), (255, 200, 0))


def draw_poses_u8(frames, points, bars, styles, *, frames_per_episode=1, first=0, bar_px=0, bar_colours=OVERLAY_BAR_COLOURS, flip=False, out=None):
    """frames uint8 (n, Hs, Ws, 3), points int32 (F, G, 4, 2) and bars int32 (F, 2) as `project_poses` writes them with F >= first + n,
    all contiguous on one device; styles: G `overlay_style`s -> uint8 (n, Hs, Ws, 3), frame i annotated with entry first + i of the
    list: per pose set the trail of the earlier centres of the same episode (`frames_per_episode` entries each), the three axes and the
    disc; with bar_px > 0 two error bars of that height at the bottom of the output, in `bar_colours`; with `flip` the rows are
    written bottom up.  Integer arithmetic only (rpe_draw_poses_u8).  out: destination, contiguous, not overlapping the frames."""
    from ._lib import OVERLAY_MAX_SETS, OVERLAY_MAX_SIDE, OverlayStyle
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or frames.numel() == 0:
        raise ValueError("draw_poses_u8: frames must be uint8 (n, Hs, Ws, 3); got %s %r" % (frames.dtype, tuple(frames.shape)))
    n, hs, ws = frames.shape[:3]
    dev = frames.device
    if hs > OVERLAY_MAX_SIDE or ws > OVERLAY_MAX_SIDE:
        raise ValueError("draw_poses_u8: frames are at most %d pixels a side; got %d x %d" % (OVERLAY_MAX_SIDE, hs, ws))
    styles = list(styles)
    g = len(styles)
    if not 1 <= g <= OVERLAY_MAX_SETS or not all(isinstance(s, OverlayStyle) for s in styles):
        raise ValueError("draw_poses_u8: styles are 1..%d overlay_style(...) values, one per pose set" % OVERLAY_MAX_SETS)
    first, fpe, bar_px = int(first), int(frames_per_episode), int(bar_px)
    if points.dtype != torch.int32 or points.dim() != 4 or tuple(points.shape[1:]) != (g, 4, 2) or points.device != dev:
        raise ValueError("draw_poses_u8: points must be int32 (F, %d, 4, 2) on the frames' device; got %s %r" % (g, points.dtype, tuple(points.shape)))
    if bars.dtype != torch.int32 or tuple(bars.shape) != (points.shape[0], 2) or bars.device != dev:
        raise ValueError("draw_poses_u8: bars must be int32 (%d, 2) on the frames' device" % points.shape[0])
    if first < 0 or first + n > points.shape[0]:
        raise ValueError("draw_poses_u8: frames %d .. %d are not in a list of %d" % (first, first + n - 1, points.shape[0]))
    if fpe < 1:
        raise ValueError("draw_poses_u8: frames_per_episode must be at least 1; got %r" % (frames_per_episode,))
    if bar_px < 0 or 2 * bar_px > hs:
        raise ValueError("draw_poses_u8: two bars of %d rows do not fit %d rows" % (bar_px, hs))
    cols = tuple(bar_colours)
    if len(cols) != 2:
        raise ValueError("draw_poses_u8: bar_colours are two colours; got %r" % (bar_colours,))
    rgb6 = (ctypes.c_ubyte * 6)(*(_colour("draw_poses_u8", cols[0]) + _colour("draw_poses_u8", cols[1])))
    if out is None:
        out = torch.empty_like(frames)
    elif out.dtype != torch.uint8 or tuple(out.shape) != tuple(frames.shape) or out.device != dev:
        raise ValueError("draw_poses_u8: out must be uint8 %r on the frames' device" % (tuple(frames.shape),))
    arr = (OverlayStyle * g)(*styles)
    lib.rpe_draw_poses_u8(_p(_chk(frames, "frames")), _p(_chk(out, "out")), n, hs, ws, _p(_chk(points, "points")), _p(_chk(bars, "bars")), first, g, arr,
                          fpe, bar_px, rgb6, int(bool(flip)), _stream())
    return out


MEASURE_MAX_SCALES = 8
# the flat list form `torch.ops.rpe.measurement_noise` takes: these five numbers, then the 1..8 variances (the seed travels as two
# 32-bit words because a double does not hold 64 bits)
MEASURE_DESC_NUMBERS = ("seed_lo", "seed_hi", "S", "N", "correlation")


def measure_scales(scales):
    """`scales` -- one variance or a sequence of 1..8 -- as a tuple of floats; ValueError unless each is finite and not negative"""
    try:
        vals = tuple(float(v) for v in scales)
    except TypeError:
        vals = (float(scales),)
    if not 1 <= len(vals) <= MEASURE_MAX_SCALES:
        raise ValueError("measurement noise takes 1..%d scales; got %d" % (MEASURE_MAX_SCALES, len(vals)))
    for v in vals:
        if not (v >= 0.0 and math.isfinite(v)):
            raise ValueError("a measurement-noise scale is a variance, finite and not negative; got %r" % (v,))
    return vals


def measure_desc(seed=0, S=1, N=1, scales=(0.001,), correlation=0.0):
    """rpe_measure_desc: `scales` are VARIANCES (one or a sequence of 1..8; sigma = sqrt(variance) is taken here, in double),
    `correlation` the AR(1) coefficient along S in [0, 1).  ValueError for anything the kernel would refuse."""
    from ._lib import MeasureDesc
    seed, s, n, rho = int(seed), int(S), int(N), float(correlation)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("measure_desc: seed must fit 64 unsigned bits; got %r" % (seed,))
    if s < 1 or n < 1 or s * n >= 2 ** 31:
        raise ValueError("measure_desc: S and N must be at least 1 and S * N below 2^31; got S = %r, N = %r" % (S, N))
    if not 0.0 <= rho < 1.0:
        raise ValueError("measure_desc: correlation must lie in [0, 1); got %r" % (correlation,))
    vals = measure_scales(scales)
    d = MeasureDesc()
    d.seed, d.S, d.N, d.num_scales, d.rho = seed, s, n, len(vals), rho
    for k, v in enumerate(vals):
        d.sigma[k] = math.sqrt(v)
    return d


def measurement_noise(x0, desc, state, picks=None, out=None):
    """x0 fp32 (..., 7) contiguous, desc.S * desc.N rows (x, y, z, qx, qy, qz, qw), time-major -> x0 + noise with the quaternion
    renormalised, fp32 of the same shape (rpe_measurement_noise).  desc: measure_desc(...).  state: int32 device tensor whose
    element 0 is the step counter; the launch advances it by one.  picks: int32 (1 + N,) device tensor receiving the step used and
    each lane's scale index (allocated when not given).  out: destination (may be `x0` itself)."""
    if x0.dtype != torch.float32 or x0.dim() < 2 or x0.shape[-1] != 7:
        raise ValueError("measurement_noise: x0 must be fp32 (..., 7); got %s %r" % (x0.dtype, tuple(x0.shape)))
    _chk(x0, "x0")
    n = int(desc.N)
    if x0.numel() != int(desc.S) * n * 7 or x0.numel() == 0:
        raise ValueError("measurement_noise: x0 has %d rows, the descriptor S * N = %d * %d" % (x0.numel() // 7, desc.S, desc.N))
    dev = x0.device
    if state.dtype != torch.int32 or state.numel() < 1 or state.device != dev:
        raise ValueError("measurement_noise: state must be an int32 tensor on x0's device")
    if out is None:
        out = torch.empty_like(x0)
    elif out.dtype != torch.float32 or out.shape != x0.shape or out.device != dev:
        raise ValueError("measurement_noise: out must be fp32 of x0's shape on its device")
    _chk(out, "out")
    if picks is None:
        picks = torch.empty(1 + n, dtype=torch.int32, device=dev)
    elif picks.dtype != torch.int32 or picks.numel() < 1 + n or picks.device != dev:
        raise ValueError("measurement_noise: picks must be int32 with at least %d elements on x0's device" % (1 + n))
    lib.rpe_measurement_noise(_p(x0), _p(out), ctypes.byref(desc), _p(_chk(state, "state")), _p(_chk(picks, "picks")), _stream())
    return out


DROPOUT_SITES = 4


def dropout_desc(p, seed=0):
    """rpe_dropout_desc of drop probability p in [0, 1): thresh = min(2^32 - 1, round(p 2^32)) (the rule of the depth augmentation's
    drop_thresh), scale = float32(1 / (1 - p)) divided in double and rounded once; seed: the 64-bit Philox key.  p = 0 gives thresh 0
    and scale 1: nothing would be dropped, and callers launch nothing (PoseModelBase.set_dropout leaves such a site off)."""
    from ._lib import DropoutDesc
    p, seed = float(p), int(seed)
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout_desc: p must lie in [0, 1); got %r" % (p,))
    if not 0 <= seed < 2 ** 64:
        raise ValueError("dropout_desc: seed must fit 64 unsigned bits; got %r" % (seed,))
    d = DropoutDesc()
    d.seed, d.thresh, d.scale = seed, min(2 ** 32 - 1, int(round(p * 2 ** 32))), 1.0 / (1.0 - p)
    return d


def _dropout_word(t, dev, name):
    """`state` / `picks` of the dropout entry points: a contiguous int32 tensor on the device `dev` (None: any GPU)"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.numel() < 1 or not t.is_cuda or (dev is not None and t.device != dev):
        raise ValueError("%s must be an int32 tensor on the device" % name)
    return _chk(t, name)


def dropout_begin(state, picks):
    """picks[0] <- the step counter state[0], which then advances by one, wrapping at 2^32 (rpe_dropout_begin): once per train step,
    in front of its dropout_rows launches.  state, picks: int32 device tensors (the counter's 32 bits are stored as they are)."""
    _dropout_word(state, None, "dropout_begin: state")
    _dropout_word(picks, state.device, "dropout_begin: picks")
    lib.rpe_dropout_begin(_p(state), _p(picks), _stream())
    return picks


def dropout_rows(x, desc, picks, site=0, c0=0, c1=None, out=None):
    """Inverted dropout of columns [c0, c1) of the fp32 row matrix x [n, cols] (any row stride; unit column stride), the mask of step
    picks[0] and of `site` (0..3): kept elements are multiplied by desc.scale, dropped ones become +0.0 (rpe_dropout_rows_f32).
    out: None or x itself = in place; otherwise a matrix of x's shape and row stride that shares no memory with it, of which only
    the columns [c0, c1) are written.  The same call masks the gradient in the backward.  Returns out."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.numel() == 0 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise ValueError("dropout_rows: x must be a non-empty fp32 matrix with unit column stride")
    if not x.is_cuda:
        raise ValueError("dropout_rows: x must be on the device (there is no CPU path)")
    n, cols = x.shape
    ld = x.stride(0) if n > 1 else max(x.stride(0), cols)
    c1 = cols if c1 is None else int(c1)
    c0, site = int(c0), int(site)
    if not 0 <= c0 < c1 <= cols:
        raise ValueError("dropout_rows: the columns must satisfy 0 <= c0 < c1 <= %d; got [%d, %d)" % (cols, c0, c1))
    if not 0 <= site < DROPOUT_SITES:
        raise ValueError("dropout_rows: site must lie in [0, %d); got %r" % (DROPOUT_SITES, site))
    if ld < cols or ld >= 2 ** 31:
        raise ValueError("dropout_rows: the row stride must be at least the column count (rows may not overlap); got %d for %d columns" % (ld, cols))
    _dropout_word(picks, x.device, "dropout_rows: picks")
    if out is None:
        out = x
    elif out is not x:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (n, cols) or out.device != x.device \
                or (n > 1 and out.stride(0) != ld) or (cols > 1 and out.stride(1) != 1):
            raise ValueError("dropout_rows: out must be fp32 of x's shape and row stride on its device")
    lib.rpe_dropout_rows_f32(_p(x), _p(out), n, ld, c0, c1, site, _p(picks), ctypes.byref(desc), _stream())
    return out
