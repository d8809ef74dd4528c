"""PyTorch dispatcher registration of the HIP operators: `torch.ops.rpe.*`.

The product boundary is the C ABI (include/rpe_hip.h); the model classes reach it through ctypes (ops.py, engine.py).  This module is
the INNER face SURVEY.md section 8(b) describes for a maintainer who wants the operators as PyTorch custom ops: every entry is
registered with the dispatcher for the CUDA (= HIP on ROCm) device type ONLY -- a call with CPU tensors fails in the dispatcher
("no implementation for device cpu"), there is no fallback -- with a fake (meta) implementation giving shapes / dtypes, and the two
differentiable ones (`rpe::conv2d`, `rpe::pose_distance_loss`) carry their backward formulas, built from the same HIP launches.

Each operator names the torch call of the reference's hot path it stands for (models/naive.py:316 runs them through torchvision's
ResNet; models/losses.py:114-128 is the loss; util/learn_utils.py:152-184 the step):

    rpe::conv2d_fwd / conv2d_dgrad / conv2d_wgrad   F.conv2d and its two gradients, NHWC activations, [Co,kh,kw,Ci] weights
    rpe::conv2d                                     the three as ONE differentiable op
    rpe::bn_apply                                   BatchNorm's affine map (+ residual) (+ ReLU) on an NHWC tensor
    rpe::linear_fwd                                 F.linear (+ ReLU)
    rpe::pose_loss / pose_distance_loss             PoseDistanceLoss (raw three-value form / differentiable scalar)
    rpe::pose_errors                                its "val" branch per sample: position error, |angle| error, unit-quaternion pose
    rpe::adam_step                                  torch.optim.Adam's update of one flat fp32 tensor, in place
    rpe::param_stats                                torch._foreach_norm over gradients and parameters, isfinite / zero counts and the update norm per tensor, two launches
    rpe::augment_frames_u8                          (no counterpart: the reference does not augment) jitter, noise and erasing of raw uint8 frames
    rpe::blur_frames_u8                             (no counterpart) defocus and motion blur of raw uint8 frames, in front of rpe::augment_frames_u8
    rpe::augment_depth_f32                          (no counterpart) depth-sensor model on raw fp32 depth: range noise, quantisation, clamp, dropout, holes, the RGB occluder
    rpe::sample_windows / gather_rows               DataLoader(shuffle=True) over episode windows resident in HBM: the batch's index, and its rows
    rpe::sample_windows_ragged / pose_loss_masked / (no counterpart: the reference's episodes all have one length) the window index, the summed loss and the
    rpe::error_stats_ragged                         error statistics of episodes of unequal length, padded to one horizon: padding is never drawn or read
    rpe::measurement_noise                          x0 + sqrt(scale) * randn_like(x0) with the quaternion renormalised (util/data_utils.py:162-167), drawn on the device
    rpe::dropout_begin / dropout_rows               F.dropout on a column range of the rows the heads read (the `dropout_prob` the reference accepts and never applies),
                                                    the mask drawn on the device from a step counter in device memory
    rpe::occlude_grid_u8 / pose_displacement /      (no counterpart: occlusion sensitivity) a frame with one rectangle of a grid covered per row; how far
    rpe::saliency_map / saliency_overlay_u8         each prediction moved; the scores spread over the pixels; the map drawn over the frame
    rpe::project_poses / draw_poses_u8              the recorded video of rollout() (util/learn_utils.py:401-403, 462-504) without the simulator: poses through a camera
                                                    matrix to an integer draw list; the list drawn on the recorded uint8 frames

Importing this module needs torch only; the HIP library is loaded on the first call (ops.py), so the schemas can be inspected on a
machine without a GPU (tests/test_host_cpu.py).
"""
from typing import List, Optional, Tuple

import torch

__all__ = ["NAMES"]

_NS = "rpe"
NAMES = ("conv2d_fwd", "conv2d_dgrad", "conv2d_wgrad", "conv2d", "bn_apply", "linear_fwd", "pose_loss", "pose_distance_loss", "pose_errors", "adam_step", "augment_frames_u8", "blur_frames_u8", "augment_depth_f32", "sample_windows", "gather_rows",
         "sample_windows_ragged", "pose_loss_masked", "error_stats_ragged", "measurement_noise", "occlude_grid_u8", "pose_displacement", "saliency_map", "saliency_overlay_u8", "param_stats", "project_poses", "draw_poses_u8", "dropout_begin", "dropout_rows")


def _ops():
    from . import ops   # (loads librpe_hip.so: raises ImportError with the build instructions when it is missing)
    return ops


def _out_hw(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


# ---- convolution (NHWC, compute dtype fp32 / bf16 / fp16) ---------------------------------------------------------------------
@torch.library.custom_op(_NS + "::conv2d_fwd", mutates_args=(), device_types="cuda")
def conv2d_fwd(x: torch.Tensor, w_krsc: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
    return _ops().conv2d_fwd(x, w_krsc, stride, pad)


@conv2d_fwd.register_fake
def _(x, w_krsc, stride, pad):
    ho, wo = _out_hw(x.shape[1], x.shape[2], w_krsc.shape[1], stride, pad)
    return x.new_empty((x.shape[0], ho, wo, w_krsc.shape[0]))


@torch.library.custom_op(_NS + "::conv2d_dgrad", mutates_args=(), device_types="cuda")
def conv2d_dgrad(dy: torch.Tensor, w_crsk: torch.Tensor, x_shape: List[int], stride: int, pad: int) -> torch.Tensor:
    return _ops().conv2d_dgrad(dy, w_crsk, tuple(x_shape), stride, pad)


@conv2d_dgrad.register_fake
def _(dy, w_crsk, x_shape, stride, pad):
    return dy.new_empty(tuple(x_shape))


@torch.library.custom_op(_NS + "::conv2d_wgrad", mutates_args=(), device_types="cuda")
def conv2d_wgrad(x: torch.Tensor, dy: torch.Tensor, k: int, stride: int, pad: int) -> torch.Tensor:
    """-> fp32 [Co, k, k, Ci], the deterministic form (per-workgroup slabs summed in a fixed order)"""
    return _ops().conv2d_wgrad(x, dy, k, stride, pad, deterministic=True)


@conv2d_wgrad.register_fake
def _(x, dy, k, stride, pad):
    return x.new_empty((dy.shape[3], k, k, x.shape[3]), dtype=torch.float32)


@torch.library.custom_op(_NS + "::conv2d", mutates_args=(), device_types="cuda")
def conv2d(x: torch.Tensor, w_krsc: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
    """differentiable: x [B,H,W,Ci] and w [Co,kh,kw,Ci] of one compute dtype; d/dw comes back in that dtype (rounded from the fp32 sum)"""
    return _ops().conv2d_fwd(x, w_krsc, stride, pad)


@conv2d.register_fake
def _(x, w_krsc, stride, pad):
    ho, wo = _out_hw(x.shape[1], x.shape[2], w_krsc.shape[1], stride, pad)
    return x.new_empty((x.shape[0], ho, wo, w_krsc.shape[0]))


def _conv2d_setup(ctx, inputs, output):
    x, w, stride, pad = inputs
    ctx.save_for_backward(x, w)
    ctx.stride, ctx.pad = stride, pad


def _conv2d_backward(ctx, dy):
    x, w = ctx.saved_tensors
    dy = dy.contiguous()
    dx = dw = None
    if ctx.needs_input_grad[0]:
        w_crsk = w.permute(3, 1, 2, 0).contiguous()   # [Ci, kh, kw, Co]: the data gradient's weight layout
        dx = torch.ops.rpe.conv2d_dgrad(dy, w_crsk, list(x.shape), ctx.stride, ctx.pad)
    if ctx.needs_input_grad[1]:
        dw = torch.ops.rpe.conv2d_wgrad(x, dy, w.shape[1], ctx.stride, ctx.pad).to(w.dtype)
    return dx, dw, None, None


conv2d.register_autograd(_conv2d_backward, setup_context=_conv2d_setup)


# ---- BatchNorm affine map, Linear ---------------------------------------------------------------------------------------------
@torch.library.custom_op(_NS + "::bn_apply", mutates_args=(), device_types="cuda")
def bn_apply(y: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, residual: Optional[torch.Tensor], relu: bool) -> torch.Tensor:
    return _ops().bn_apply(y, scale, shift, residual, relu)


@bn_apply.register_fake
def _(y, scale, shift, residual, relu):
    return torch.empty_like(y)


@torch.library.custom_op(_NS + "::linear_fwd", mutates_args=(), device_types="cuda")
def linear_fwd(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], relu: bool) -> torch.Tensor:
    return _ops().linear_fwd(x, w, bias, relu).contiguous()


@linear_fwd.register_fake
def _(x, w, bias, relu):
    return x.new_empty((x.shape[0], w.shape[0]))


# ---- PoseDistanceLoss ------------------------------------------------------------------------------------------------------------
@torch.library.custom_op(_NS + "::pose_loss", mutates_args=(), device_types="cuda")
def pose_loss(pred: torch.Tensor, truth: torch.Tensor, metric: int, mode: int, scale: float, alpha: float, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> ([loss, val position error, val orientation error] fp32, d loss / d pred); metric 0 l2, 1 l1, 2 linf, 3 combined; mode 0 position, 1 pose (the two validation metrics are always in elements 1, 2)"""
    out3, grad = _ops().pose_loss(pred, truth, metric, mode, scale, alpha, eps, want_grad=True)
    return out3, grad


@pose_loss.register_fake
def _(pred, truth, metric, mode, scale, alpha, eps):
    return pred.new_empty((3,)), torch.empty_like(pred)


@torch.library.custom_op(_NS + "::pose_distance_loss", mutates_args=(), device_types="cuda")
def pose_distance_loss(pred: torch.Tensor, truth: torch.Tensor, metric: int, mode: int, scale: float, alpha: float, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """differentiable in pred: -> (scalar loss, its gradient w.r.t. pred -- saved for the backward, not differentiable itself)"""
    out3, grad = _ops().pose_loss(pred, truth, metric, mode, scale, alpha, eps, want_grad=True)
    return out3[0].clone(), grad


@pose_distance_loss.register_fake
def _(pred, truth, metric, mode, scale, alpha, eps):
    return pred.new_empty(()), torch.empty_like(pred)


def _pdl_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])


def _pdl_backward(ctx, dloss, _dgrad):
    (g,) = ctx.saved_tensors
    return g * dloss, None, None, None, None, None, None


pose_distance_loss.register_autograd(_pdl_backward, setup_context=_pdl_setup)


@torch.library.custom_op(_NS + "::pose_errors", mutates_args=(), device_types="cuda")
def pose_errors(pred: torch.Tensor, truth: torch.Tensor, eps: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """pred, truth (n, 7) fp32 -> (position error (n,), |angle| error in radians (n,), pred with a unit quaternion (n, 7)): the "val" mode of PoseDistanceLoss per sample"""
    pos, ori, pose = _ops().pose_errors(pred, truth, eps, want_pose=True)
    return pos, ori, pose


@pose_errors.register_fake
def _(pred, truth, eps):
    return pred.new_empty(pred.shape[:-1]), pred.new_empty(pred.shape[:-1]), torch.empty_like(pred)


# ---- Adam ------------------------------------------------------------------------------------------------------------------------
@torch.library.custom_op(_NS + "::adam_step", mutates_args=("p", "m", "v"), device_types="cuda")
def adam_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, lr: float, beta1: float, beta2: float, eps: float, step: int) -> None:
    _ops().adam_step(p, g, m, v, lr, beta1, beta2, eps, step)


# ---- training telemetry --------------------------------------------------------------------------------------------------------
@torch.library.custom_op(_NS + "::param_stats", mutates_args=("partials", "out"), device_types="cuda")
def param_stats(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, table: torch.Tensor, table_host: torch.Tensor, partials: torch.Tensor,
                out: torch.Tensor, beta1: float, beta2: float, eps: float, state: torch.Tensor, every: int) -> None:
    """per-tensor statistics of the four fp32 arenas into out fp64 (T, 10), columns ops.PARAM_STATS_COLUMNS; table / table_host:
    ops.param_stats_table(...) on the device / on the host; written only when (long)state[5] % every == 0"""
    _ops().param_stats(p, g, m, v, table, table_host, partials, out, beta1, beta2, eps, state, every)


# ---- frame augmentation --------------------------------------------------------------------------------------------------------
@torch.library.custom_op(_NS + "::augment_frames_u8", mutates_args=("state",), device_types="cuda")
def augment_frames_u8(frames: torch.Tensor, desc: List[int], state: torch.Tensor) -> torch.Tensor:
    """frames uint8 (..., Hs, Ws, 3) -> augmented uint8 frames; desc: the integers of rpe_augment_desc in the order of
    ops.AUGMENT_DESC_FIELDS; state: int32, element 0 is the step counter, advanced by one"""
    ops = _ops()
    if len(desc) != len(ops.AUGMENT_DESC_FIELDS):
        raise ValueError("augment_frames_u8: desc has %d integers (%s)" % (len(ops.AUGMENT_DESC_FIELDS), ", ".join(ops.AUGMENT_DESC_FIELDS)))
    return ops.augment_frames_u8(frames, ops.augment_desc(**dict(zip(ops.AUGMENT_DESC_FIELDS, desc))), state)


@augment_frames_u8.register_fake
def _(frames, desc, state):
    return torch.empty_like(frames)


@torch.library.custom_op(_NS + "::blur_frames_u8", mutates_args=(), device_types="cuda")
def blur_frames_u8(frames: torch.Tensor, desc: List[int], state: torch.Tensor) -> torch.Tensor:
    """frames uint8 (..., Hs, Ws, 3) -> blurred uint8 frames; desc: the integers of rpe_blur_desc as ops.blur_desc_numbers(...) lists
    them; state: int32, element 0 is the step counter, read and NOT advanced (rpe::augment_frames_u8, which follows, advances it)"""
    ops = _ops()
    return ops.blur_frames_u8(frames, ops.blur_desc_from_numbers(desc), state)


@blur_frames_u8.register_fake
def _(frames, desc, state):
    return torch.empty_like(frames)


@torch.library.custom_op(_NS + "::augment_depth_f32", mutates_args=("state",), device_types="cuda")
def augment_depth_f32(depth: torch.Tensor, desc: List[float], state: torch.Tensor, rgb_params: Optional[torch.Tensor] = None, rgb_group: int = 0) -> torch.Tensor:
    """depth fp32 (..., Hs, Ws, 1) or (..., 1, H, W) -> augmented fp32 depth; desc: the numbers of ops.DEPTH_AUGMENT_DESC_NUMBERS (the
    seed as two 32-bit words, then the fields of rpe_depth_augment_desc); state: int32, element 0 is the step counter, advanced by
    one; rgb_params / rgb_group: the table rpe::augment_frames_u8's launch wrote for the same batch, for the shared occluder"""
    ops = _ops()
    if len(desc) != len(ops.DEPTH_AUGMENT_DESC_NUMBERS):
        raise ValueError("augment_depth_f32: desc has %d numbers (%s)" % (len(ops.DEPTH_AUGMENT_DESC_NUMBERS), ", ".join(ops.DEPTH_AUGMENT_DESC_NUMBERS)))
    lo, hi = int(desc[0]), int(desc[1])
    if not (0 <= lo < 2 ** 32 and 0 <= hi < 2 ** 32):
        raise ValueError("augment_depth_f32: the seed travels as two 32-bit words; got %r, %r" % (desc[0], desc[1]))
    fields = dict(zip(ops.DEPTH_AUGMENT_DESC_FIELDS[1:], desc[2:]))
    return ops.augment_depth_f32(depth, ops.depth_augment_desc(seed=lo | (hi << 32), **fields), state, rgb_params=rgb_params, rgb_group=rgb_group)


@augment_depth_f32.register_fake
def _(depth, desc, state, rgb_params=None, rgb_group=0):
    return torch.empty_like(depth)


# ---- minibatch sampling from resident episodes ---------------------------------------------------------------------------------
@torch.library.custom_op(_NS + "::sample_windows", mutates_args=("state",), device_types="cuda")
def sample_windows(desc: List[int], sel: torch.Tensor, state: torch.Tensor) -> torch.Tensor:
    """-> int32 (1 + 2 N,): the step used, then per window (episode number in the file, first timestep); desc: the integers of
    rpe_sample_desc in the order of ops.SAMPLE_DESC_FIELDS; sel: int32 episode numbers; state: int32, element 0 is the step
    counter, advanced by one"""
    ops = _ops()
    if len(desc) != len(ops.SAMPLE_DESC_FIELDS):
        raise ValueError("sample_windows: desc has %d integers (%s)" % (len(ops.SAMPLE_DESC_FIELDS), ", ".join(ops.SAMPLE_DESC_FIELDS)))
    return ops.sample_windows(ops.sample_desc(**dict(zip(ops.SAMPLE_DESC_FIELDS, desc))), sel, state)


@sample_windows.register_fake
def _(desc, sel, state):
    return sel.new_empty((1 + 2 * desc[5],))


@torch.library.custom_op(_NS + "::gather_rows", mutates_args=(), device_types="cuda")
def gather_rows(pool: torch.Tensor, index: torch.Tensor, S: int, T: int) -> torch.Tensor:
    """pool (E_file, T, ...) -> (S, N, ...): out[s, n] = pool[index.episode[n], index.t0[n] + s], index as rpe::sample_windows writes it"""
    return _ops().gather_rows(pool, index, S, T)


@gather_rows.register_fake
def _(pool, index, S, T):
    return pool.new_empty((S, (index.shape[0] - 1) // 2) + tuple(pool.shape[2:]))


# ---- episodes of unequal length ------------------------------------------------------------------------------------------------
@torch.library.custom_op(_NS + "::sample_windows_ragged", mutates_args=("state",), device_types="cuda")
def sample_windows_ragged(desc: List[int], sel: torch.Tensor, lengths: torch.Tensor, state: torch.Tensor) -> torch.Tensor:
    """rpe::sample_windows when episode sel[e] has only lengths[sel[e]] timesteps; lengths: int32, one entry per episode in the file"""
    ops = _ops()
    if len(desc) != len(ops.SAMPLE_DESC_FIELDS):
        raise ValueError("sample_windows_ragged: desc has %d integers (%s)" % (len(ops.SAMPLE_DESC_FIELDS), ", ".join(ops.SAMPLE_DESC_FIELDS)))
    return ops.sample_windows_ragged(ops.sample_desc(**dict(zip(ops.SAMPLE_DESC_FIELDS, desc))), sel, lengths, state)


@sample_windows_ragged.register_fake
def _(desc, sel, lengths, state):
    return sel.new_empty((1 + 2 * desc[5],))


@torch.library.custom_op(_NS + "::pose_loss_masked", mutates_args=(), device_types="cuda")
def pose_loss_masked(pred: torch.Tensor, truth: torch.Tensor, valid: torch.Tensor, metric: int, mode: int, scale: float, alpha: float,
                     eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """rpe::pose_loss over the rows valid (uint8 or bool, pred.shape[:-1]) marks; the other rows are never read and get a +0 gradient"""
    out3, grad = _ops().pose_loss(pred, truth, metric, mode, scale, alpha, eps, want_grad=True, valid=valid)
    return out3, grad


@pose_loss_masked.register_fake
def _(pred, truth, valid, metric, mode, scale, alpha, eps):
    return pred.new_empty((3,)), torch.empty_like(pred)


@torch.library.custom_op(_NS + "::error_stats_ragged", mutates_args=(), device_types="cuda")
def error_stats_ragged(err: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
    """err fp32 (E, T), lengths int32 (E,) -> fp64 (3 + 2 E,): mean, population std, max over the valid values, then per-row sums and means"""
    return _ops().error_stats(err, lengths)


@error_stats_ragged.register_fake
def _(err, lengths):
    return err.new_empty((3 + 2 * err.shape[0],), dtype=torch.float64)


# ---- measurement noise ---------------------------------------------------------------------------------------------------------
@torch.library.custom_op(_NS + "::measurement_noise", mutates_args=("state",), device_types="cuda")
def measurement_noise(x0: torch.Tensor, desc: List[float], state: torch.Tensor) -> torch.Tensor:
    """x0 fp32 (S, N, 7) or (B, 7) -> x0 + noise with the quaternion renormalised; desc: the numbers of ops.MEASURE_DESC_NUMBERS
    (seed low word, seed high word, S, N, correlation), then the 1..8 variances; state: int32, element 0 is the step counter,
    advanced by one"""
    ops = _ops()
    k = len(ops.MEASURE_DESC_NUMBERS)
    if not k + 1 <= len(desc) <= k + ops.MEASURE_MAX_SCALES:
        raise ValueError("measurement_noise: desc is %s and then 1..%d variances" % (", ".join(ops.MEASURE_DESC_NUMBERS), ops.MEASURE_MAX_SCALES))
    lo, hi, s, n = (int(v) for v in desc[:4])
    if not (0 <= lo < 2 ** 32 and 0 <= hi < 2 ** 32):
        raise ValueError("measurement_noise: the seed travels as two 32-bit words; got %r, %r" % (desc[0], desc[1]))
    return ops.measurement_noise(x0, ops.measure_desc(seed=lo | (hi << 32), S=s, N=n, scales=list(desc[k:]), correlation=desc[4]), state)


@measurement_noise.register_fake
def _(x0, desc, state):
    return torch.empty_like(x0)


# ---- head dropout --------------------------------------------------------------------------------------------------------------
@torch.library.custom_op(_NS + "::dropout_begin", mutates_args=("state", "picks"), device_types="cuda")
def dropout_begin(state: torch.Tensor, picks: torch.Tensor) -> None:
    """picks[0] <- the step counter state[0], which advances by one (int32 device tensors): once per train step"""
    _ops().dropout_begin(state, picks)


@dropout_begin.register_fake
def _(state, picks):
    return None


@torch.library.custom_op(_NS + "::dropout_rows", mutates_args=(), device_types="cuda")
def dropout_rows(x: torch.Tensor, desc: List[float], picks: torch.Tensor, site: int, c0: int, c1: int) -> torch.Tensor:
    """x fp32 (n, cols) -> a copy whose columns [c0, c1) went through inverted dropout with the mask of step picks[0] and of `site`;
    desc: the seed's low word, its high word, the drop probability p in [0, 1).  The same call masks a gradient."""
    ops = _ops()
    if len(desc) != 3:
        raise ValueError("dropout_rows: desc is seed_lo, seed_hi, p")
    lo, hi = int(desc[0]), int(desc[1])
    if not (0 <= lo < 2 ** 32 and 0 <= hi < 2 ** 32):
        raise ValueError("dropout_rows: the seed travels as two 32-bit words; got %r, %r" % (desc[0], desc[1]))
    d = ops.dropout_desc(desc[2], lo | (hi << 32))
    out = x.contiguous().clone()
    if d.thresh == 0:   # p = 0: nothing is dropped, nothing is launched
        return out
    return ops.dropout_rows(out, d, picks, site=site, c0=c0, c1=c1)


@dropout_rows.register_fake
def _(x, desc, picks, site, c0, c1):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


# ---- occlusion sensitivity -----------------------------------------------------------------------------------------------------
def _occlusion_desc(name, desc):
    ops = _ops()
    if len(desc) != len(ops.OCCLUSION_DESC_FIELDS):
        raise ValueError("%s: desc has %d integers (%s)" % (name, len(ops.OCCLUSION_DESC_FIELDS), ", ".join(ops.OCCLUSION_DESC_FIELDS)))
    return ops.occlusion_desc(**dict(zip(ops.OCCLUSION_DESC_FIELDS, desc)))


@torch.library.custom_op(_NS + "::occlude_grid_u8", mutates_args=(), device_types="cuda")
def occlude_grid_u8(frame: torch.Tensor, desc: List[int], B: int, k0: int) -> torch.Tensor:
    """frame uint8 (Hs, Ws, 3) -> (B, Hs, Ws, 3): row 0 the frame, row r >= 1 the frame with rectangle k0 + r - 1 covered; desc: the
    integers of rpe_occlusion_desc in the order of ops.OCCLUSION_DESC_FIELDS"""
    return _ops().occlude_grid_u8(frame, _occlusion_desc("occlude_grid_u8", desc), B, k0)


@occlude_grid_u8.register_fake
def _(frame, desc, B, k0):
    return frame.new_empty((B,) + tuple(frame.shape))


@torch.library.custom_op(_NS + "::pose_displacement", mutates_args=(), device_types="cuda")
def pose_displacement(pred: torch.Tensor, ref: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """pred (..., 7), ref (7,) fp32 -> (distance (...), rotation angle in radians (...)) of every pose from ref; exactly 0 for an equal row"""
    pos, ori = _ops().pose_displacement(pred, ref)
    return pos, ori


@pose_displacement.register_fake
def _(pred, ref):
    return pred.new_empty(pred.shape[:-1]), pred.new_empty(pred.shape[:-1])


@torch.library.custom_op(_NS + "::saliency_map", mutates_args=(), device_types="cuda")
def saliency_map(scores: torch.Tensor, desc: List[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """scores (M, K) or (M, Gy, Gx) fp32 -> (maps (M, Hs, Ws), minmax (M, 2)): per pixel the mean score of the covering rectangles"""
    maps, minmax = _ops().saliency_map(scores, _occlusion_desc("saliency_map", desc))
    return maps, minmax


@saliency_map.register_fake
def _(scores, desc):
    return scores.new_empty((scores.shape[0], desc[0], desc[1])), scores.new_empty((scores.shape[0], 2))


@torch.library.custom_op(_NS + "::saliency_overlay_u8", mutates_args=(), device_types="cuda")
def saliency_overlay_u8(frame: torch.Tensor, smap: torch.Tensor, minmax: torch.Tensor, table: torch.Tensor, alpha_q8: int, fade: bool) -> torch.Tensor:
    """frame uint8 (Hs, Ws, 3), smap fp32 (Hs, Ws), minmax fp32 (2,), table uint8 (256, 3) -> the map drawn over the frame, uint8 (Hs, Ws, 3)"""
    return _ops().saliency_overlay_u8(frame, smap, minmax, table, alpha_q8, fade)


@saliency_overlay_u8.register_fake
def _(frame, smap, minmax, table, alpha_q8, fade):
    return torch.empty_like(frame)


# ---- pose overlay --------------------------------------------------------------------------------------------------------------
@torch.library.custom_op(_NS + "::project_poses", mutates_args=(), device_types="cuda")
def project_poses(poses: torch.Tensor, cam: torch.Tensor, cam_index: torch.Tensor, axis_len: float, pos_err: Optional[torch.Tensor],
                  ori_err: Optional[torch.Tensor], pos_full: float, ori_full: float, width: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """poses fp32 (F, G, 7), cam fp64 (C, 3, 4), cam_index int32 (F,) -> (points int32 (F, G, 4, 2) in sixteenths of a pixel, bars int32 (F, 2))"""
    points, bars = _ops().project_poses(poses, cam, cam_index, axis_len, pos_err, ori_err, pos_full, ori_full, width)
    return points, bars


@project_poses.register_fake
def _(poses, cam, cam_index, axis_len, pos_err, ori_err, pos_full, ori_full, width):
    return poses.new_empty((poses.shape[0], poses.shape[1], 4, 2), dtype=torch.int32), poses.new_empty((poses.shape[0], 2), dtype=torch.int32)


@torch.library.custom_op(_NS + "::draw_poses_u8", mutates_args=(), device_types="cuda")
def draw_poses_u8(frames: torch.Tensor, points: torch.Tensor, bars: torch.Tensor, styles: List[int], frames_per_episode: int, first: int, bar_px: int,
                  bar_colours: List[int], flip: bool) -> torch.Tensor:
    """frames uint8 (n, Hs, Ws, 3) annotated with entries first .. first + n - 1 of the draw list; styles: per pose set the integers of
    rpe_overlay_style in the order of ops.OVERLAY_STYLE_FIELDS, one set after the other; bar_colours: six bytes"""
    ops = _ops()
    k = len(ops.OVERLAY_STYLE_FIELDS)
    if not styles or len(styles) % k or len(bar_colours) != 6:
        raise ValueError("draw_poses_u8: styles has %d integers per pose set (%s), bar_colours six" % (k, ", ".join(ops.OVERLAY_STYLE_FIELDS)))
    sets = [ops.overlay_style_from_list(styles[i:i + k]) for i in range(0, len(styles), k)]
    return ops.draw_poses_u8(frames, points, bars, sets, frames_per_episode=frames_per_episode, first=first, bar_px=bar_px,
                             bar_colours=(bar_colours[:3], bar_colours[3:]), flip=flip)


@draw_poses_u8.register_fake
def _(frames, points, bars, styles, frames_per_episode, first, bar_px, bar_colours, flip):
    return torch.empty_like(frames)
