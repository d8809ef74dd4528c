/*
 * rpe_hip.h -- C ABI of librpe_hip.so: the MI355X (gfx950) implementation of the
 * RGB + proprioception pose-regression TRAIN STEP of
 * cremebrule/rgb-proprioceptive-pose-estimator.
 *
 * The reference has no FFI / plugin layer: the path sits behind Python classes
 * (models/naive.py, models/time_sensitive.py, models/losses.py, util/learn_utils.py).
 * Every entry point below therefore replaces the torch op(s) a reference line
 * dispatches; the citation after "replaces:" is the reference file:line.  The Python
 * host side (rgb-proprioceptive-pose-estimator_amd/) binds these with ctypes and
 * keeps the reference's class / constructor / state_dict surface.
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer unless its name ends in _host.  Buffers are
 *    borrowed: nothing is freed or retained past the call except by the engine
 *    object, which retains exactly what rpe_resnet50_bind() hands it.
 *  - `stream` is a hipStream_t passed as void*.  Calls only enqueue work; no entry
 *    point synchronises, allocates or frees device memory (hipGraph-capturable).
 *  - Activations of the conv trunk are NHWC ([B][H][W][C], C contiguous) in the
 *    compute dtype (RPE_F32, RPE_BF16 or RPE_F16; accumulation is always fp32).  Head tensors
 *    (features, MLP / LSTM, loss) are fp32 with a leading dimension `ld`.
 *  - Operands must be 16-byte aligned and channel counts / leading dimensions
 *    multiples of the 16-byte chunk (4 fp32 / 8 bf16) unless stated otherwise.
 *  - Return value: 0 on success, an RPE_ERR_* code otherwise; rpe_last_error()
 *    returns a thread-local message.  No exceptions cross the boundary.
 */
#ifndef RPE_HIP_H
#define RPE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define RPE_ABI_VERSION 3   /* 2: BN partial-sum row counts depend on the element type (halo form of the 3x3 convs); 3: the staged image x4 is zero-bordered */

enum { RPE_F32 = 0, RPE_BF16 = 1, RPE_F16 = 2 };   /* RPE_F16: IEEE half activations / weight copies (BASELINE config C5), fp32 accumulate */
enum {
    RPE_OK = 0,
    RPE_ERR_SHAPE = 1,     /* bad dimension / unsupported configuration */
    RPE_ERR_DTYPE = 2,
    RPE_ERR_ALIGN = 3,
    RPE_ERR_HIP = 4,       /* a HIP runtime call failed */
    RPE_ERR_WORKSPACE = 5, /* caller-provided workspace too small */
    RPE_ERR_STATE = 6      /* engine used before bind / forward */
};

int rpe_abi_version(void);
/* the first 16 hex digits of the SHA-256 of the sources this library was built from (fixed at build time; csrc/Makefile): ties
 * measurements kept beside the repository (profiles/hbm_traffic_pmc.json, "build_id") to the library a process actually loaded */
const char* rpe_build_id(void);
const char* rpe_last_error(void);

/* ------------------------------------------------------------------ convolution */
/* replaces: nn.Conv2d(bias=False) forward/backward inside torchvision resnet50
 * (constructed at util/model_utils.py:136, called at models/naive.py:84,316 and
 * models/time_sensitive.py:185,472,733). */
typedef struct {
    int batch, in_h, in_w, in_c; /* NHWC input */
    int out_c, kh, kw;
    int stride, pad;             /* stride 1 or 2 */
} rpe_conv_desc;

int rpe_conv_out_hw(const rpe_conv_desc* d, int* ho, int* wo);
/* number of 128-row tiles = rows of the BN partial-sum buffer [tiles][2][out_c] of the 1x1 / stem / strided launches */
long rpe_conv_stats_tiles(long rows);
/* rows of stats_part [tiles][2][out_c] rpe_conv2d_fwd writes for this conv and element type: 128-row tiles, except the 3x3 / stride 1 /
 * pad 1 convs of the 16-bit types, whose tiles are whole output rows (the halo form) */
long rpe_conv2d_fwd_stats_tiles(const rpe_conv_desc* d, int dtype);

/* y[B][Ho][Wo][out_c] = conv(x, w);  w_krsc = [out_c][kh][kw][in_c].
 * stats_part (nullable): per-128-row-tile column sums and sums of squares of the fp32
 * accumulators, consumed by rpe_bn_finalize. */
int rpe_conv2d_fwd(const rpe_conv_desc* d, int dtype, const void* x, const void* w_krsc, void* y, float* stats_part, void* stream);
/* inference form: out = [relu](conv(x, w) + bias[out_c] (+ addend[rows][out_c])) in one launch.  With w = weight * BN scale
 * (rpe_pack_desc.scale) and bias = BN shift this is conv -> BatchNorm2d(eval) -> (+identity) -> ReLU of torchvision's
 * Bottleneck (called at models/naive.py:316 in eval mode / rollout). */
int rpe_conv2d_fwd_affine(const rpe_conv_desc* d, int dtype, const void* x, const void* w_krsc, void* out, const float* bias, const void* addend,
                          int relu, void* stream);
/* The same with a caller-provided workspace: launches with few output tiles and a long reduction (one rollout frame through
 * layer2-4: 4..26 tiles of 64 x 64 walking K = 1152..4608 alone) are split along K over 4..32 workgroups per tile; the
 * partial fp32 tiles go through the workspace and are added in a fixed order by a second small launch.  The query returns 0
 * for shapes that are not split (the call then equals rpe_conv2d_fwd_affine); workspace 16-byte aligned, no state kept in it. */
long rpe_conv2d_fwd_affine_workspace_bytes(const rpe_conv_desc* d, int dtype);
int rpe_conv2d_fwd_affine_ws(const rpe_conv_desc* d, int dtype, const void* x, const void* w_krsc, void* out, const float* bias, const void* addend,
                             int relu, void* workspace, long workspace_bytes, void* stream);
/* dx[B][H][W][in_c] = conv_transpose(dy, w) (+ addend);  w_crsk = [in_c][kh][kw][out_c]. */
int rpe_conv2d_dgrad(const rpe_conv_desc* d, int dtype, const void* dy, const void* w_crsk, void* dx, const void* addend, void* stream);
/* Data gradient with the BatchNorm-backward reduction of the PRODUCING layer fused into the epilogue:
 * dz[B][H][W][in_c] = (conv_transpose(dy, w) + addend) * [ReLU mask of that layer's output], and per-128-row-tile partial
 * sums (sum dz, sum dz*xhat) -> bn->stats_part [tiles][2][in_c], consumed by rpe_bn_backward_from_dz.
 * mask: a_mask != NULL: its bits;  else a_out != NULL: a_out > 0;  else scale/shift != NULL: y*scale+shift > 0 (BN+ReLU
 * without residual);  else none.
 * Rows of stats_part (rpe_conv2d_dgrad_stats_tiles of them, every one written in every column, nothing behind them), by form:
 *   plain tiles (1x1 / stride 1 and every shape not named below): row t = the rows [128 t, 128 t + 128) of dz [B H W][in_c];
 *   class-major (stride 2, even in_h and in_w): row cls * ceil(rows_q / 128) + t, cls = 2 (h & 1) + (w & 1), rows_q = B (H/2) (W/2):
 *     the t-th 128 pixels of that parity class's own list (b, h', w');
 *   halo tiles (3x3 / stride 1 / pad 1, 16-bit types, out_c % 64 == 0): row t = the rt whole image rows [rt t, rt t + rt) of the
 *     B * in_h rows, rt * in_w <= 128 pixels.
 * Consumers may rely on the column totals over all rows only; which pixels a row covers is a contract for the 1x1 / stride-1 form alone. */
typedef struct {
    const void* y;       /* raw conv output the BN normalised, same shape as dz.  NULL together with a_mask (1x1 / stride-1 convs of a 16-bit
                          * type): that output does not exist -- only sum dz is emitted (the second half of every partial row is 0),
                          * sum dz*xhat then follows from the weight gradient's first product (rpe_bn_backward_coeffs_t) */
    const void* a_out;   /* BN(+residual)+ReLU output, or NULL */
    const float *mean, *invstd, *scale, *shift;
    float* stats_part;
    const unsigned char* a_mask; /* or: the packed ReLU mask rpe_bn_apply_mask wrote, [rows][in_c/8] bytes (bit j = channel 8k+j > 0) */
} rpe_bn_bwd_epilogue;
/* rows of bn->stats_part the fused data gradient writes (stride-2 layers enumerate rows per parity class; 3x3 / stride 1 in 16-bit types: halo tiles) */
long rpe_conv2d_dgrad_stats_tiles(const rpe_conv_desc* d, int dtype);
int rpe_conv2d_dgrad_bn(const rpe_conv_desc* d, int dtype, const void* dy, const void* w_crsk, void* dz, const void* addend,
                        const rpe_bn_bwd_epilogue* bn, void* stream);
/* Compact data gradient of a 1x1 / stride-2 / pad-0 conv with even in_h, in_w (a ResNet projection shortcut of layers 2-4; replaces the
 * conv-transpose of downsample[0] in torchvision's Bottleneck, util/model_utils.py:136): such a conv reads the pixels (b, 2h', 2w') alone, so
 *   dx_compact[B][in_h/2][in_w/2][in_c] = dy[B*Ho*Wo][out_c] * w_crsk^T      (one dense GEMM, no zero-filled full-resolution tensor)
 * holds every non-zero row of rpe_conv2d_dgrad's dx.  Other shapes: RPE_ERR_SHAPE.
 * The *_sub forms are rpe_conv2d_dgrad / rpe_conv2d_dgrad_bn / rpe_conv1x1_dgrad_kcat_y of a 1x1 / stride-1 conv with even in_h, in_w whose
 * addend is such a compact tensor [B][in_h/2][in_w/2][in_c]: pixel (b, h, w) adds compact pixel (b, h/2, w/2) when h and w are even and
 * +0 otherwise -- bitwise what the unchanged call returns for the same values scattered into a zero-filled full-resolution addend.
 * With a BN epilogue the ReLU mask comes from bn->a_mask or bn->a_out; the other mask forms take no compact addend (RPE_ERR_SHAPE). */
int rpe_conv1x1s2_dgrad_compact(const rpe_conv_desc* d, int dtype, const void* dy, const void* w_crsk, void* dx_compact, void* stream);
int rpe_conv2d_dgrad_sub(const rpe_conv_desc* d, int dtype, const void* dy, const void* w_crsk, void* dx, const void* addend_compact, void* stream);
int rpe_conv2d_dgrad_bn_sub(const rpe_conv_desc* d, int dtype, const void* dy, const void* w_crsk, void* dz, const void* addend_compact,
                            const rpe_bn_bwd_epilogue* bn, void* stream);
/* A bottleneck block WITHOUT its raw conv3 output (16-bit element types; replaces conv3 -> bn3 -> (+identity) -> ReLU of torchvision's
 * Bottleneck in training mode -- util/model_utils.py:136 builds it, models/naive.py:316 calls it -- and their backward).
 * BatchNorm statistics of a 1x1 conv follow from its INPUT: y = x W^T gives mean_c = w_c . colsum(x) / M, E[y_c^2] = w_c^T (x^T x) w_c / M.
 * rpe_gram: x [M][C] -> out fp32 [rpe_gram_ones_row(C) + 1][C]: x^T x in rows [0, C), colsum(x) in row rpe_gram_ones_row(C) (one
 * weight-gradient-style launch, fixed-order slab sum).  rpe_bn_stats_from_gram: what rpe_bn_finalize produces (scale, shift, saved
 * mean / invstd, running statistics), from the Gram matrix and the compute-dtype weight.  rpe_conv1x1_fwd_bn: the conv with
 * out = relu(acc * scale + shift + residual [* res_scale + res_shift]) and the packed ReLU mask in its epilogue -- the raw output
 * is written only when y_out is given.  Without y_out, with a residual and a mask, in_c 64 / 128, out_c a multiple of 256 and >= 512 rows
 * (the y3-free blocks of layers 1-2) the launch is the row-streaming kernel of csrc/stream1x1.hip (weights resident in registers, a per-wave
 * LDS-DMA ring), bitwise the tiled form; RPE_NO_STREAM1X1=1 keeps the tiled form. */
/* rpe_bn_apply_gram: out = relu(y * scale + shift) (bn2's apply pass) AND the Gram buffer of `out` -- same layout and values as rpe_gram(out)
 * -- in one pass over y (C = 64 or 128, 16-bit element types; workspace = per-workgroup fp32 partials, summed in a fixed order). */
long rpe_bn_apply_gram_workspace_bytes(int dtype, long rows, int C);
int rpe_bn_apply_gram(int dtype, const void* y, void* out, const float* scale, const float* shift, long rows, int C, float* gram_out,
                      void* workspace, long workspace_bytes, void* stream);
long rpe_gram_ones_row(int C);
long rpe_gram_workspace_bytes(int dtype, long M, int C);
int rpe_gram(int dtype, const void* x, long M, int C, float* out, void* workspace, long workspace_bytes, void* stream);
int rpe_bn_stats_from_gram(int dtype, const void* w, int Co, int Ci, const float* gram, int ones_row, long count, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, long long* num_batches, float momentum, float eps, float* scale, float* shift,
                           float* save_mean, float* save_invstd, void* stream);
int rpe_conv1x1_fwd_bn(const rpe_conv_desc* d, int dtype, const void* x, const void* w, void* out, void* y_out, const float* scale, const float* shift,
                       const void* residual, const float* res_scale, const float* res_shift, unsigned char* relu_mask, void* stream);
/* BatchNorm backward folded into the data gradient of the 1x1 / stride-1 conv in front of it (y = a_in W^T, z = BN(y)):
 *   dx = dz (A o W) + a_in G + 1 b^T   with A = gamma invstd, G = W^T diag(C') W, b = W^T B'  (C', B' from the BN coefficients),
 * so the data gradient reads dz and the conv's INPUT instead of a materialised dy = BN'(dz, y).
 * rpe_bn_bwd_fold_conv1x1 builds w_kcat [in_c][out_c + in_c] (compute dtype) and bias [in_c] from the packed weights
 * (w_fwd [out_c][in_c], w_dgrad [in_c][out_c]) and c1c2 (rpe_bn_backward_coeffs); rpe_conv1x1_dgrad_kcat is the GEMM
 * (A operand = [dz | a_in], optional fused BN-backward epilogue of the layer BEHIND, as rpe_conv2d_dgrad_bn).
 * replaces: autograd's BatchNorm2d backward + conv3 data gradient of a torchvision Bottleneck (util/model_utils.py:136). */
long rpe_bn_bwd_fold_scratch_bytes(int dtype, int out_c, int in_c);
int rpe_bn_bwd_fold_conv1x1(int dtype, int out_c, int in_c, const void* w_fwd, const void* w_dgrad, const float* gamma, const float* invstd,
                            const float* mean, const float* c1c2, void* w_kcat, float* bias, void* scratch, long scratch_bytes, void* stream);
int rpe_conv1x1_dgrad_kcat(const rpe_conv_desc* d, int dtype, const void* dz, const void* a_in, const void* w_kcat, const float* bias, void* dx,
                           const rpe_bn_bwd_epilogue* bn, void* stream);
/* The same fold for the conv in FRONT of a narrow BatchNorm -- a Bottleneck's conv1 (x [M][in_c] -> y [M][out_c], z = bn1(y)):
 *   dx = [dz | y] [A o W ; C' o W] + 1 b^T   (y is the second K-concatenated operand itself: K = 2 out_c, no Gram matrix),
 *   dW[k][n] = A_k ((dz^T x)[k][n] - c1_k s1[n]) + C'_k ((y^T x)[k][n] - mean_k s1[n]),  s1 = colsum(x)   (one row-concatenated launch),
 * so neither gradient reads a materialised dy and bn1's streaming dz, y -> dy pass is gone (replaces the BatchNorm2d backward + conv1
 * backward of a torchvision Bottleneck as torch autograd runs them: util/model_utils.py:136, models/naive.py:316).
 * rpe_bn_bwd_fold_y_conv1x1: w_kcat [in_c][2 out_c] (compute dtype), bias [in_c] from the data-gradient copy of the weight [in_c][out_c]
 * and the BN coefficients (rpe_bn_backward_coeffs); rpe_conv1x1_dgrad_kcat_y: the data gradient (+ bias, + addend, + the fused BN-backward
 * epilogue of the layer behind, as rpe_conv2d_dgrad_bn); rpe_conv1x1_wgrad_folded_y: the weight gradient into dw [out_c][in_c] fp32. */
int rpe_bn_bwd_fold_y_conv1x1(int dtype, int out_c, int in_c, const void* w_dgrad, const float* gamma, const float* invstd, const float* mean,
                              const float* c1c2, void* w_kcat, float* bias, void* stream);
int rpe_conv1x1_dgrad_kcat_y(const rpe_conv_desc* d, int dtype, const void* dz, const void* y, const void* w_kcat, const float* bias, void* dx,
                             const void* addend, const rpe_bn_bwd_epilogue* bn, void* stream);
/* (addend = a compact shortcut gradient: see rpe_conv1x1s2_dgrad_compact) */
int rpe_conv1x1_dgrad_kcat_y_sub(const rpe_conv_desc* d, int dtype, const void* dz, const void* y, const void* w_kcat, const float* bias, void* dx,
                                 const void* addend_compact, const rpe_bn_bwd_epilogue* bn, void* stream);
long rpe_conv1x1_wgrad_folded_y_scratch_bytes(const rpe_conv_desc* d, int dtype);
int rpe_conv1x1_wgrad_folded_y(const rpe_conv_desc* d, int dtype, const void* dz, const void* y, const void* x, const float* gamma, const float* invstd,
                               const float* mean, const float* c1c2, float* dw, void* scratch, long scratch_bytes, void* stream);
/* The weight-gradient side of the same fold: dw[out_c][in_c] (fp32, OVERWRITTEN) = A o (dz^T a_in) + B' colsum(a_in)^T + C' o (W S),
 * S = a_in^T a_in -- reads dz and a_in only, no dy.  w_master: the fp32 weight [out_c][in_c].  Deterministic (slab sums). */
long rpe_conv1x1_wgrad_folded_scratch_bytes(const rpe_conv_desc* d, int dtype);
int rpe_conv1x1_wgrad_folded(const rpe_conv_desc* d, int dtype, const void* dz, const void* a_in, const float* w_master, const float* gamma,
                             const float* invstd, const float* mean, const float* c1c2, float* dw, void* scratch, long scratch_bytes, void* stream);
/* Backward of a block whose raw conv3 output was never written (rpe_conv1x1_fwd_bn with y_out = NULL).  The fused data gradient that
 * produces dz (rpe_conv2d_dgrad_bn with bn->y = NULL, bn->a_mask set) emits sum dz only; the weight gradient's first product
 * T = dz^T a_in ([out_c][in_c] fp32 = rpe_conv2d_wgrad_det(x = a_in, dy = dz)) then gives sum dz*y = rowdot(T_c, W_c):
 * rpe_bn_backward_coeffs_t = rpe_bn_backward_coeffs with that second sum (w: the compute-dtype weight [C][Ci] the forward used), and
 * rpe_conv1x1_wgrad_combine = the last step of rpe_conv1x1_wgrad_folded from T and the FORWARD's Gram buffer (rpe_gram of a_in):
 * dw = A o (T - c1 s1^T) + C' o (W S - mean s1^T).  Replaces autograd's BatchNorm2d + conv3 backward of a torchvision Bottleneck. */
/* rpe_conv1x1_dgrad_bn_t: the fused data gradient of the NEXT block's conv1 (rpe_conv2d_dgrad_bn with bn->y = NULL: dz of the producing
 * block, its ReLU mask applied, sum dz per tile) that ALSO leaves T = dz^T a_prev ([in_c][P] fp32, a_prev [rows][P] = the producing
 * block's conv3 input, P = 64 or 128) behind -- from the dz tile on its way out, so the separate dz^T a launch and its re-read of dz
 * are gone.  Persistent launch (per-workgroup partials in `workspace`, summed in workgroup order: deterministic). */
long rpe_conv1x1_dgrad_bn_t_workspace_bytes(const rpe_conv_desc* d, int P);
int rpe_conv1x1_dgrad_bn_t(const rpe_conv_desc* d, int dtype, const void* dy, const void* w_crsk, void* dz, const void* addend, const rpe_bn_bwd_epilogue* bn,
                           const void* a_prev, int P, float* t_out, void* workspace, long workspace_bytes, void* stream);
int rpe_bn_backward_coeffs_t(int dtype, const float* stats_part, int tiles, int C, long rows, const float* dzt_a, const void* w, int Ci, const float* mean,
                             const float* invstd, float* dgamma, float* dbeta, float* c1c2, double* dpart, void* stream);
int rpe_conv1x1_wgrad_combine(const rpe_conv_desc* d, const float* dzt_a, const float* gram, const float* w_master, const float* gamma, const float* invstd,
                              const float* mean, const float* c1c2, float* dw, void* stream);
/* the two halves of rpe_bn_backward_from_dz as separate calls (c1c2: [2][C] fp32 = mean(dz), mean(dz xhat)) */
int rpe_bn_backward_coeffs(const float* stats_part, int tiles, int C, long rows, float* dgamma, float* dbeta, float* c1c2, double* dpart, void* stream);
int rpe_bn_backward_apply_dz(int dtype, const void* dz, const void* y, const float* mean, const float* invstd, const float* gamma, const float* c1c2,
                             void* dy, long rows, int C, void* stream);
/* dw_krsc[out_c][kh][kw][in_c] (fp32) += x (*) dy.  Atomic accumulation: zero it first. */
int rpe_conv2d_wgrad(const rpe_conv_desc* d, int dtype, const void* x, const void* dy, float* dw_krsc, void* stream);
/* Deterministic form: dw_krsc = x (*) dy (OVERWRITTEN, no zeroing needed).  Every workgroup stores its fp32 tile into
 * `workspace` (>= rpe_conv2d_wgrad_workspace_bytes(), 16-byte aligned, caller-owned, free again when the call's work has run)
 * and a second launch sums the tiles in a fixed order: bitwise reproducible, no float atomics. */
long rpe_conv2d_wgrad_workspace_bytes(const rpe_conv_desc* d, int dtype);
int rpe_conv2d_wgrad_det(const rpe_conv_desc* d, int dtype, const void* x, const void* dy, float* dw_krsc, void* workspace, long workspace_bytes,
                         void* stream);

/* ResNet stem conv1 (3->64, 7x7 / 2, pad 3) on the staged image x4; w_packed = [64][8][8][4] from rpe_pack_stem_weight.
 * x4 is ZERO-BORDERED NHWC4: [B][H + 2 RPE_STEM_PAD][W + 2 RPE_STEM_PAD][4] in the compute dtype, the image at rows / columns
 * [RPE_STEM_PAD, RPE_STEM_PAD + H) x [.., + W), channel 3 = 0, and ZEROS around it (conv1's padding made explicit: every 16-byte
 * piece of an im2col row is then an in-bounds aligned read, so the conv and its weight gradient stage through LDS-DMA -- round 4; the
 * unpadded layout of rounds 1-3 forced register staging at 1.8-2.1 TB/s).  rpe_stage_image_nhwc4 / rpe_stage_frames_u8[_resized] write
 * the interior only: zero the buffer once before its first use (rpe_x4_bytes() bytes).  H, W even. */
#define RPE_STEM_PAD 3
long rpe_x4_bytes(int dtype, int B, int H, int W);
int rpe_stem_conv_fwd(int dtype, const void* x4, const void* w_packed, void* y, float* stats_part, int B, int H, int W, void* stream);
int rpe_stem_conv_fwd_affine(int dtype, const void* x4, const void* w_packed, void* out, const float* bias, int relu, int B, int H, int W,
                             void* stream);
/* dw_packed [64][8][8][4] fp32 += x4 (*) dy.  Atomic accumulation INTO what dw_packed holds: zero it first for the plain gradient.
 * Channel 3 of every tap receives exactly 0 (x4's channel 3 is zero); tap row 7 / column 7 are not gradients (they meet the image
 * shifted by one row / column) and rpe_unpack_stem_grad skips them. */
int rpe_stem_conv_wgrad(int dtype, const void* x4, const void* dy, float* dw_packed, int B, int H, int W, void* stream);
/* deterministic form (see rpe_conv2d_wgrad_det): dw_packed is overwritten */
long rpe_stem_conv_wgrad_workspace_bytes(int dtype, int B, int H, int W);
int rpe_stem_conv_wgrad_det(int dtype, const void* x4, const void* dy, float* dw_packed, int B, int H, int W, void* workspace, long workspace_bytes,
                            void* stream);

/* weight layouts.  w_krsc_f32 is the fp32 master in channels_last storage. */
int rpe_pack_conv_weight(int dtype, const float* w_krsc, void* w_fwd, void* w_dgrad, int Co, int R, int S, int Ci, void* stream);
/* the same for many layers in one launch; the descriptor table lives in device memory */
typedef struct {
    const float* src; /* [Co][RS][Ci] fp32 */
    void* wf;         /* forward copy or NULL */
    void* wd;         /* dgrad copy [Ci][RS][Co] or NULL */
    int Co, RS, Ci;
    int pad_;
    long start;       /* first flat element index of this layer */
    const float* scale; /* NULL, or [Co]: the forward copy is written as w * scale[co] (inference: BatchNorm folded into the conv) */
} rpe_pack_desc;
int rpe_pack_conv_weights_multi(int dtype, const rpe_pack_desc* table_dev, int nlayers, long total, void* stream);
/* scale: NULL or [64] (see rpe_pack_desc.scale) */
int rpe_pack_stem_weight(int dtype, const float* w_oihw, const float* scale, void* out, void* stream);
int rpe_unpack_stem_grad(const float* d_packed, float* dw_oihw, void* stream);

/* replaces: the per-tensor .cuda() staging of util/learn_utils.py:130-138 for `img`
 * ((B,3,H,W) fp32 NCHW, util/data_utils.py:62-73) -> the interior of the zero-bordered NHWC4 image x4 (see rpe_stem_conv_fwd). */
int rpe_stage_image_nhwc4(int dtype, const float* img_nchw, void* out, int B, int H, int W, void* stream);

/* replaces: the CPU image transform ToPILImage -> Resize(256) -> CenterCrop(224) -> ToTensor -> Normalize
 * (util/data_utils.py:48-54) for frames whose shorter side already equals the resize target: uint8 [B][Hs][Ws][3] frames are
 * centre-cropped to (H, W), normalised with the HOST arrays mean3/std3 and written as NHWC4 in the compute dtype.
 * The crop starts at row (Hs - H) / 2, column (Ws - W) / 2 in integer division: an odd difference is FLOORED.  torchvision's CenterCrop
 * rounds half to even there, so callers send odd differences to rpe_stage_frames_u8_resized with their own (top, left) instead
 * (engine.py, ops.stage_frames); with both passes off that call is a pure window. */
int rpe_stage_frames_u8(int dtype, const unsigned char* frames, void* out, int B, int Hs, int Ws, int H, int W, const float* mean3_host,
                        const float* std3_host, void* stream);
/* The same for frames whose shorter side is not the transform's resize target: Pillow's antialiased 8-bit bilinear resample
 * (Resize(256) on a PIL image, util/data_utils.py:48-54) to Hr x Wr in its own 22-bit fixed-point arithmetic, then the crop of
 * H x W at (top, left) and the normalisation.  xb/yb: [Wr]/[Hr] x (first tap, tap count); xk/yk: [Wr][ksx] / [Hr][ksy] int32 weights
 * (device pointers; a pass whose size does not change takes nulls); tmp: B*Hs*Wr*3 bytes of device scratch. */
int rpe_stage_frames_u8_resized(int dtype, const unsigned char* frames, void* out, int B, int Hs, int Ws, int Hr, int Wr, int top, int left, int H, int W,
                                const int* xb, const int* xk, int ksx, const int* yb, const int* yk, int ksy, unsigned char* tmp, const float* mean3_host,
                                const float* std3_host, void* stream);

/* replaces: the CPU depth transform ToPILImage -> Resize(256) -> CenterCrop(224) -> ToTensor (util/data_utils.py:55-60) for raw
 * fp32 depth frames [B][Hs][Ws]: Pillow's 32-bit-float bilinear resample (mode F: double accumulation over ascending taps, the
 * horizontal pass rounded to fp32 before the vertical one) to Hr x Wr, of which out [B][H][W] fp32 receives the window
 * [top, top + H) x [left, left + W) -- bit for bit what Pillow writes; ToTensor does not rescale a float image.  xb/yb as in
 * rpe_stage_frames_u8_resized; xk/yk: [Wr][ksx] / [Hr][ksy] DOUBLE weights (device pointers; a pass whose size does not change
 * takes nulls, with both null this is a crop copy).  One launch, no scratch. */
int rpe_stage_depth_f32_resized(const float* frames, float* out, int B, int Hs, int Ws, int Hr, int Wr, int top, int left, int H, int W,
                                const int* xb, const double* xk, int ksx, const int* yb, const double* yk, int ksy, void* stream);

/* Label-preserving augmentation of raw camera frames (no counterpart in the reference, whose transform is deterministic): photometric
 * jitter, sensor noise and random erasing on uint8 [B][Hs][Ws][3] frames, uint8 out, in front of rpe_stage_frames_u8[_resized].  All
 * arithmetic is integer and specified to the bit ("Frame augmentation"); random numbers are Philox4x32-10 keyed by
 * `seed` with the counter (a, b, step, purpose), bounded draws are (r * n) >> 32. */
typedef struct {
    unsigned long long seed;
    int qb_lo, qb_hi, qc_lo, qc_hi, qs_lo, qs_hi; /* brightness / contrast / saturation factor ranges in Q16: 65536 = identity, 0 <= lo <= hi <= 4 * 65536 */
    int noise_q;                                  /* Q16 multiplier on the centred sum of four random bytes, 0 = off, at most 4 * 65536 */
    unsigned erase_thresh;                        /* a stream erases iff its word r < erase_thresh (probability * 2^32, capped at 2^32 - 1); 0 = off */
    int eh_lo, eh_hi, ew_lo, ew_hi;               /* rectangle height / width bounds in pixels, 1 <= lo <= hi <= Hs / Ws */
    int fill_mode;                                /* 0: fill_rgb, 1: random bytes */
    unsigned char fill_rgb[3];
    int group;                                    /* 0: frame b draws its parameters from stream b; N > 0: from stream b % N */
} rpe_augment_desc;
/* in / out: device, [B][Hs][Ws][3], the same buffer or disjoint ones; Hs * Ws < 2^32.  state: device, state[0] is the step counter --
 * the launch reads it and advances it by one, so a captured call draws fresh numbers at every replay.  params: device, 1 + 8 G ints
 * (G = B, or `group`), receives [0] = the step used, then per stream qb, qc, qs, erase, top, left, h, w.  sums: device, B entries,
 * receives each frame's sum of grey values after the brightness stage (untouched when the contrast range is {65536}). */
int rpe_augment_frames_u8(const unsigned char* in, unsigned char* out, int B, int Hs, int Ws, const rpe_augment_desc* d, unsigned* state, int* params,
                          unsigned long long* sums, void* stream);

/* Blur of raw camera frames (no counterpart in the reference): defocus (Gaussian) and linear motion blur on uint8 [B][Hs][Ws][3]
 * frames, uint8 out, run IN FRONT of rpe_augment_frames_u8 -- optics first, then photometry, noise and the occluder.  All arithmetic
 * is integer and specified to the bit ("Frame blur"); coordinates are clamped to the frame (replicate border).
 *   Gaussian, level s: radius R = radius[s] <= 8, half-kernel w = taps[s][0..R] >= 0 with w[0] + 2 (w[1] + .. + w[R]) = 2048;
 *     h(x, y) = sum_{k=-R..R} w[|k|] v(x + k, y);  out(x, y) = (sum_{k=-R..R} w[|k|] h(x, y + k) + 2^21) >> 22
 *   motion, odd length L = 3 .. 15, direction d: for t = -(L-1)/2 .. (L-1)/2, dx = (t dir_cx[d] + 128) >> 8, dy = (t dir_cy[d] + 128) >> 8
 *     (floor shifts);  out = (2 sum_t v(x + dx, y + dy) + L) / (2 L)
 * Each stream g (frame b, or b % group) draws r0..r3 = Philox4x32-10(key = seed, counter (g, 0, step, 0x424C5552 "BLUR")):
 *   kind = r0 < gauss_thresh ? 1 : ((u64)r0 < (u64)gauss_thresh + motion_thresh ? 2 : 0)   (0: the frame is copied)
 *   level = (r1 n_levels) >> 32,  L = 3 + 2 ((r2 n_lengths) >> 32),  d = (r3 n_dirs) >> 32 */
typedef struct {
    unsigned long long seed;
    unsigned gauss_thresh, motion_thresh;         /* a stream is blurred iff its word r0 is below ...; the sum is at most 2^32 - 1 */
    int n_levels;                                 /* 1 .. 8 */
    int radius[8];                                /* 0 .. 8 per level */
    int taps[8][9];                               /* taps[s][k], k <= radius[s]; entries beyond the radius are ignored */
    int n_lengths;                                /* 1 .. 7: L in {3, 5, .., 1 + 2 n_lengths} */
    int n_dirs;                                   /* 1 .. 16 */
    int dir_cx[16], dir_cy[16];                   /* Q8 direction components, each within +-256 */
    int group;                                    /* 0: frame b draws from stream b; N > 0: from stream b % N */
} rpe_blur_desc;
/* in / out: device, [B][Hs][Ws][3], DISJOINT (a stencil cannot run in place); Hs * Ws < 2^32.  state: device, state[0] is the step
 * counter -- the launch READS it and never advances it: the rpe_augment_frames_u8 call that follows does, so both tables of one
 * step carry the same [0] and a captured pair draws fresh numbers at every replay.  params: device, 1 + 4 G ints (G = B, or `group`),
 * receives [0] = the step used, then per stream kind, level, L, d.  Refused with RPE_ERR_SHAPE before any launch: a null pointer,
 * non-positive sizes, Hs * Ws >= 2^32, n_levels outside 1..8, a radius outside 0..8, a negative tap or a level whose taps do not sum
 * to 2048, n_lengths outside 1..7, n_dirs outside 1..16, a direction component beyond +-256, thresholds whose sum exceeds 2^32 - 1,
 * group < 0, in and out overlapping.  4-byte loads and stores where both pointers and the pixel rows (Ws % 4 == 0) are 4-byte
 * aligned, bytes otherwise.  Two launches. */
int rpe_blur_frames_u8(const unsigned char* in, unsigned char* out, int B, int Hs, int Ws, const rpe_blur_desc* d, const unsigned* state, int* params,
                       void* stream);

/* Shuffled minibatches from recorded episodes resident in device memory (no counterpart in the reference, whose DataLoader walks the
 * episodes in lockstep, unshuffled): an index launch and a row gather in front of rpe_augment_frames_u8 / rpe_stage_frames_u8[_resized].
 * All arithmetic is unsigned / 64-bit integer and specified to the bit ("Minibatch sampling").
 * Windows: K = (T - S) / stride + 1 start positions per episode, M = E K windows over the E selected episodes; window w is episode
 * sel[w / K], first timestep (w % K) * stride.  Draw i of step `step` has the global index g = step N + i (64 bits), epoch = g / M,
 * pos = g % M; shuffle 0: w = pos; shuffle 1: w = the epoch's keyed bijection of [0, M) at pos (4-round balanced Feistel network on
 * Philox4x32-10 keyed by `seed`, counter (R, round, epoch mod 2^32, 0x53414D50), cycle-walked), so M consecutive draws from a multiple
 * of M visit every window once. */
typedef struct {
    unsigned long long seed;
    int E, T, S, stride, N; /* selected episodes, timesteps per episode, timesteps per window, distance of window starts, windows per step */
    int shuffle;            /* 0: file order, 1: a fresh keyed permutation per epoch */
} rpe_sample_desc;
/* sel: device, E episode numbers in the file.  state: device, state[0] is the step counter -- the launch reads it and advances it by
 * one, so a captured call draws the next batch at every replay.  index: device, 1 + 2 N ints, receives [0] = the step used, then per
 * window (episode number in the file, first timestep).  E K must stay below 2^31.  One launch of one workgroup. */
int rpe_sample_windows(const rpe_sample_desc* d, const int* sel, unsigned* state, int* index, void* stream);
/* Episodes of unequal length: the same draw when episode e of the selection has only len_e = clamp(lengths[sel[e]], 0, T) of its T
 * rows (the rest is padding).  lengths: device, one entry per episode IN THE FILE, read as lengths[sel[e]] at every launch -- like sel,
 * so a captured call follows a refresh.  K_e = len_e >= S ? (len_e - S) / stride + 1 : 0, P_0 = 0, P_{e+1} = P_e + K_e, M = P_E: the
 * window table is scanned on the device (LDS), M and the half width of the Feistel domain, (max(bitlen(M - 1), 2) + 1) / 2, belong to
 * the launch.  g, epoch, pos, the bijection, its key, purpose word and cycle walk are rpe_sample_windows'; window w lies in episode e =
 * the largest index with P_e <= w (binary search) and starts at (w - P_e) stride, so t0 + S <= len_e: index[1 + 2 i] = sel[e],
 * index[2 + 2 i] = (w - P_e) stride.  index[0] and the counter as above.  With all lengths equal the table is rpe_sample_windows' bit
 * for bit.  M == 0 (no episode holds a window): every window is (sel[0], 0), in bounds for the gather and meaningless.
 * E <= 8192 (RPE_ERR_SHAPE beyond: the prefix table is 32 KB of LDS); E ((T - S) / stride + 1) must stay below 2^31.  One launch of
 * one workgroup. */
int rpe_sample_windows_ragged(const rpe_sample_desc* d, const int* sel, const int* lengths, unsigned* state, int* index, void* stream);
/* out row s N + n <- pool row index.episode[n] * T + index.t0[n] + s for s < S, n < N; rows of row_bytes bytes, 64-bit offsets.  pool:
 * device, [episodes in the file][T] rows; out: device, [S][N] rows, not overlapping the pool; index: as rpe_sample_windows writes it
 * (the entries are trusted: episode < episodes in the file, t0 + S <= T).  16-byte loads and stores when row_bytes and both pointers
 * are multiples of 16, 4-byte when multiples of 4, single bytes otherwise.  One launch. */
int rpe_gather_rows(const void* pool, void* out, long row_bytes, long T, const int* index, int S, int N, void* stream);

/* replaces: the measurement noise the reference draws on the host per refresh, x0bar = x0 + N(0, variance I) with the quaternion
 * renormalised (util/data_utils.py:162-167), drawn on the device at every launch instead ("Measurement noise").  Philox4x32-10
 * keyed by `seed`.  Lane n draws ONE scale for its whole window: index 0 when num_scales == 1, else k = (r0 num_scales) >> 32 with r0 =
 * word 0 at counter (n, 0, step, 0x4D45414B).  Row r = s N + n, component c: words (r0, r1) at counter (r, c, step, 0x4D454153), in
 * fp64 u1 = (r0 + 0.5) 2^-32, u2 = r1 2^-32, z = sqrt(-2 log u1) cos(2 pi u2); e[0] = z[0], e[s] = rho e[s-1] + sqrt(1 - rho^2) z[s]
 * per lane and component (stationary, unit variance; rho = 0: e = z); v[c] = x0[r][c] + sigma[k] e[s][c]; out[r][0..2] = v[0..2],
 * out[r][3..6] = v[3..6] / |v[3..6]|, all in fp64 and rounded to fp32 once (a zero norm gives what IEEE division gives). */
typedef struct {
    unsigned long long seed;   /* Philox key = (low word, high word) */
    int S, N;                  /* rows are time-major: row s*N + n; S*N < 2^31; a flat batch is S = 1 */
    int num_scales;            /* 1..8 */
    double sigma[8];           /* sqrt(variance), computed on the host in double */
    double rho;                /* 0 <= rho < 1: AR(1) coefficient along s; 0 = white */
} rpe_measure_desc;
/* x0, out: device, [S*N][7] fp32 (x, y, z, qx, qy, qz, qw), the same buffer or disjoint ones.  state: device, state[0] is the step
 * counter -- the launch reads it and advances it by one (wrapping at 2^32), so a captured call draws fresh numbers at every replay.
 * picks: device, 1 + N ints, receives [0] = the step used, [1 + n] = the scale index lane n drew.  Two launches. */
int rpe_measurement_noise(const float* x0, float* out, const rpe_measure_desc* d, unsigned* state, int* picks, void* stream);

/* Depth-sensor augmentation of raw depth frames (replaces nothing: the reference's depth transform is deterministic), fp32
 * [B][Hs][Ws] in, fp32 out, in front of rpe_stage_depth_f32_resized ("Depth augmentation").  Per pixel d, in this order:
 *   1 noise (any n_i != 0): sd = (n0 + n1 d) + (n2 d) d, v = d + sd (double)T with the integer T = 2 (h0 + .. + h5) - 6 * 65535 over
 *     the six 16-bit halves of the pixel's words r0, r1, r2 (low half first); Var T = 2 (2^32 - 1), so n_i = sigma_i / sqrt(2 (2^32 - 1))
 *   2 quantisation (q > 0): v = rint(v inv_q) q, round half even
 *   3 clamp: v = v < lo ? lo : v, then v = v > hi ? hi : v (lo = -inf and hi = +inf: off)
 *   4 dropout: hole_value iff the pixel's word r3 < drop_thresh
 *   5 holes: hole_value inside any of the first `count` of the stream's four rectangles
 *   6 shared occluder (rgb_params given): occluder_value inside the rectangle of rpe_augment_frames_u8's table where the stream erases
 * Later stages win.  1-3 are fp64 with one rounding to fp32 at the store, every product and sum rounded on its own (no fused
 * multiply-add).  The input's bit pattern is copied where 1-3 are all off and for a non-finite input; a neutral descriptor is the
 * identity.  Philox4x32-10 keyed by `seed`, bounded draws (r n) >> 32, counters
 *   (g, 0, step, 0x44455048): count = hole_lo + draw(r0, hole_hi - hole_lo + 1) of stream g
 *   (g, j, step, 0x44455052): rectangle j < 4: h = hh_lo + draw(r0, .), w = hw_lo + draw(r1, .), top = draw(r2, Hs - h + 1),
 *                             left = draw(r3, Ws - w + 1); all four are drawn and tabled
 *   (y Ws + x, b, step, 0x44455058): r0..r2 the noise, r3 the dropout of pixel (y, x) of frame b -- always per frame; run only when
 *                             noise or dropout is on */
typedef struct {
    unsigned long long seed;          /* Philox key = (low word, high word) */
    double n0, n1, n2;                /* noise coefficients, finite and >= 0; all 0 = off */
    double q, inv_q;                  /* quantisation step and 1 / q, both computed on the host in double; q = 0: off */
    double lo, hi;                    /* clamp range, lo <= hi */
    unsigned drop_thresh;             /* probability * 2^32, capped at 2^32 - 1; 0 = off */
    int hole_lo, hole_hi;             /* holes per stream, 0 <= lo <= hi <= 4 */
    int hh_lo, hh_hi, hw_lo, hw_hi;   /* hole height / width bounds in pixels, 1 <= lo <= hi <= Hs / Ws (checked when hole_hi > 0) */
    float hole_value, occluder_value; /* what a dropped / hole pixel and an occluded pixel become */
    int group;                        /* 0: frame b draws its holes from stream b; N > 0: from stream b % N */
} rpe_depth_augment_desc;
/* in / out: device, [B][Hs][Ws] fp32, the same buffer or disjoint ones; Hs * Ws < 2^32.  state: device, state[0] is the step counter --
 * the launch reads it and advances it by one (wrapping at 2^32), so a captured call draws fresh numbers at every replay.  params:
 * device, 1 + 17 G ints (G = B, or `group`), receives [0] = the step used, then per stream count and four (top, left, h, w).
 * rgb_params: null, or the table rpe_augment_frames_u8 wrote for the same batch with group == rgb_group (1 + 8 G ints, read only).
 * Refused with RPE_ERR_SHAPE before any launch: a null pointer, a non-finite or negative n_i, q or inv_q, lo > hi or a NaN bound, a
 * hole count outside 0 <= lo <= hi <= 4, rectangle bounds outside 1 <= lo <= hi <= Hs / Ws when hole_hi > 0, group < 0,
 * Hs * Ws >= 2^32, rgb_group != group with rgb_params given, in and out overlapping without being equal.  16-byte loads and stores
 * where both pointers are 16-byte aligned.  Two launches. */
int rpe_augment_depth_f32(const float* in, float* out, int B, int Hs, int Ws, const rpe_depth_augment_desc* d, unsigned* state, int* params,
                          const int* rgb_params, int rgb_group, void* stream);

/* replaces: the dropout the reference's sequence models promise and never apply ("dropout_prob ... TODO: Currently does nothing",
 * models/time_sensitive.py): inverted dropout on the rows the heads read, the mask drawn on the device ("Head dropout").
 * Element (r, c) of an fp32 [n][ld] matrix, c the ABSOLUTE column: words = Philox4x32-10 keyed by `seed` (low word, high word) at
 * counter (r, c >> 2, step, 0x44524F50 + site); the element's word is number c & 3; kept iff word >= thresh.  kept: out = x * scale,
 * one correctly rounded fp32 multiply; dropped: out = +0.0f by selection (a NaN or an infinity in a dropped position does not survive,
 * -0 does not appear).  The host derives thresh = min(2^32 - 1, round(p 2^32)) and scale = (float)(1.0 / (1.0 - p)) for 0 <= p < 1;
 * with p = 0 it launches nothing. */
typedef struct {
    unsigned long long seed;   /* Philox key: k0 = low word, k1 = high word */
    unsigned thresh;           /* an element is dropped iff its word < thresh */
    float scale;               /* what a kept element is multiplied by */
} rpe_dropout_desc;
/* state: device, state[0] is the step counter.  picks: device, one int.  The launch writes picks[0] = state[0] and advances the counter
 * by one (wrapping at 2^32); it is the only reader and writer of `state`, so a captured train step draws a fresh mask at every
 * replay.  Every rpe_dropout_rows_f32 launch of that step reads picks[0]: forward and backward agree whatever order they run in.
 * One launch. */
int rpe_dropout_begin(unsigned* state, int* picks, void* stream);
/* x, out: device, fp32 [n][ld], the same buffer (in place) or disjoint ones.  Only columns [c0, c1) are read and written; everything
 * else keeps its contents in either mode.  site 0..3 selects the purpose word, so sites draw unrelated masks in one step.  One thread
 * per aligned group of four columns, rows grid-stride; 16-byte accesses when both pointers are 16-byte aligned and ld % 4 == 0,
 * 4-byte ones for the partial groups at either end.  Refused: n < 1 or n >= 2^32, c0 < 0, c1 > ld, c0 >= c1, site outside 0..3,
 * buffers that overlap without being equal.  One launch; serves activations (forward) and gradients (backward) alike. */
int rpe_dropout_rows_f32(const float* x, float* out, long n, int ld, int c0, int c1, int site, const int* picks, const rpe_dropout_desc* d, void* stream);

/* ------------------------------------------------------------------ batch norm */
/* replaces: nn.BatchNorm2d (train mode: biased batch variance, eps, momentum with
 * unbiased running variance) + the in-place nn.ReLU and `out += identity` of the
 * torchvision Bottleneck. */
/* dpart: RPE_BN_DPART_DOUBLES(C) doubles of scratch for the staged (deterministic) partial-sum reduction: 64 doubles that hold
 * the arrival counters of the fused reduce+finalize launch, then the slice sums.  The first 64 doubles must be ZERO before the
 * first use (the kernels leave them zero again); two launches that may run concurrently need separate dpart buffers. */
#define RPE_BN_DPART_DOUBLES(C) ((long)RPE_BN_MAX_SLICES * 2 * (C) + 64)
#define RPE_BN_MAX_SLICES 256
int rpe_bn_finalize(const float* part, int tiles, int C, long count, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, long long* num_batches, float momentum, float eps, float* scale, float* shift,
                    float* save_mean, float* save_invstd, double* dpart, void* stream);
int rpe_bn_eval_affine(int C, const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                       float* scale, float* shift, void* stream);
/* out = relu?(y*scale + shift (+ residual)) */
int rpe_bn_apply(int dtype, const void* y, const void* residual, void* out, const float* scale, const float* shift, long rows, int C,
                 int relu, void* stream);
/* the same, also writing the ReLU mask as one byte per 8 channels ([rows][C/8], bit j = out[8k+j] > 0): the backward reads it
 * (1/16 of the bytes of `out`) instead of `out` to mask the gradient (rpe_bn_bwd_epilogue.a_mask).  C % 8 == 0. */
int rpe_bn_apply_mask(int dtype, const void* y, const void* residual, void* out, const float* scale, const float* shift, long rows, int C,
                      unsigned char* relu_mask, void* stream);
/* the same with a residual that is itself a raw conv output under its own BatchNorm (the projection shortcut: downsample.0 ->
 * downsample.1, no ReLU): out = [relu](y*scale + shift + res_y*res_scale + res_shift), optional packed mask -- the shortcut's own
 * apply pass and normalised copy disappear (torchvision Bottleneck.forward: `identity = self.downsample(x)`; `out += identity`) */
int rpe_bn_apply_res_bn(int dtype, const void* y, const void* res_y, const float* res_scale, const float* res_shift, void* out, const float* scale,
                        const float* shift, long rows, int C, int relu, unsigned char* relu_mask, void* stream);
/* dz = dA * (a_out > 0) (a_out null: no ReLU); dgamma, dbeta; dy = BN backward of dz; dz_out (nullable) = dz.
 * part: >= 2*1024*C floats of scratch; c1c2: 2*C floats of scratch; dpart: as for rpe_bn_finalize.
 * C: with K = C / (16-byte chunk: 4 fp32, 8 16-bit elements), K <= 256 must divide 256 and K > 256 must be a multiple of 256
 * (whole column slabs), C <= 4096; any other C is refused with RPE_ERR_SHAPE and nothing is written.  The same holds for
 * rpe_bn_backward_reduce. */
int rpe_bn_backward(int dtype, const void* dA, const void* a_out, const void* y, const float* mean, const float* invstd,
                    const float* gamma, float* dgamma, float* dbeta, void* dy, void* dz_out, long rows, int C, float* part,
                    long part_floats, float* c1c2, double* dpart, void* stream);

/* The reduction half of rpe_bn_backward alone (dgamma, dbeta, c1c2 = mean(dz), mean(dz * xhat)): for a BatchNorm whose apply pass is
 * folded into its consumers and whose sums no fused data-gradient epilogue has produced (the stride-1 projection shortcut). */
int rpe_bn_backward_reduce(int dtype, const void* dA, const void* a_out, const void* y, const float* mean, const float* invstd, const float* gamma,
                           float* dgamma, float* dbeta, long rows, int C, float* part, long part_floats, float* c1c2, double* dpart, void* stream);
/* second half of the fused form: partial sums -> dgamma, dbeta; dy = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)).
 * dy may alias dz. */
int rpe_bn_backward_from_dz(int dtype, const void* dz, const void* y, const float* mean, const float* invstd, const float* gamma,
                            const float* stats_part, int tiles, float* dgamma, float* dbeta, void* dy, long rows, int C, float* c1c2,
                            double* dpart, void* stream);

/* ------------------------------------------------------------------ pooling */
/* replaces: nn.MaxPool2d(3, 2, 1) of the ResNet stem; x [B][H][W][C] -> out, idx [B][(H-1)/2+1][(W-1)/2+1][C]; idx keeps the winning
 * tap kh * 3 + kw (0..8) of each output element.  The rule is torch's max_pool2d: padding counts as -inf (never as 0); among equal
 * values the first in-image tap in (kh, kw) order wins; a NaN beats everything and the LAST NaN of a window is named; a window whose
 * in-image taps are all -inf names its first in-image tap (never a tap outside the image).
 * B, H, W > 0 and C a positive multiple of the 16-byte chunk (4 fp32 / 8 16-bit elements), in the forward and the backward:
 * anything else is refused with RPE_ERR_SHAPE before any launch and nothing is written. */
int rpe_maxpool3x3s2_fwd(int dtype, const void* x, void* out, unsigned char* idx, int B, int H, int W, int C, void* stream);
/* BatchNorm apply + ReLU and the 3x3 / stride 2 / pad 1 max pool behind it in one pass over the raw conv output y [B][H][W][C] (H, W even):
 * a = relu(y * scale + shift) [B][H][W][C], out = maxpool(a) [B][H/2][W/2][C], idx = winner taps -- bitwise what rpe_bn_apply followed by
 * rpe_maxpool3x3s2_fwd give (replaces bn1 -> relu -> maxpool of torchvision's ResNet stem, util/model_utils.py:136). */
int rpe_bn_apply_maxpool3x3s2(int dtype, const void* y, const float* scale, const float* shift, void* a, void* out, unsigned char* idx, int B, int H,
                              int W, int C, void* stream);
/* the same pass with the bn1 aux head riding along (see rpe_resnet50_set_aux_head); 64 channels; `a` may be NULL (not written) */
int rpe_bn_apply_maxpool3x3s2_aux(int dtype, const void* y, const float* scale, const float* shift, void* a, void* out, unsigned char* idx, int B, int H,
                                  int W, const float* aux_w, const float* aux_bias, const float* depth_feat, float* aux_out, long ld_aux_out, float* aux_raw,
                                  unsigned char* aux_idx, void* stream);
/* dx [B][H][W][C] = (addend, or 0 when NULL) + the gradients dout of the windows whose idx names the pixel, summed in fp32 in
 * ascending (kh, kw) order behind the addend and rounded once.  Shapes and refusals as for the forward. */
int rpe_maxpool3x3s2_bwd(int dtype, const void* dout, const unsigned char* idx, const void* addend, void* dx, int B, int H, int W, int C,
                         void* stream);
/* Stem backward in two passes over y (fused form of rpe_maxpool3x3s2_bwd + the aux head's scatter + rpe_bn_backward for the
 * 64-channel bn1): the gradient of a1 = relu(bn1(y)) is gathered on the fly from dpool / pool_idx (B, H/2, W/2, 64) and,
 * when aux_dout != NULL, from the aux head (gradient dout[b*aux_ld + pos] (x aux_depth_feat) of the winner pixel aux_idx of
 * each 2x2 window, times aux_w[c]); the ReLU mask is recomputed from y*scale + shift.  part: >= 128 floats per block of the
 * reduction pass (up to 8192 blocks are used when it is large enough); c1c2: 128
 * floats; dpart as for rpe_bn_finalize.  replaces: autograd through torchvision's bn1 / relu / maxpool and the aux branch
 * (models/naive.py:203-211,223-231). */
int rpe_stem_bwd(int dtype, const void* dpool, const unsigned char* pool_idx, const void* y, const float* scale, const float* shift, const float* mean,
                 const float* invstd, const float* gamma, const float* aux_dout, long aux_ld, const float* aux_depth_feat,
                 const unsigned char* aux_idx, const float* aux_w, float* dgamma, float* dbeta, void* dy, int B, int H, int W, float* part,
                 long part_floats, float* c1c2, double* dpart, void* stream);
/* replaces: nn.AdaptiveAvgPool2d((1,1)) + flatten; x [B][HW][C] -> output fp32 [B][C], and its backward dx = dout / HW.
 * B, HW > 0 and C a positive multiple of the 16-byte chunk (4 fp32 / 8 16-bit elements): anything else is refused with
 * RPE_ERR_SHAPE before any launch and nothing is written. */
int rpe_avgpool_fwd(int dtype, const void* x, float* out, int B, int HW, int C, void* stream);
int rpe_avgpool_bwd(int dtype, const float* dout, void* dx, int B, int HW, int C, void* stream);

/* ------------------------------------------------------------------ heads */
/* replaces: aux_nets[i] = Conv2d(64->1,1x1) -> MaxPool2d(2) -> Flatten and the
 * `aux * depth` product (models/naive.py:223-231,318-330; time_sensitive.py:377-385,477-488).
 * out[b*ld_out + p] = max2x2(a1 . w + bias) * (depth_feat ? depth_feat[b][p] : 1); raw keeps the
 * un-multiplied value, idx the winning pixel. */
int rpe_aux_head_fwd(int dtype, const void* a1, const float* w, const float* bias, const float* depth_feat, float* out, long ld_out,
                     float* raw, unsigned char* idx, int B, int H, int W, void* stream);
/* d_a1 (dense gradient of a1, zero except the winner pixels) may be NULL when the stem backward gathers it itself (rpe_stem_bwd) */
int rpe_aux_head_bwd(int dtype, const float* dout, long ld_dout, const void* a1, const float* w, const float* depth_feat, const float* raw,
                     const unsigned char* idx, void* d_a1, float* dw, float* dbias, float* d_depth_feat, int B, int H, int W, void* stream);
/* deterministic form: the parameter gradients leave every block as plain stores into the workspace and are added in block order by a
 * second tiny launch (dw[64], dbias OVERWRITTEN, bitwise reproducible; the atomic form above accumulates) */
long rpe_aux_head_bwd_workspace_floats(int dtype, int B, int H, int W);
int rpe_aux_head_bwd_det(int dtype, const float* dout, long ld_dout, const void* a1, const float* w, const float* depth_feat, const float* raw,
                         const unsigned char* idx, void* d_a1, float* dw, float* dbias, float* d_depth_feat, int B, int H, int W, float* workspace,
                         long workspace_floats, void* stream);
/* ... and from the RAW stem conv output y with bn1's scale / shift (the activated tensor was not written: rpe_bn_apply_maxpool3x3s2_aux) */
int rpe_aux_head_bwd_det_y(int dtype, const float* dout, long ld_dout, const void* y, const float* bn_scale, const float* bn_shift, const float* w,
                           const float* depth_feat, const float* raw, const unsigned char* idx, float* dw, float* dbias, float* d_depth_feat, int B, int H,
                           int W, float* workspace, long workspace_floats, void* stream);
/* replaces: depth_nets[i] = AvgPool2d(2) x2 -> InstanceNorm2d(1, affine) -> Flatten (models/naive.py:233-240) */
int rpe_depth_head_fwd(const float* depth, const float* w, const float* b, float* feat, float* xhat, int B, int H, int W, void* stream);
int rpe_depth_head_bwd(const float* d_feat, const float* xhat, long n, float* dw, float* db, void* stream);
/* The same two heads on any hooked feature map x[B][H][W][C] (feature_layer_nums other than (9,): conv1's raw output, the layer1..3
 * outputs; models/naive.py:196-240): C = 64..1024 in whole 16-byte chunks (a power of two of them).  The backward writes a DENSE
 * gradient d_x (zeroed inside: pixels outside the 2x2 windows and the windows' losers stay zero); the depth head pools
 * `pools` = int(log4(224^2 / (H W / 4))) times, flooring odd sizes as AvgPool2d does. */
int rpe_aux_head_fwd_c(int dtype, const void* x, int C, const float* w, const float* bias, const float* depth_feat, float* out, long ld_out,
                       float* raw, unsigned char* idx, int B, int H, int W, void* stream);
int rpe_aux_head_bwd_c(int dtype, const float* dout, long ld_dout, const void* x, int C, const float* w, const float* depth_feat, const float* raw,
                       const unsigned char* idx, void* d_x, float* dw, float* dbias, float* d_depth_feat, int B, int H, int W, void* stream);
int rpe_depth_head_fwd_pools(const float* depth, const float* w, const float* b, float* feat, float* xhat, int B, int H, int W, int pools, void* stream);
/* dst += src over n elements of the compute dtype (n a multiple of the 16-byte chunk) */
int rpe_tensor_add(int dtype, void* dst, const void* src, long n, void* stream);

/* ------------------------------------------------------------------ layer capture */
/* replaces: the forward hook of visualize_layer, `output.squeeze(dim=0).detach().numpy()` (util/model_utils.py:38-40), on the engine's
 * buffers: image `image` of an NHWC activation x[..][H][W][C] in the compute dtype -> out[C][H][W] fp32 (the widening is exact) and,
 * per channel, the minimum and maximum over its FINITE values, minmax[C][2] (+inf, -inf for a channel without one; -0 == +0).
 * C a whole number of 16-byte chunks with x 16-byte aligned takes the vector path, any other C >= 1 element loads (the heads' [B][h*w]
 * vectors are H = h, W = w, C = 1 maps).  _batch: all B images of the buffer in one launch, out[B][C][H][W], minmax[B][C][2]. */
int rpe_feature_planes(int dtype, const void* x_nhwc, int image, int H, int W, int C, float* out_chw_f32, float* minmax, void* stream);
int rpe_feature_planes_batch(int dtype, const void* x_nhwc, int B, int H, int W, int C, float* out_bchw_f32, float* minmax, void* stream);
/* replaces: the subplot(n, n, i + 1) / imshow / invert_yaxis loop of visualize_layer (util/model_utils.py:88-104) up to the colour
 * lookup: one uint8 colour-INDEX image of rows = ceil(C / cols) by cols tiles, tile c at cell (c / cols, c % cols), tile pitch
 * (H + gutter, W + gutter), size rows (H + gutter) - gutter by cols (W + gutter) - gutter; gutter pixels and unused cells are 0.
 * A pixel v of channel c with (lo, hi) = minmax[c]: t = (v - lo) / (hi - lo), index = min(255, (int)(t * 256)), every operation
 * correctly rounded fp32 (matplotlib's Normalize + 256-entry lookup); hi == lo (a constant channel) or a non-finite v -> 0.
 * flip_y: tile row r shows plane row H - 1 - r (invert_yaxis). */
int rpe_feature_mosaic(const float* planes, const float* minmax, int C, int H, int W, int cols, int gutter, int flip_y, unsigned char* out_u8,
                       void* stream);

/* ------------------------------------------------------------------ occlusion sensitivity */
/* No counterpart in the reference: which pixels of a raw frame the predicted pose depends on.  One rectangle of the frame at a time is
 * set to a fill colour, the model runs, and the distance the prediction moves is the rectangle's score; the scores are spread back
 * over the pixels and drawn over the frame.  Everything is specified to the bit ("Occlusion sensitivity").
 * The grid: Gy = ceil((Hs - ph) / sy) + 1 by Gx = ceil((Ws - pw) / sx) + 1 rectangles, K = Gy Gx; rectangle k = gy Gx + gx has
 * top = min(gy sy, Hs - ph), left = min(gx sx, Ws - pw): the last row and column are clamped to the frame's edge, the origins stay
 * distinct.  A descriptor is refused (RPE_ERR_SHAPE) unless 1 <= ph <= Hs, 1 <= pw <= Ws, 1 <= sy <= ph, 1 <= sx <= pw and
 * Hs Ws < 2^31 / 3. */
typedef struct {
    int Hs, Ws;               /* frame size in pixels */
    int ph, pw;               /* rectangle size, 1 <= ph <= Hs, 1 <= pw <= Ws */
    int sy, sx;               /* distance of rectangle origins, 1 <= sy <= ph, 1 <= sx <= pw (every pixel is covered) */
    unsigned char fill_rgb[3];
} rpe_occlusion_desc;
/* host only: -> K, with *gy = Gy and *gx = Gx (either may be null); -1 with rpe_last_error set for a refused descriptor */
long rpe_occlusion_grid(const rpe_occlusion_desc* d, int* gy, int* gx);
/* frame: device, [Hs][Ws][3]; out: device, [B][Hs][Ws][3], disjoint from it.  Row 0 is the frame unchanged, row r >= 1 the frame with
 * rectangle k0 + r - 1 set to fill_rgb, a row whose rectangle number is >= K the frame unchanged (the padding of the last chunk, so
 * that every chunk runs at one batch size).  B >= 1, k0 >= 0.  16-byte loads and stores when Hs Ws 3 and both pointers are multiples
 * of 16, 4-byte when multiples of 4, single bytes otherwise.  One launch. */
int rpe_occlude_grid_u8(const unsigned char* frame, unsigned char* out, int B, int k0, const rpe_occlusion_desc* d, void* stream);
/* pred: device, [n][7] poses (x, y, z, qx, qy, qz, qw); ref: device, [7].  All arithmetic in double, the results rounded once to fp32:
 * pos[i] = sqrt(|p_i - p_ref|^2) (no epsilon); with a = q_i / |q_i|, b = q_ref / |q_ref|, dm = |a - b|, dp = |a + b|:
 * ori[i] = 4 atan2(min(dm, dp), max(dm, dp)), the rotation angle between the two orientations in [0, pi], blind to the sign of
 * either quaternion.  A row equal to ref gives exactly (0, 0) -- rpe_pose_errors' 2 acos(w) gives about 7e-4 rad when fp32 w is one
 * ulp below 1.  A zero quaternion gives NaN in ori only; no other row is touched.  One sample per thread, grid-stride, n >= 1. */
int rpe_pose_displacement(const float* pred, const float* ref, long n, float* pos, float* ori, void* stream);
/* scores: device, [M][K]; maps: device, [M][Hs][Ws]; minmax: device, [M][2].  Pixel (y, x) of map m is the mean of the scores of the
 * rectangles that cover it: an fp32 sum from 0 over the covering rectangles by ascending gy, then ascending gx, one correctly rounded
 * add each, then one correctly rounded division by their number.  A NaN score makes the pixels it covers NaN.  minmax[m] is the
 * range of map m over its finite values ((+inf, -inf) without one; -0 == +0), as rpe_feature_planes writes it.  M >= 1. */
int rpe_saliency_map(const float* scores, int M, const rpe_occlusion_desc* d, float* maps, float* minmax, void* stream);
/* frame, out: device, [Hs][Ws][3]; map: device, [Hs][Ws]; minmax: device, [2] = (lo, hi); table: device, 256 x 3 bytes.  Per pixel
 * v: t = (v - lo) / (hi - lo), k = min(255, (int)(t * 256)), every operation correctly rounded fp32 (rpe_feature_mosaic's rule;
 * hi == lo gives k = 0); a = alpha_q8 in [0, 256], or (alpha_q8 k) >> 8 when `fade` is set; per channel
 * out = (frame (256 - a) + table[k] a + 128) >> 8.  A non-finite v copies the frame's pixel.  Hs Ws < 2^31 / 3.  One launch. */
int rpe_saliency_overlay_u8(const unsigned char* frame, const float* map, const float* minmax, const unsigned char* table, int Hs, int Ws,
                            int alpha_q8, int fade, unsigned char* out, void* stream);

/* ------------------------------------------------------------------ pose overlay */
/* replaces: the second pass of the reference's rollout (util/learn_utils.py:401-403, 462-504: an indicator object moved to every estimated
 * position inside the simulator, frames recorded) without the simulator: poses are projected through a camera matrix and drawn on the
 * recorded uint8 frames.  Two launches; everything floating-point sits in the first, the second is integer only ("Pose
 * overlay"; tests/_overlay_oracle.py restates both).
 * Convention: [u w, v w, w] = P [x, y, z, 1]; u is the column and v the row of the frame AS STORED, pixel centres at integers.
 * Coordinates are Q4 (1/16 pixel) int32.  RPE_OVERLAY_INVALID in BOTH components marks a point that draws nothing. */
#define RPE_OVERLAY_INVALID (-2147483647 - 1)
#define RPE_OVERLAY_NEAR 0.0009765625 /* 2^-10: a point with w <= this is behind (or in) the camera */
#define RPE_OVERLAY_CLAMP_Q4 131072   /* 2^17: |coordinate| of a valid point */
#define RPE_OVERLAY_AXIS_Q4 8192      /* 2^13: |tip - centre| per component of a valid axis (512 px) */
#define RPE_OVERLAY_MAX_SETS 4
#define RPE_OVERLAY_MAX_TRAIL 64
#define RPE_OVERLAY_MAX_RADIUS_Q4 256
#define RPE_OVERLAY_MAX_SIDE 4096
/* poses: device, [F][G][7] fp32 (x, y, z, qx, qy, qz, qw), 1 <= G <= 4; cam: device, [C][3][4] fp64; cam_index: device, [F] int32 in
 * [0, C) (an index outside invalidates the frame's points); pos_err, ori_err: device, [F] fp32, both or neither.
 * points: device, [F][G][4][2] int32 = centre, tip of x, y, z axis, each (u, v) in Q4; bars: device, [F][2] int32.
 * One thread per (frame, pose set).  Every operation is an fp64 + - * / or sqrt, none contracted, in this order:
 *   h_r(X) = ((P[r][0] X0 + P[r][1] X1) + P[r][2] X2) + P[r][3] for r = 0, 1, 2;  (uw, vw, w) = h(X)
 *   X is valid iff uw, vw and w are finite and w > RPE_OVERLAY_NEAR (a non-finite pose or matrix entry makes them non-finite)
 *   u_q4 = clamp(floor(16 (uw / w) + 0.5), -2^17, 2^17), v_q4 alike
 *   n = sqrt(((qx qx + qy qy) + qz qz) + qw qw); the tips are invalid unless 0 < n < inf; (a, b, c, d) = q / n
 *   R e_0 = (1 - 2 (b b + c c), 2 (a b + c d), 2 (a c - b d));  R e_1 = (2 (a b - c d), 1 - 2 (a a + c c), 2 (b c + a d))
 *   R e_2 = (2 (a c + b d), 2 (b c - a d), 1 - 2 (a a + b b));  tip_i = p + axis_len (R e_i), component by component
 * A tip is invalid as well when the centre is, or when it lies more than RPE_OVERLAY_AXIS_Q4 from the centre in either component.
 * bars[f] = (bar(pos_err[f], pos_full), bar(ori_err[f], ori_full)), bar(e, full) = clamp(floor(((double)e / full) width), 0, width),
 * 0 for a NaN; (0, 0) without errors.  pos_full, ori_full > 0, 0 <= width <= 4096, axis_len finite. */
int rpe_project_poses(const float* poses, const double* cam, const int* cam_index, long F, int G, int C, double axis_len, const float* pos_err,
                      const float* ori_err, double pos_full, double ori_full, int width, int* points, int* bars, void* stream);
/* how one pose set is drawn; _lib.OverlayStyle mirrors the layout (32 bytes) */
typedef struct {
    unsigned char rgb[3];        /* the disc's and the trail's colour */
    unsigned char axis_rgb[9];   /* the colours of the x, y and z axis */
    int alpha_q8;                /* opacity, [0, 256] */
    int r_q4;                    /* disc radius, [0, 256] */
    int hw_q4;                   /* half the axes' width, [0, 256] */
    int trail;                   /* N: the centres of the N frames before are drawn too, [0, 64] */
    int trail_r_q4;              /* their radius, [0, 256] */
} rpe_overlay_style;
/* frames: device, [n][Hs][Ws][3] uint8; out: device, the same shape, disjoint from it; points / bars: device, as rpe_project_poses
 * writes them for F >= first + n frames -- frame i of `frames` is frame first + i of the list; styles: HOST, G of them.
 * Integer arithmetic only.  A point is used when neither component is RPE_OVERLAY_INVALID and both lie within +-2^17; an axis when
 * its centre and tip are and |tip - centre| <= 2^13 in both components.  Pixel (x, y) has four subsamples (16 x +- 4, 16 y +- 4); the
 * coverage of a shape is the number of them inside it:
 *   disc (c, r):      d = s - c;  d.d <= r r
 *   capsule (c, tip, hw): e = tip - c, v = s - c, t = v.e, L = e.e;  t <= 0: v.v <= hw hw;  t >= L: (v - e).(v - e) <= hw hw;
 *                     otherwise (v x e)^2 <= hw hw L;  only subsamples with lo - 8 <= s <= hi + 8 per component, lo / hi = min / max of
 *                     (c, tip) -/+ hw, are looked at, so |v| <= 2^13 + 2^9 per component and |t|, |v x e| < 2^28, (v x e)^2 < 2^56, hw hw L <= 2^43: int64
 * and a shape of colour k with coverage cov changes a byte to (px (1024 - w) + k w + 512) >> 10, w = cov * alpha (w = 0: unchanged).
 * Order: first, per set g = 0 .. G-1, the trail -- with t = (first + i) mod frames_per_episode, the union of the discs of radius
 * trail_r_q4 at the usable centres of set g in frames first + i - k, 1 <= k <= min(N, t), as ONE shape with alpha = alpha_q8 >> 1;
 * then, per set, the axes x, y, z (alpha_q8, their colours) and the disc (alpha_q8, rgb).
 * bar_px > 0: output rows Hs - 2 bar_px .. Hs - bar_px - 1 (band 0) and Hs - bar_px .. Hs - 1 (band 1) show, after the shapes, the colour
 * bar_rgb[3 band ..] where x < bars[first + i][band] and the byte >> 1 elsewhere; 2 bar_px <= Hs; bar_rgb: HOST, 6 bytes.
 * flip: stored row y is written to output row Hs - 1 - y (the bars are at the bottom of the OUTPUT).  Drawing is in stored coordinates.
 * A frame nothing is drawn on comes out byte-identical up to the flip.  16-byte loads and stores when Hs Ws 3 (with flip: Ws 3) and
 * both pointers are multiples of 16, 4-byte when multiples of 4, single bytes otherwise.  One launch.
 * Refused: n < 1, first < 0, Hs or Ws outside [1, 4096], G outside [1, 4], frames_per_episode < 1, a style outside its ranges. */
int rpe_draw_poses_u8(const unsigned char* frames, unsigned char* out, long n, int Hs, int Ws, const int* points, const int* bars, long first, int G,
                      const rpe_overlay_style* styles, int frames_per_episode, int bar_px, const unsigned char* bar_rgb, int flip, void* stream);

/* replaces: nn.Linear (+ F.relu) of the proprio-fusion MLP (models/naive.py:343-345), the
 * ResNet fc (util/model_utils.py:141), the LSTM input/recurrent GEMMs and the fc heads
 * (models/time_sensitive.py:420-423,510).  y[M][N] = x[M][K] w[N][K]^T (+bias) (+addend) (relu).
 * The data gradient is the same call with the transposed weight. */
int rpe_linear_fwd(int dtype, const void* x, int ldx, const void* w, int ldw, const float* bias, void* y, int ldy, int M, int N, int K,
                   int relu, const void* addend, int ld_add, void* stream);
/* the same with a caller-provided workspace: launches with few output tiles and a long reduction (the heads' layers at a few hundred
 * rows: 256 x 3655 -> 1024 is 64 tiles of 64 x 64 walking 229 K steps alone) are split along K, partial tiles added in a fixed order
 * by a second small launch (as rpe_conv2d_fwd_affine_ws).  The query returns 0 for shapes that are not split. */
long rpe_linear_fwd_workspace_bytes(int dtype, int M, int N, int K);
int rpe_linear_fwd_ws(int dtype, const void* x, int ldx, const void* w, int ldw, const float* bias, void* y, int ldy, int M, int N, int K,
                      int relu, const void* addend, int ld_add, void* workspace, long workspace_bytes, void* stream);
/* dw[N][K] (fp32, ld lddw) += dy[M][N]^T x[M][K]  (atomic accumulation) */
int rpe_linear_wgrad(int dtype, const void* dy, int lddy, const void* x, int ldx, float* dw, int lddw, int M, int N, int K, void* stream);
/* deterministic form (see rpe_conv2d_wgrad_det): dw = dy^T x, or dw += dy^T x when `accumulate` (one fixed-order add per element) */
long rpe_linear_wgrad_workspace_bytes(int dtype, int M, int N, int K);
int rpe_linear_wgrad_det(int dtype, const void* dy, int lddy, const void* x, int ldx, float* dw, int lddw, int M, int N, int K, int accumulate,
                         void* workspace, long workspace_bytes, void* stream);
int rpe_transpose_f32(const float* in, float* out, int rows, int cols, int ldi, int ldo, void* stream);
int rpe_relu_bwd(const float* out, const float* dy, float* dx, long n, void* stream);
int rpe_colsum(const float* x, long rows, int cols, int ld, float* out, int accumulate, void* stream);
int rpe_copy2d(const float* src, int ld_src, float* dst, int ld_dst, long rows, int cols, void* stream);

/* replaces: the pointwise part of nn.LSTM (models/time_sensitive.py:212,235,501,759,768); gate order i,f,g,o.
 * gates[N][4H] holds x W_ih^T + h W_hh^T (no biases) and is overwritten with the activated gates. */
int rpe_lstm_cell_fwd(float* gates, const float* b_ih, const float* b_hh, const float* c_prev, float* c_out, float* h_out, int N, int Hd,
                      void* stream);
int rpe_lstm_cell_bwd(const float* gates_act, const float* c_prev, const float* c_cur, const float* dh, float* dc_io, float* dgates, int N,
                      int Hd, void* stream);

/* replaces: PoseDistanceLoss.forward (models/losses.py:47-128) and its autograd backward.
 * metric 0 l2 / 1 l1 / 2 linf / 3 combined; mode 0 position / 1 pose.
 * out3 = { loss, sum_i sqrt(|dp_i|^2+eps) , sum_i |angle_i| } -- the last two are the "val" mode
 * outputs (losses.py:95-113) computed on device instead of the per-sample numpy loop.
 * grad (nullable) = d loss / d pred. */
int rpe_pose_loss(const float* pred, const float* truth, long n, int metric, int mode, float scale, float alpha, float eps, float* out3,
                  float* grad, void* stream);

/* rpe_pose_loss over the rows with valid[i] != 0 only (valid: device, n bytes) -- batches cut from episodes of unequal length, whose
 * padded lanes may hold anything.  A row with valid[i] == 0 is skipped by selection: it adds nothing to any of the three sums, its
 * grad row is written as +0.0, and neither its pred nor its truth enters any arithmetic (NaN, inf or a zero quaternion there changes
 * no bit of the result).  A valid row runs the device function rpe_pose_loss runs, in the same thread and order: with an all-ones mask
 * out3 and grad equal rpe_pose_loss' bit for bit.  All rows masked: out3 = (0, 0, 0). */
int rpe_pose_loss_masked(const float* pred, const float* truth, const unsigned char* valid, long n, int metric, int mode, float scale, float alpha,
                         float eps, float* out3, float* grad, void* stream);

/* replaces: the per-sample numpy loop of PoseDistanceLoss's "val" branch (models/losses.py:95-113) as rollout() calls it once per
 * step, and the quaternion normalisation of the printed pose (util/learn_utils.py:451-452,488-489).
 * pred, truth [n][7] fp32.  pos_err[i] = sqrtf(|dp_i|^2 + eps); ori_err[i] = |angle_i| in radians; pose_unit[n][7] (nullable) =
 * the predicted position copied and the predicted quaternion divided by its norm.  The arithmetic is that of the two validation
 * sums of rpe_pose_loss (one device function serves both): fp32 w = <qhat, t> / |t|^2 clipped to [-1, 1]; in double, angle 0
 * where sqrt(1 - w^2) == 0, else 2 acos(w), minus 2 pi above pi, then |.|.
 * An all-zero predicted quaternion gives NaN in ori_err[i] and in the quaternion of pose_unit[i], as in the reference; pos_err[i]
 * stays finite and no other row is touched.  (The SUM in rpe_pose_loss's out3[2] counts such a row as 0: its fp32 clip drops
 * the NaN.)  One sample per thread, grid-stride, any n >= 1. */
int rpe_pose_errors(const float* pred, const float* truth, long n, float eps, float* pos_err, float* ori_err, float* pose_unit,
                    void* stream);

/* replaces: np.sum / np.average per episode and np.average / np.std over all steps of the evaluation print-out
 * (util/learn_utils.py:527-538), on the device.
 * err [E][T] fp32 (episode-major).  out: 3 + 2 E doubles --
 *     out[0]            mean over all E*T values
 *     out[1]            population standard deviation (numpy's ddof = 0), two passes: the mean, then the squared deviations
 *     out[2]            maximum
 *     out[3 .. 3+E)     sum of each episode's T values
 *     out[3+E .. 3+2E)  mean of each episode's T values
 * fp64 accumulation in one fixed order by a single workgroup, no atomics: two calls give the same bits.  A NaN in `err`
 * propagates into every figure it takes part in (mean, std, max, its episode's sum and mean). */
int rpe_error_stats(const float* err, int E, int T, double* out, void* stream);
/* The same table when row e holds only lengths[e] values (lengths: device, E entries in the order of the rows, each in [1, T]) and the
 * rest of the row is padding: mean, population standard deviation and maximum run over the sum of the lengths valid values, a row's
 * sum over its first lengths[e] values and its mean is that sum / lengths[e].  Same layout, same fixed-order fp64 accumulation by one
 * workgroup without atomics.  Padding is never read into a sum or the maximum (a NaN there is invisible); a NaN in a valid entry
 * propagates as above.  With every lengths[e] == T the output equals rpe_error_stats' bit for bit. */
int rpe_error_stats_ragged(const float* err, int E, int T, const int* lengths, double* out, void* stream);

/* replaces: torch.optim.Adam(model.parameters(), lr).step() (scripts/train_model.py:228,
 * util/learn_utils.py:179) over one flat parameter / gradient / moment buffer. */
int rpe_adam_step(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2, double eps, int step,
                  void* stream);

/* Dynamic loss scaling for the RPE_F16 compute path (BASELINE config C5; the reference trains in fp32 and has no counterpart:
 * util/learn_utils.py:152-179 is the loop these three calls slot into, between loss.backward() and optimizer.step()).
 * state: 8 device floats {scale, 1/scale, found_inf, skip, finite-step streak, optimizer steps taken, -, -}; nothing is read
 * back by the host.  unscale: grads *= 1/scale, found_inf |= any non-finite.  update: found_inf -> scale *= backoff, skip = 1;
 * else steps += 1, and every `growth_interval` finite steps scale *= growth.  adam_step_amp: rpe_adam_step whose step count and
 * skip decision are read from `state` on the device. */
int rpe_amp_unscale(float* grads, long n, float* state, void* stream);
int rpe_amp_update(float* state, float growth_factor, float backoff_factor, int growth_interval, void* stream);
int rpe_adam_step_amp(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2, double eps, const float* state,
                      void* stream);

/* replaces: torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) followed by torch.optim.AdamW(..., weight_decay).step()
 * (neither is in the reference, which trains with plain Adam: scripts/train_model.py:228), over the flat gradient arena and
 * without a host round trip.
 * grad_sumsq: sum of squares of one gradient segment g[0..n), every element widened to fp64 BEFORE it is squared (1e20 does not
 *     overflow, 1e-20 does not underflow), as rpe_grad_sumsq_rows(n) fp64 partial rows written with plain stores to `partials`
 *     (the caller passes its own row offset per segment).  The row count is a function of n alone -- never of the device -- so
 *     data-parallel ranks sum in the same order.  n >= 1; g must be 16-byte aligned.
 * clip_coef: one workgroup sums `rows` partials in a fixed order in fp64 and writes state[6] = (float)sqrt(sum), state[7] =
 *     (float)min(1, max_norm / (norm + 1e-6)) -- torch's rule, evaluated in fp64 and rounded once.  max_norm <= 0 or +inf:
 *     measure only, coefficient 1.  rows == 0: norm 0, coefficient 1.  A NaN norm gives a NaN coefficient, an infinite norm 0.
 * adamw_step_clip: rpe_adam_step_amp (step count state[5], skip flag state[3]) with gc = g * state[7] when use_clip is set,
 *     m' = m + (gc - m)(1 - beta1), v' = v beta2 + gc gc (1 - beta2), p' = p (1 - lr weight_decay) - (lr / bc1) m' / (sqrt(v') /
 *     sqrt(bc2) + eps): decoupled decay applied to the old p.  g is NOT written (torch's clip scales .grad in place). */
long rpe_grad_sumsq_rows(long n);
int rpe_grad_sumsq(const float* g, long n, double* partials, void* stream);
int rpe_clip_coef(const double* partials, long rows, double max_norm, float* state, void* stream);
int rpe_adamw_step_clip(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2, double eps,
                        double weight_decay, const float* state, int use_clip, void* stream);

/* replaces: a torch.optim.lr_scheduler stepped on the host (LinearLR warm-up followed by CosineAnnealingLR / StepLR / nothing) and
 * torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay)); neither is in the reference, which builds a plain
 * Adam with no schedule (scripts/train_model.py:228).  Both live on the device, so a captured train step advances them at every replay.
 * lr_schedule: one small launch after the step bump.  e = (long)state[5] - 1, the optimizer steps taken before this one; the factor
 *     f(e) is evaluated in fp64 and rounded once:  e < warmup_steps: s + (1 - s) e / W (s = warmup_start_factor);  kind 0 (constant):
 *     1;  kind 1 (cosine): fmin + (1 - fmin)(1 + cos(pi (min(e, T) - W) / (T - W))) / 2, held at fmin beyond T = total_steps;  kind 2
 *     (step): gamma^((e - W) / step_size), the quotient floored.  sched[0] = f, sched[1] = (float)e; `sched` is a block of 4 floats of
 *     its own, and `state` is read, never written.  state[3] != 0 (a skipped fp16 step): sched stays as it was.  The count is a float:
 *     exact up to 2^24 steps.  Refused (nothing launched): warmup_steps < 0, cosine with total_steps <= warmup_steps, step_size < 1,
 *     warmup_start_factor or min_factor outside [0, 1], gamma outside (0, 1], an unknown kind, null pointers.
 * adamw_step_sched: rpe_adamw_step_clip at the rate lr (double)sched[0]: rate and decay factor 1 - lr_eff weight_decay are formed in
 *     double and rounded once each, so sched[0] == 1 and ema == NULL give rpe_adamw_step_clip's bits.  ema != NULL: ema' = ema + (p' -
 *     ema)(1 - ema_decay) from the NEW p' (ema_decay in [0, 1)).  A set skip flag leaves p, m, v and ema as they are; g is never
 *     written.  All five buffers must be 16-byte aligned.
 * swap_f32: exchanges a[0..n) and b[0..n) in place (the averaged weights into the arena and back, without an arena-sized
 *     temporary).  16-byte aligned, not overlapping. */
int rpe_lr_schedule(const float* state, int kind, long warmup_steps, double warmup_start_factor, long total_steps, double min_factor,
                    long step_size, double gamma, float* sched, void* stream);
int rpe_adamw_step_sched(float* p, const float* g, float* m, float* v, float* ema, long n, double lr, double beta1, double beta2, double eps,
                         double weight_decay, double ema_decay, const float* state, const float* sched, int use_clip, void* stream);
int rpe_swap_f32(float* a, float* b, long n, void* stream);

/* replaces: the per-layer instruments one would write in torch after optimizer.step() -- torch._foreach_norm over the gradients and
 * over the parameters, an isfinite count and a zero count per tensor, the update-to-weight ratio, and the .tolist() that brings them
 * to the host (none of it is in the reference, whose loop logs epoch averages only): several launches per
 * tensor (a ResNet-50 arena holds 161) and a host synchronisation that a captured train step cannot contain.  Here: two launches per
 * param group, nothing read by the host, gated by the device's own step count.
 * p, g, m, v: four fp32 arenas of one layout (parameters, gradients, Adam's moments), 16-byte aligned; none is written.
 * table: T entries {offset, numel, first_row} of int64 on the device, in arena order.  Tensor t is elements [offset, offset + numel)
 *     of every arena -- nothing outside these ranges is ever loaded, so padding lanes and frozen neighbours cannot reach a result --
 *     and owns the rpe_param_stats_rows(numel) partial rows from first_row on.  rpe_param_stats_rows is a function of numel alone
 *     (ceil(numel / a fixed chunk), at least 1; it needs no device), never of the device, so data-parallel ranks add in one order.
 * param_stats: one workgroup per row writes RPE_PARAM_STATS_PART_COLS fp64 values to partials[row][..] with plain stores (fixed
 *     reduction tree, no atomics).  Per element, everything widened to fp64 first: g^2, p^2, d^2 with d = (m / bc1) / (sqrt(v) /
 *     sqrt(bc2) + eps), bc1 = 1 - beta1^t, bc2 = 1 - beta2^t, t = state[5] -- rpe_adamw_step_clip's direction of the update just
 *     applied, in fp64; the non-finite counts of g and of p; the count of g == 0 (either sign); the maxima of |g| and |p|.  A
 *     non-finite element is counted and left out of every sum and maximum; a non-finite d is left out of sum d^2.
 * param_stats_finalize: one workgroup per tensor adds its rows in ascending order and writes out[t][0 .. RPE_PARAM_STATS_COLS), fp64:
 *     0 sum g^2    1 sum p^2    2 sum d^2 (0 when state[3] != 0: a skipped fp16 step applied nothing)    3 max|g|    4 max|p|
 *     5 non-finite elements of g    6 elements of g equal to 0    7 non-finite elements of p    8 stamp: state[5] of the step measured
 *     9 the first step at which column 5 or 7 was non-zero: written only while it is 0, so it stays until the host zeroes it (0: never)
 *     `out` must hold zeros (column 9 at least) before the first call.
 * Gate: every >= 1.  When (long)state[5] % every != 0 every workgroup of both kernels returns at once, and partials and out keep
 *     their contents bit for bit: a captured step launches at every replay and the device decides.
 * Refused, nothing launched: T <= 0, a null pointer, every < 1 (RPE_ERR_SHAPE); an arena that is not 16-byte aligned or an offset that
 *     is not a multiple of 4 floats (RPE_ERR_ALIGN); a negative offset or numel, or a first_row that is not the sum of the rows of the
 *     entries before it (RPE_ERR_SHAPE).  The table is checked on the HOST side of this call, from `table_host`, a host copy of the
 *     same 3 T integers passed alongside (the device table is not read back); the grid is the row total derived from it.  finalize
 *     reads the device table only: run it after a param_stats call that accepted the same table. */
#define RPE_PARAM_STATS_COLS 10
#define RPE_PARAM_STATS_PART_COLS 8
long rpe_param_stats_rows(long numel);
int rpe_param_stats(const float* p, const float* g, const float* m, const float* v, const long* table, const long* table_host, int T,
                    double* partials, double beta1, double beta2, double eps, const float* state, long every, void* stream);
int rpe_param_stats_finalize(const double* partials, const long* table, int T, double* out, const float* state, long every, void* stream);

/* ------------------------------------------------------------------ ResNet-50 trunk engine */
/* One object = one (batch, dtype) plan for the whole torchvision-shaped ResNet-50 body:
 * stage image -> conv1/bn1/relu -> maxpool -> 16 bottlenecks -> avgpool -> fc, forward and
 * backward, launched back to back on one stream with no host round trips.
 * replaces: self.feature_net(img) and its autograd backward (models/naive.py:316,
 * models/time_sensitive.py:472) including the bn1 forward hook (models/naive.py:211,282-283). */
typedef struct rpe_resnet50 rpe_resnet50_t;

#define RPE_RESNET50_NUM_CONV 53
/* parameter table order: see rpe_resnet50_param_name(); 161 fp32 tensors (53 conv w, 53 x (gamma, beta), fc w, fc b) */
#define RPE_RESNET50_NUM_PARAMS 161
/* buffer table: 53 x (running_mean, running_var) fp32 + 53 num_batches_tracked (int64) */
#define RPE_RESNET50_NUM_BUFFERS 106

int rpe_resnet50_create(rpe_resnet50_t** out, int batch, int height, int width, int dtype, int latent_dim);
/* the same engine for every ResNet the reference's import_resnet offers (util/model_utils.py:130-136): the bottleneck networks
 * depth 50 ([3,4,6,3] blocks), 101 ([3,4,23,3]) or 152 ([3,8,36,3]), and the BasicBlock networks 18 ([2,2,2,2] blocks of two 3x3
 * convs, identity shortcut in layer1.0, fc input 512) or 34 ([3,4,6,3]).  Parameter / buffer tables in torchvision's order for that
 * depth (rpe_resnet50_param_name); the rpe_resnet50_* entry points below take the handle of any depth.  The BasicBlock plan is
 * the general launch sequence (conv + statistics, finalize, apply; fused data gradient + BatchNorm reduction; dz, y -> dy; weight
 * gradients on the second stream) -- the bottleneck-only forms (folded conv3 backward, y3-free blocks) do not apply to it. */
int rpe_resnet_create(rpe_resnet50_t** out, int depth, int batch, int height, int width, int dtype, int latent_dim);
void rpe_resnet50_destroy(rpe_resnet50_t* e);
/* bytes of device workspace the engine needs (activations, gradients, packed weights, scratch) */
long rpe_resnet50_workspace_bytes(const rpe_resnet50_t* e);
/* state_dict key (torchvision naming, e.g. "layer1.0.conv1.weight") and element count of parameter i */
const char* rpe_resnet50_param_name(const rpe_resnet50_t* e, int i);
long rpe_resnet50_param_numel(const rpe_resnet50_t* e, int i);
/* host arrays of device pointers: params/grads [NUM_PARAMS] fp32 (conv weights in channels_last
 * storage = [Co][kh][kw][Ci]; conv1.weight plain OIHW), running stats [2*53], num_batches [53] */
int rpe_resnet50_bind(rpe_resnet50_t* e, void* workspace, long workspace_bytes, float* const* params_host, float* const* grads_host,
                      float* const* running_host, long long* const* num_batches_host);
/* re-pack compute-dtype copies of the weights (call after every optimizer step / load_state_dict) */
int rpe_resnet50_pack_weights(rpe_resnet50_t* e, void* stream);
/* The fp32 masters or the BN running statistics bound to this engine were changed by someone else (an optimizer step or a
 * training forward that ran through ANOTHER engine object bound to the same tensors, load_state_dict): every cached weight
 * copy -- the compute-dtype training copies and the BN-folded inference copies -- is rebuilt by the next forward.
 * replaces: nothing in the reference (torch modules read their parameters in place, util/model_utils.py:136-141). */
int rpe_resnet50_weights_changed(rpe_resnet50_t* e);
/* The engine's second stream (weight gradients in the backward, the projection shortcuts in the training forward) is PROBED when it is
 * created (first training pass): does a kernel on it run while a kernel of the caller's stream executes?  HIP deals streams to a few
 * hardware queues in creation order, and a stream that shares a queue (or, at low priority, a pipe) with the caller's serialises or
 * starves (Schedule).  candidates: streams created until one overlapped (1..4, 0 before the first training pass);
 * concurrent: 1 the stream in use overlapped, 0 none of four did, -1 not probed (RPE_NO_SIDE_PROBE=1, or created under capture). */
int rpe_resnet50_side_stream_info(const rpe_resnet50_t* e, int* candidates, int* concurrent);
/* The bn1 aux head (aux_nets[0]: Conv2d(64 -> 1, 1x1) + MaxPool2d(2) + Flatten [x the depth feature], models/naive.py:223-231,318-330)
 * computed BY the next training forward, inside the stem's BatchNorm-apply + ReLU + max-pool pass (rpe_bn_apply_maxpool3x3s2_aux): the
 * activated tensor relu(bn1(conv1 x)) is then never written (rpe_resnet50_early_feature returns NULL after such a forward) and the
 * separate aux launch with its re-read disappears.  out: the aux columns of the fused feature rows (row pitch ld_out floats); raw / idx:
 * [B][(H/4)(W/4)] window maxima and winner taps for the backward.  The setting is consumed by ONE forward; w = NULL clears it.
 * rpe_resnet50_aux_head_bwd: the head's parameter gradients (dw [64], dbias, d_depth_feat) from the raw stem output, as
 * rpe_aux_head_bwd_det computes them from a1 (workspace: rpe_aux_head_bwd_workspace_floats); its gradient towards the stem still
 * travels in compact form through rpe_resnet50_set_aux_grad. */
int rpe_resnet50_set_aux_head(rpe_resnet50_t* e, const float* w, const float* bias, const float* depth_feat, float* out, long ld_out, float* raw,
                              unsigned char* idx);
int rpe_resnet50_aux_head_bwd(rpe_resnet50_t* e, const float* dout, long ld_dout, const float* w, const float* depth_feat, const float* raw,
                              const unsigned char* idx, float* dw, float* dbias, float* d_depth_feat, float* workspace, long workspace_floats, void* stream);
/* img: (B,3,H,W) fp32 NCHW.  features: fp32 [B][ld_features] (first latent_dim columns written).
 * training != 0: batch statistics + running-stat update and everything backward needs is kept. */
int rpe_resnet50_forward(rpe_resnet50_t* e, const float* img_nchw, float* features, long ld_features, int training, void* stream);
/* the same from raw simulator frames (uint8 [B][Hs][Ws][3]): crop + normalise + stage in one kernel (rpe_stage_frames_u8) */
int rpe_resnet50_forward_u8(rpe_resnet50_t* e, const unsigned char* frames, int Hs, int Ws, const float* mean3_host, const float* std3_host,
                            float* features, long ld_features, int training, void* stream);
/* ... with the resize in front (rpe_stage_frames_u8_resized); `rs`: its geometry and device tables */
typedef struct {
    int Hr, Wr, top, left, ksx, ksy;
    const int *xb, *xk, *yb, *yk;
    unsigned char* tmp;
} rpe_resize_plan;
int rpe_resnet50_forward_u8_resized(rpe_resnet50_t* e, const unsigned char* frames, int Hs, int Ws, const rpe_resize_plan* rs, const float* mean3_host,
                                    const float* std3_host, float* features, long ld_features, int training, void* stream);
/* the hooked early feature relu(bn1(conv1 x)): NHWC [B][H/2][W/2][64] in the compute dtype (inside the workspace) */
const void* rpe_resnet50_early_feature(const rpe_resnet50_t* e);
/* gradient buffer of the early feature; the caller writes d(loss)/d(early) there (or passes use_d_early = 0) */
void* rpe_resnet50_early_grad(rpe_resnet50_t* e);
/* parameter gradients are WRITTEN (not accumulated) into the bound grad tensors */
int rpe_resnet50_backward(rpe_resnet50_t* e, const float* d_features, long ld_d_features, int use_d_early, void* stream);
/* Optional measurement aid: HIP events around every launch of the plan (on the launch stream), summed per
 * category.  enable=1 clears the counters.  Used by bench.py for the roofline line; off in timed regions. */
enum { RPE_PROF_CONV_FWD = 0, RPE_PROF_CONV_DGRAD = 1, RPE_PROF_CONV_WGRAD = 2, RPE_PROF_BN_FWD = 3, RPE_PROF_BN_BWD = 4,
       RPE_PROF_OTHER = 5, RPE_PROF_NUM = 6 };
int rpe_resnet50_profile(rpe_resnet50_t* e, int enable);
int rpe_resnet50_profile_read(rpe_resnet50_t* e, float* ms, int* launches, double* flops, double* bytes);
/* the same spans aggregated per kernel symbol: text lines "name;launches;ms;flops;bytes" (algorithmic work) written to buf; returns bytes written */
long rpe_resnet50_profile_kernels(rpe_resnet50_t* e, char* buf, long buflen);
/* short name of the implicit-GEMM kernel instance the last conv / Linear call on this thread launched,
 * e.g. "nt_kernel<bf16,2,128,4,0,3,1>" = <dtype, waves_m, BN, chunks per K-row, mode, ring depth, role> */
const char* rpe_last_kernel_name(void);
/* Walk direction of the calling thread's NEXT launches of the direction-aware kernels (the implicit-GEMM kernels and the BatchNorm apply
 * passes): every XCD owns one contiguous eighth of a launch's row tiles / spans and walks it upwards (mode 0, the default), downwards
 * (1), or alternately launch by launch starting upwards (2) -- a consumer that walks against its producer's direction reads what the
 * producer wrote last, i.e. what the 256-MiB Infinity Cache still holds of a larger tensor, first (tools/micro/mall_order.hip).
 * Results do not depend on it (partial sums are indexed by tile).  The engine sets mode 2 around its training step and restores the
 * caller's mode; RPE_NO_WALK_ALT=1 keeps it at 0.  No reference counterpart (scheduling only). */
void rpe_set_walk_direction(int mode);
/* Narrowest feature map (in pixels) whose 3x3 / stride-1 / pad-1 DETERMINISTIC weight gradient (rpe_conv2d_wgrad_det, 16-bit element types,
 * out_c % 64 == 0, in_c % 32 == 0 [% 64 for 64 output channels], width <= 60) runs in the halo form (csrc/wgrad_halo.hip: all nine taps in
 * one workgroup, x streamed once through a ring of pixels in LDS; the reduction walks the zero-padded pixel grid, which costs
 * (H + 2)(W + 2) / (H W) of the useful work -- hence a lower bound on the width).  Default 28 (RPE_WGRAD_HALO_MINW); returns the previous
 * value.  Process-wide; set it before sizing workspaces (rpe_conv2d_wgrad_workspace_bytes follows the choice).  Scheduling / summation
 * order only: no reference counterpart. */
int rpe_conv2d_wgrad_halo_min_width(int width);
/* The same backward in stages, so a data-parallel caller can all-reduce finished gradients while the rest is computed:
 * begin (fc + avgpool) -> blocks(count, join=1) ... until all 16 blocks are done -> end (stem).  After blocks(.., join=1)
 * every gradient of the blocks processed so far is complete in stream order on `stream`. */
int rpe_resnet50_backward_begin(rpe_resnet50_t* e, const float* d_features, long ld_d_features, void* stream);
int rpe_resnet50_backward_blocks(rpe_resnet50_t* e, int count, int join, void* stream);
int rpe_resnet50_backward_end(rpe_resnet50_t* e, int use_d_early, void* stream);
/* Backward of a FROZEN trunk -- import_resnet freezes every ResNet parameter when feature_extract and use_pretrained are both set
 * (util/model_utils.py:110-113,136-137; the setting of every published job: scripts/train_no.sbatch:83, train_tdo.sbatch:83,
 * train_tdo_v2.sbatch:84) and then installs a fresh, trainable fc (util/model_utils.py:140-141): only that fc's weight and bias take
 * a gradient, nothing flows into the body (no data gradient, no BN backward, no conv weight gradients: ~2/3 of the step's work).
 * The forward stays the training forward (BatchNorm on batch statistics, running statistics updated), as torch runs it. */
int rpe_resnet50_backward_frozen(rpe_resnet50_t* e, const float* d_features, long ld_d_features, void* stream);
/* Instead of a dense early-feature gradient tensor (rpe_resnet50_early_grad), hand the aux head's gradient to the next backward
 * in its compact form (see rpe_stem_bwd); the pointers must stay valid until that backward's end stage has been enqueued.
 * aux_dout == NULL clears it. */
int rpe_resnet50_set_aux_grad(rpe_resnet50_t* e, const float* aux_dout, long aux_ld, const float* aux_depth_feat, const unsigned char* aux_idx,
                              const float* aux_w);
/* debugging / parity: device pointer, rows and channels of a named intermediate (e.g. "layer1.0.y1") */
int rpe_resnet50_tensor(const rpe_resnet50_t* e, const char* name, const void** ptr, long* rows, int* channels);
/* Hooks other than bn1.  set_hook_grad: a dense gradient (compute dtype, the tensor's own NHWC shape) of conv1's raw output (layer 0:
 * `conv1.y`) or of the output of layer1..3 (`layerN.<last>.conv3.a`, see rpe_resnet50_tensor) that the NEXT backward adds where that
 * tensor's gradient is formed (layer outputs: into the shortcut gradient of the following stage-entry block; conv1: behind BN1's
 * backward, which then runs unfused); cleared by that backward; the tensor must stay alive until it has been enqueued.
 * set_stem_raw: the inference forward keeps conv1's raw output (conv and BN as two launches instead of the folded one). */
int rpe_resnet50_set_hook_grad(rpe_resnet50_t* e, int layer, const void* dense_grad);
int rpe_resnet50_set_stem_raw(rpe_resnet50_t* e, int on);

#ifdef __cplusplus
}
#endif
#endif /* RPE_HIP_H */
