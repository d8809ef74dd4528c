// Head-side kernels of the pose path: early-feature auxiliary head, depth head, LSTM cell,
// PoseDistanceLoss (+ on-device validation metrics), Adam, weight packing.  All fp32 except
// where a tensor of the conv trunk (compute type T) is read or written.
#include "common.h"

namespace rpe {

// ---------------------------------------------------------------------------------------------
// aux head: Conv2d(64 -> 1, 1x1, bias) -> MaxPool2d(2) -> Flatten  [* depth feature]
// reference: models/naive.py:223-231,318-330.  a1 = relu(bn1(conv1 x)) is [B][H][W][64] (T).
// A group of LPP = 64/CE lanes owns one output pixel (2x2 input window).
// ---------------------------------------------------------------------------------------------
// A lane's share of the 1x1 conv: products and sums rounded separately, in channel order.  Left to the compiler, two taps of a window
// were contracted to fused multiply-adds and two were not: two taps holding the same pixel then differed in the last bit (the later
// one could win the window), and bn_apply_maxpool_kernel<AUX> (norm.hip: stem_aux_dot, the same statement, which it has always
// compiled to) did not give this kernel's bits.
template <int CE>
__device__ __forceinline__ float aux_dot(const float* v, const float* w) {
#pragma clang fp contract(off)
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < CE; ++e) d += v[e] * w[e];
    return d;
}

template <typename T>
__global__ __launch_bounds__(256) void aux_fwd_kernel(const T* __restrict__ a1, const float* __restrict__ w, const float* __restrict__ bias,
                                                     const float* __restrict__ depth_feat, float* __restrict__ out, long ld_out,
                                                     float* __restrict__ raw, unsigned char* __restrict__ idx, int B, int H, int W) {
    constexpr int CE = Elem<T>::kChunk, LPP = 64 / CE;
    const int Ho = H / 2, Wo = W / 2;
    const long total = (long)B * Ho * Wo;
    const int sub = threadIdx.x % LPP;
    float wv[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) wv[e] = w[sub * CE + e];
    const float bv = bias[0];
    const int groups = blockDim.x / LPP;
    for (long o = (long)blockIdx.x * groups + threadIdx.x / LPP; o < total; o += (long)gridDim.x * groups) {
        long t = o;
        const int ow = (int)(t % Wo); t /= Wo;
        const int oh = (int)(t % Ho);
        const int b = (int)(t / Ho);
        float best = -INFINITY;
        int bi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ih = oh * 2 + (k >> 1), iw = ow * 2 + (k & 1);
            float v[CE];
            chunk_to_f<T>(*(const u32x4*)(a1 + (((long)b * H + ih) * W + iw) * 64 + sub * CE), v);
            float d = aux_dot<CE>(v, wv);
#pragma unroll
            for (int s = 1; s < LPP; s <<= 1) d += __shfl_xor(d, s);
            d += bv;
            if (d > best || d != d) { best = d; bi = k; }
        }
        if (sub == 0) {
            const long pos = (long)oh * Wo + ow;
            const float df = depth_feat ? depth_feat[(long)b * Ho * Wo + pos] : 1.f;
            out[(long)b * ld_out + pos] = best * df;
            raw[(long)b * Ho * Wo + pos] = best;
            idx[(long)b * Ho * Wo + pos] = (unsigned char)bi;
        }
    }
}

// backward: d_a1 (full tensor, zero except the winning pixel; skipped when null), dw (64), dbias, d_depth_feat
template <typename T>
__global__ __launch_bounds__(256) void aux_bwd_kernel(const float* __restrict__ dout, long ld_dout, const T* __restrict__ a1,
                                                     const float* __restrict__ w, const float* __restrict__ depth_feat,
                                                     const float* __restrict__ raw, const unsigned char* __restrict__ idx,
                                                     T* __restrict__ d_a1, float* __restrict__ dw, float* __restrict__ dbias,
                                                     float* __restrict__ d_depth_feat, int B, int H, int W, float* __restrict__ part,
                                                     const float* __restrict__ bn_scale, const float* __restrict__ bn_shift) {
    // bn_scale / bn_shift (round 4): `a1` is the RAW stem conv output y and the activated value is recomputed at the winner pixel,
    // a1 = round_T(relu(y * scale + shift)) -- the tensor itself is not written when the aux head rides on the stem's apply + pool pass
    constexpr int CE = Elem<T>::kChunk, LPP = 64 / CE;
    __shared__ float sh_dw[64];
    __shared__ float sh_db;
    if (threadIdx.x < 64) sh_dw[threadIdx.x] = 0.f;
    if (threadIdx.x == 0) sh_db = 0.f;
    __syncthreads();
    const int Ho = H / 2, Wo = W / 2;
    const long total = (long)B * Ho * Wo;
    const int sub = threadIdx.x % LPP;
    float wv[CE], gw[CE], bsc[CE], bsh[CE];
#pragma unroll
    for (int e = 0; e < CE; ++e) { wv[e] = w[sub * CE + e]; gw[e] = 0.f; bsc[e] = bn_scale ? bn_scale[sub * CE + e] : 1.f; bsh[e] = bn_scale ? bn_shift[sub * CE + e] : 0.f; }
    float gb = 0.f;
    const int groups = blockDim.x / LPP;
    for (long o = (long)blockIdx.x * groups + threadIdx.x / LPP; o < total; o += (long)gridDim.x * groups) {
        long t = o;
        const int ow = (int)(t % Wo); t /= Wo;
        const int oh = (int)(t % Ho);
        const int b = (int)(t / Ho);
        const long pos = (long)oh * Wo + ow;
        const long flat = (long)b * Ho * Wo + pos;
        float d = dout[(long)b * ld_dout + pos];
        if (depth_feat) {
            if (sub == 0 && d_depth_feat) d_depth_feat[flat] = d * raw[flat];
            d *= depth_feat[flat];
        }
        const int bi = idx[flat];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ih = oh * 2 + (k >> 1), iw = ow * 2 + (k & 1);
            const long off = (((long)b * H + ih) * W + iw) * 64 + sub * CE;
            float g[CE];
            if (k == bi) {
                float v[CE];
                chunk_to_f<T>(*(const u32x4*)(a1 + off), v);
                if (bn_scale) {
#pragma unroll
                    for (int e = 0; e < CE; ++e) v[e] = fmaxf(fmaf(v[e], bsc[e], bsh[e]), 0.f);
                    chunk_to_f<T>(f_to_chunk<T>(v), v);   // as the forward rounded it
                }
#pragma unroll
                for (int e = 0; e < CE; ++e) { g[e] = d * wv[e]; gw[e] += d * v[e]; }
            } else {
#pragma unroll
                for (int e = 0; e < CE; ++e) g[e] = 0.f;
            }
            if (d_a1) *(u32x4*)(d_a1 + off) = f_to_chunk<T>(g);
            else if (k == bi) break;   // compact form (rpe_stem_bwd gathers the a1 gradient itself): only the winner is read
        }
        if (sub == 0) gb += d;
    }
    // lanes l, l + LPP, l + 2 LPP, .. of a wave own the same channels: fold them with shuffles first, so that LPP lanes per wave
    // (not all 64) touch the shared accumulators -- the 2048 same-address LDS atomics per block were most of this kernel's time
#pragma unroll
    for (int e = 0; e < CE; ++e) {
        for (int o = LPP; o < 64; o <<= 1) gw[e] += __shfl_xor(gw[e], o);
    }
    for (int o = LPP; o < 64; o <<= 1) gb += __shfl_xor(gb, o);
    __shared__ float sh_w[4][65];   // per-wave sums, added in wave order below (no shared atomics: the block's sums are order-free)
    if ((threadIdx.x & 63) < LPP) {
#pragma unroll
        for (int e = 0; e < CE; ++e) sh_w[threadIdx.x >> 6][sub * CE + e] = gw[e];
        if (sub == 0) sh_w[threadIdx.x >> 6][64] = gb;
    }
    __syncthreads();
    if (threadIdx.x < 64) sh_dw[threadIdx.x] = ((sh_w[0][threadIdx.x] + sh_w[1][threadIdx.x]) + sh_w[2][threadIdx.x]) + sh_w[3][threadIdx.x];
    if (threadIdx.x == 64) sh_db = ((sh_w[0][64] + sh_w[1][64]) + sh_w[2][64]) + sh_w[3][64];
    __syncthreads();
    if (part) {   // deterministic form: this block's 65 sums as plain stores, added in block order by aux_bwd_reduce_kernel
        if (threadIdx.x < 64) part[(long)threadIdx.x * gridDim.x + blockIdx.x] = sh_dw[threadIdx.x];   // [65][blocks]: a column is contiguous
        if (threadIdx.x == 64) part[64L * gridDim.x + blockIdx.x] = sh_db;
        return;
    }
    if (threadIdx.x < 64) atomicAdd(&dw[threadIdx.x], sh_dw[threadIdx.x]);
    if (threadIdx.x == 0) atomicAdd(dbias, sh_db);
}

// dw[0..63], dbias = sums over the blocks of part [65][blocks]: one workgroup per column, every lane a strided share of the (contiguous)
// column, the lanes' sums folded in a fixed order
__global__ __launch_bounds__(256) void aux_bwd_reduce_kernel(const float* __restrict__ part, int blocks, float* __restrict__ dw, float* __restrict__ dbias) {
    __shared__ float sh[256];
    const int c = blockIdx.x;
    const float* col = part + (long)c * blocks;
    float s = 0.f;
    for (int r = threadIdx.x; r < blocks; r += 256) s += col[r];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) { if (c < 64) dw[c] = sh[0]; else *dbias = sh[0]; }
}

// ---------------------------------------------------------------------------------------------
// depth head: AvgPool2d(2) x2 -> InstanceNorm2d(1, affine, eps 1e-5) -> Flatten
// reference: models/naive.py:233-240.  depth is [B][1][H][W] fp32; one block per image.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void depth_fwd_kernel(const float* __restrict__ depth, const float* __restrict__ w, const float* __restrict__ b,
                                                       float* __restrict__ feat, float* __restrict__ xhat, int H, int W) {
    extern __shared__ float pooled[];  // Ho*Wo
    __shared__ double red[2][4];
    const int Ho = H / 4, Wo = W / 4, n = Ho * Wo;
    const float* img = depth + (long)blockIdx.x * H * W;
    double s = 0.0, q = 0.0;
    for (int o = threadIdx.x; o < n; o += blockDim.x) {
        const int oh = o / Wo, ow = o - oh * Wo;
        // avg of the four 2x2 averages (same association as two AvgPool2d(2) passes)
        float acc = 0.f;
        for (int a = 0; a < 2; ++a)
            for (int c = 0; c < 2; ++c) {
                const float* p = img + (long)(oh * 4 + a * 2) * W + ow * 4 + c * 2;
                acc += (p[0] + p[1] + p[W] + p[W + 1]) * 0.25f;
            }
        acc *= 0.25f;
        pooled[o] = acc;
        s += acc;
        q += (double)acc * acc;
    }
    s = wave_sum_d(s);
    q = wave_sum_d(q);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s; red[1][threadIdx.x >> 6] = q; }
    __syncthreads();
    s = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    q = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    const double mean = s / n;
    double var = q / n - mean * mean;
    if (var < 0.0) var = 0.0;
    const float invstd = (float)(1.0 / sqrt(var + 1e-5));
    const float wv = w[0], bv = b[0];
    for (int o = threadIdx.x; o < n; o += blockDim.x) {
        const float xh = (pooled[o] - (float)mean) * invstd;
        xhat[(long)blockIdx.x * n + o] = xh;
        feat[(long)blockIdx.x * n + o] = xh * wv + bv;
    }
}

// ---------------------------------------------------------------------------------------------
// The same two heads on ANY hooked feature map (models/naive.py:196-240: feature_layer_nums other than the scripts' (9,)):
// conv1's raw output, bn1, layer1..layer3 outputs -- C = 64..1024 channels, H x W = 112^2..14^2.  Not a hot path (no reference
// script hooks anything but bn1): one lane group per output pixel walking the channel chunks, a DENSE feature gradient.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void auxc_fwd_kernel(const T* __restrict__ x, int C, const float* __restrict__ w, const float* __restrict__ bias,
                                                      const float* __restrict__ depth_feat, float* __restrict__ out, long ld_out,
                                                      float* __restrict__ raw, unsigned char* __restrict__ idx, int B, int H, int W) {
    constexpr int CE = Elem<T>::kChunk;
    const int cpp = C / CE, LPP = cpp < 64 ? cpp : 64;     // chunks per pixel; lanes per output pixel (a power of two)
    const int Ho = H / 2, Wo = W / 2;
    const long total = (long)B * Ho * Wo;
    const int sub = threadIdx.x % LPP, groups = blockDim.x / LPP;
    const float bv = bias[0];
    for (long o = (long)blockIdx.x * groups + threadIdx.x / LPP; o < total; o += (long)gridDim.x * groups) {
        long t = o;
        const int ow = (int)(t % Wo); t /= Wo;
        const int oh = (int)(t % Ho);
        const int b = (int)(t / Ho);
        float best = -INFINITY;
        int bi = 0;
        for (int k = 0; k < 4; ++k) {
            const int ih = oh * 2 + (k >> 1), iw = ow * 2 + (k & 1);
            const T* px = x + (((long)b * H + ih) * W + iw) * C;
            float d = 0.f;
            for (int ch = sub; ch < cpp; ch += LPP) {
                float v[CE];
                chunk_to_f<T>(*(const u32x4*)(px + ch * CE), v);
#pragma unroll
                for (int e = 0; e < CE; ++e) d += v[e] * w[ch * CE + e];
            }
            for (int s = 1; s < LPP; s <<= 1) d += __shfl_xor(d, s);
            d += bv;
            if (d > best || d != d) { best = d; bi = k; }
        }
        if (sub == 0) {
            const long pos = (long)oh * Wo + ow;
            const float df = depth_feat ? depth_feat[(long)b * Ho * Wo + pos] : 1.f;
            out[(long)b * ld_out + pos] = best * df;
            raw[(long)b * Ho * Wo + pos] = best;
            idx[(long)b * Ho * Wo + pos] = (unsigned char)bi;
        }
    }
}

// d_x must be zero on entry (pixels outside the 2x2 windows and the three losers of every window keep a zero gradient)
template <typename T>
__global__ __launch_bounds__(256) void auxc_bwd_kernel(const float* __restrict__ dout, long ld_dout, const T* __restrict__ x, int C,
                                                      const float* __restrict__ w, const float* __restrict__ depth_feat,
                                                      const float* __restrict__ raw, const unsigned char* __restrict__ idx,
                                                      T* __restrict__ d_x, float* __restrict__ dw, float* __restrict__ dbias,
                                                      float* __restrict__ d_depth_feat, int B, int H, int W) {
    constexpr int CE = Elem<T>::kChunk;
    extern __shared__ float sh_dwc[];   // [C] + 1
    for (int i = threadIdx.x; i <= C; i += blockDim.x) sh_dwc[i] = 0.f;
    __syncthreads();
    const int cpp = C / CE, LPP = cpp < 64 ? cpp : 64;
    const int Ho = H / 2, Wo = W / 2;
    const long total = (long)B * Ho * Wo;
    const int sub = threadIdx.x % LPP, groups = blockDim.x / LPP;
    float gb = 0.f;
    for (long o = (long)blockIdx.x * groups + threadIdx.x / LPP; o < total; o += (long)gridDim.x * groups) {
        long t = o;
        const int ow = (int)(t % Wo); t /= Wo;
        const int oh = (int)(t % Ho);
        const int b = (int)(t / Ho);
        const long pos = (long)oh * Wo + ow;
        const long flat = (long)b * Ho * Wo + pos;
        float d = dout[(long)b * ld_dout + pos];
        if (depth_feat) {
            if (sub == 0 && d_depth_feat) d_depth_feat[flat] = d * raw[flat];
            d *= depth_feat[flat];
        }
        const int bi = idx[flat];
        const long pix = (((long)b * H + oh * 2 + (bi >> 1)) * W + ow * 2 + (bi & 1)) * C;
        for (int ch = sub; ch < cpp; ch += LPP) {
            float v[CE], g[CE];
            chunk_to_f<T>(*(const u32x4*)(x + pix + ch * CE), v);
#pragma unroll
            for (int e = 0; e < CE; ++e) { g[e] = d * w[ch * CE + e]; atomicAdd(&sh_dwc[ch * CE + e], d * v[e]); }
            *(u32x4*)(d_x + pix + ch * CE) = f_to_chunk<T>(g);
        }
        if (sub == 0) gb += d;
    }
    if (sub == 0) atomicAdd(&sh_dwc[C], gb);
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += blockDim.x) atomicAdd(&dw[i], sh_dwc[i]);
    if (threadIdx.x == 0) atomicAdd(dbias, sh_dwc[C]);
}

// AvgPool2d(2) x `pools` (each flooring odd sizes, as torch does) -> InstanceNorm2d(1, affine) -> Flatten: an output pixel is the mean
// of the 2^pools x 2^pools window at (oh, ow) * 2^pools.  One block per image, one wave per output pixel at a time.
__global__ __launch_bounds__(256) void depth_pools_fwd_kernel(const float* __restrict__ depth, const float* __restrict__ w, const float* __restrict__ b,
                                                             float* __restrict__ feat, float* __restrict__ xhat, int H, int W, int pools) {
    extern __shared__ float pooled[];  // Ho*Wo
    __shared__ double red[2];
    const int win = 1 << pools, Ho = H >> pools, Wo = W >> pools, n = Ho * Wo;
    const float* img = depth + (long)blockIdx.x * H * W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv = 1.f / (float)(win * win);
    for (int o = wave; o < n; o += 4) {
        const int oh = o / Wo, ow = o - oh * Wo;
        float acc = 0.f;
        for (int i = lane; i < win * win; i += 64) {
            const int r = i >> pools, c = i & (win - 1);
            acc += img[(long)(oh * win + r) * W + ow * win + c];
        }
        acc = wave_sum(acc);
        if (lane == 0) pooled[o] = acc * inv;
    }
    __syncthreads();
    if (threadIdx.x == 0) {   // n <= 3136 values: one thread sums them in double, in order
        double s = 0.0, q = 0.0;
        for (int o = 0; o < n; ++o) { s += pooled[o]; q += (double)pooled[o] * pooled[o]; }
        red[0] = s; red[1] = q;
    }
    __syncthreads();
    const double mean = red[0] / n;
    double var = red[1] / n - mean * mean;
    if (var < 0.0) var = 0.0;
    const float invstd = (float)(1.0 / sqrt(var + 1e-5));
    const float wv = w[0], bv = b[0];
    for (int o = threadIdx.x; o < n; o += blockDim.x) {
        const float xh = (pooled[o] - (float)mean) * invstd;
        xhat[(long)blockIdx.x * n + o] = xh;
        feat[(long)blockIdx.x * n + o] = xh * wv + bv;
    }
}

// dst += src over 16-byte chunks (a hooked feature's gradient joins the trunk's own gradient of that tensor)
template <typename T>
__global__ __launch_bounds__(256) void tensor_add_kernel(T* __restrict__ dst, const T* __restrict__ src, long chunks) {
    constexpr int CE = Elem<T>::kChunk;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < chunks; i += (long)gridDim.x * blockDim.x) {
        float a[CE], b[CE];
        chunk_to_f<T>(*(const u32x4*)(dst + i * CE), a);
        chunk_to_f<T>(*(const u32x4*)(src + i * CE), b);
#pragma unroll
        for (int e = 0; e < CE; ++e) a[e] += b[e];
        *(u32x4*)(dst + i * CE) = f_to_chunk<T>(a);
    }
}

// dw += sum d*xhat ; db += sum d   (the depth image itself needs no gradient)
__global__ __launch_bounds__(256) void depth_bwd_kernel(const float* __restrict__ d_feat, const float* __restrict__ xhat, long n, float* dw, float* db) {
    __shared__ float red[2][4];
    float s = 0.f, q = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float d = d_feat[i];
        s += d * xhat[i];
        q += d;
    }
    s = wave_sum(s);
    q = wave_sum(q);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s; red[1][threadIdx.x >> 6] = q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(dw, red[0][0] + red[0][1] + red[0][2] + red[0][3]);
        atomicAdd(db, red[1][0] + red[1][1] + red[1][2] + red[1][3]);
    }
}

// ---------------------------------------------------------------------------------------------
// LSTM cell (torch gate order i, f, g, o).  gates: [N][4H] pre-activations WITHOUT biases
// (x W_ih^T + h W_hh^T); overwritten with the activated gates, which the backward re-reads.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }

__global__ __launch_bounds__(256) void lstm_cell_fwd_kernel(float* __restrict__ gates, const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                           const float* __restrict__ c_prev, float* __restrict__ c_out, float* __restrict__ h_out,
                                                           int N, int Hd) {
    const long total = (long)N * Hd;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int n = (int)(i / Hd), j = (int)(i - (long)n * Hd);
        float* g = gates + (long)n * 4 * Hd;
        const float gi = sigmoidf_(g[j] + b_ih[j] + b_hh[j]);
        const float gf = sigmoidf_(g[Hd + j] + b_ih[Hd + j] + b_hh[Hd + j]);
        const float gg = tanhf(g[2 * Hd + j] + b_ih[2 * Hd + j] + b_hh[2 * Hd + j]);
        const float go = sigmoidf_(g[3 * Hd + j] + b_ih[3 * Hd + j] + b_hh[3 * Hd + j]);
        const float c = gf * (c_prev ? c_prev[i] : 0.f) + gi * gg;
        g[j] = gi; g[Hd + j] = gf; g[2 * Hd + j] = gg; g[3 * Hd + j] = go;
        c_out[i] = c;
        h_out[i] = go * tanhf(c);
    }
}

// dh: total gradient wrt h_t (output grad + recurrent); dc_io: in = dL/dc_t from step t+1, out = dL/dc_{t-1}
__global__ __launch_bounds__(256) void lstm_cell_bwd_kernel(const float* __restrict__ gates_act, const float* __restrict__ c_prev,
                                                           const float* __restrict__ c_cur, const float* __restrict__ dh,
                                                           float* __restrict__ dc_io, float* __restrict__ dgates, int N, int Hd) {
    const long total = (long)N * Hd;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int n = (int)(i / Hd), j = (int)(i - (long)n * Hd);
        const float* g = gates_act + (long)n * 4 * Hd;
        const float gi = g[j], gf = g[Hd + j], gg = g[2 * Hd + j], go = g[3 * Hd + j];
        const float tc = tanhf(c_cur[i]);
        const float dhv = dh[i];
        const float dc = dc_io[i] + dhv * go * (1.f - tc * tc);
        const float cp = c_prev ? c_prev[i] : 0.f;
        float* dg = dgates + (long)n * 4 * Hd;
        dg[j] = dc * gg * gi * (1.f - gi);
        dg[Hd + j] = dc * cp * gf * (1.f - gf);
        dg[2 * Hd + j] = dc * gi * (1.f - gg * gg);
        dg[3 * Hd + j] = dhv * tc * go * (1.f - go);
        dc_io[i] = dc * gf;
    }
}

// ---------------------------------------------------------------------------------------------
// The validation half of PoseDistanceLoss for ONE sample (models/losses.py:95-113), shared by pose_loss_kernel (which sums it) and
// pose_errors_kernel (which stores it per sample): both run these very operations, in this order.
// ---------------------------------------------------------------------------------------------
// squared position difference, summed x, y, z in that order; d[k] = p[k] - t[k]
__device__ __forceinline__ float pose_pos_sq(const float* __restrict__ p, const float* __restrict__ t, float d[3]) {
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) { d[k] = p[k] - t[k]; sq += d[k] * d[k]; }
    return sq;
}

// qhat = q / |q| (no eps: an all-zero quaternion yields NaN, as in the reference); returns <qhat, t>
__device__ __forceinline__ float pose_unit_quat(const float* __restrict__ p, const float* __restrict__ t, float h[4], float& mag) {
    const float q0 = p[3], q1 = p[4], q2 = p[5], q3 = p[6];
    mag = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    h[0] = q0 / mag; h[1] = q1 / mag; h[2] = q2 / mag; h[3] = q3 / mag;
    return h[0] * t[3] + h[1] * t[4] + h[2] * t[5] + h[3] * t[6];
}

// validation angle: w of qhat * truth^-1 (xyzw) = ip / |t|^2 in fp32, clipped; in double 2 acos(w) (0 where sqrt(1 - w^2) == 0),
// wrapped to [-pi, pi]; |.|.  The fp32 clip drops a NaN (fmaxf(NaN, -1) = -1 -> angle 0); *w_raw is the unclipped value for the
// caller that has to tell.
__device__ __forceinline__ double pose_val_angle(float ip, const float* __restrict__ t, float* w_raw) {
    const float tt = t[3] * t[3] + t[4] * t[4] + t[5] * t[5] + t[6] * t[6];
    float w = ip / tt;
    if (w_raw) *w_raw = w;
    w = fminf(fmaxf(w, -1.f), 1.f);
    double ang = 0.0;
    if (sqrt(1.0 - (double)w * (double)w) != 0.0) ang = 2.0 * acos((double)w);
    if (ang > 3.14159265358979323846) ang -= 2.0 * 3.14159265358979323846;
    return fabs(ang);
}

// ---------------------------------------------------------------------------------------------
// PoseDistanceLoss forward + gradient + validation metrics in one launch (single block).
// reference: models/losses.py:47-128.  metric: 0 l2, 1 l1, 2 linf, 3 combined; mode: 0 position, 1 pose.
// out[0] = loss, out[1] = sum_i sqrt(|dp_i|^2 + eps) (val position error), out[2] = sum_i |angle_i| (val orientation error)
// ---------------------------------------------------------------------------------------------
// one sample: its gradient row (when grad is given) and its terms of the three sums; pose_loss_kernel and pose_loss_masked_kernel both
// run this, a thread over its rows in ascending order
__device__ __forceinline__ void pose_loss_row(const float* __restrict__ pred, const float* __restrict__ truth, long i, int metric, int mode, float scale,
                                              float alpha, float eps, float* __restrict__ grad, double& l_acc, double& p_acc, double& a_acc) {
    const float* p = pred + i * 7;
    const float* t = truth + i * 7;
    float d[3], ad[3], g[7];
    const float sq = pose_pos_sq(p, t, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) { ad[k] = fabsf(d[k]); g[k] = 0.f; }
    const float l2 = sqrtf(sq + eps);
    float pos = 0.f;
    if (metric == 0 || metric == 3) {
        pos += l2;
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] += d[k] / l2;
    }
    if (metric == 1 || metric == 3) {
        pos += ad[0] + ad[1] + ad[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] += (d[k] > 0.f) ? 1.f : ((d[k] < 0.f) ? -1.f : 0.f);
    }
    if (metric == 2 || metric == 3) {
        int am = 0;  // torch.max(dim) gradient goes to the first maximal index
        if (ad[1] > ad[am]) am = 1;
        if (ad[2] > ad[am]) am = 2;
        pos += ad[am];
        g[am] += (d[am] > 0.f) ? 1.f : ((d[am] < 0.f) ? -1.f : 0.f);
    }
    // quaternion part: qhat = q / |q| (no eps: an all-zero quaternion yields NaN, as in the reference)
    float h[4], mag;
    const float ip = pose_unit_quat(p, t, h, mag);
    const float h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3];
    float ori = 0.f;
    float gh[4] = {0.f, 0.f, 0.f, 0.f};  // dL/d qhat
    if (mode == 1) {
        ori = (1.f - ip * ip) + fmaxf(-h3, 0.f);
        const float c = -2.f * ip;
        gh[0] = c * t[3]; gh[1] = c * t[4]; gh[2] = c * t[5]; gh[3] = c * t[6];
        if (-h3 >= 0.f) gh[3] -= 1.f;  // torch.clamp(min=0) passes the gradient at the boundary
    }
    // d qhat / d q = (I - qhat qhat^T) / |q|
    // (mode 0, "position": the normalised quaternion is not part of the reference's graph -- models/losses.py:124-126 --
    // so its gradient is exactly zero, also for an all-zero predicted quaternion where the Jacobian below is 0/0)
    g[3] = g[4] = g[5] = g[6] = 0.f;
    if (mode == 1) {
        const float hd = gh[0] * h0 + gh[1] * h1 + gh[2] * h2 + gh[3] * h3;
        g[3] = (gh[0] - h0 * hd) / mag; g[4] = (gh[1] - h1 * hd) / mag; g[5] = (gh[2] - h2 * hd) / mag; g[6] = (gh[3] - h3 * hd) / mag;
    }
    if (grad) {
#pragma unroll
        for (int k = 0; k < 3; ++k) grad[i * 7 + k] = scale * g[k];
#pragma unroll
        for (int k = 3; k < 7; ++k) grad[i * 7 + k] = scale * alpha * g[k];
    }
    l_acc += (double)pos + (double)alpha * (double)ori;
    p_acc += (double)l2;
    a_acc += pose_val_angle(ip, t, nullptr);
}

// the threads' partial sums -> out[0..2]: lanes by the xor butterfly, then the four waves in index order
__device__ __forceinline__ void pose_loss_finish(double l_acc, double p_acc, double a_acc, float scale, float* __restrict__ out) {
    __shared__ double red[3][4];
    l_acc = wave_sum_d(l_acc); p_acc = wave_sum_d(p_acc); a_acc = wave_sum_d(a_acc);
    if ((threadIdx.x & 63) == 0) { const int wv = threadIdx.x >> 6; red[0][wv] = l_acc; red[1][wv] = p_acc; red[2][wv] = a_acc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = scale * (float)(red[0][0] + red[0][1] + red[0][2] + red[0][3]);
        out[1] = (float)(red[1][0] + red[1][1] + red[1][2] + red[1][3]);
        out[2] = (float)(red[2][0] + red[2][1] + red[2][2] + red[2][3]);
    }
}

__global__ __launch_bounds__(256) void pose_loss_kernel(const float* __restrict__ pred, const float* __restrict__ truth, long n, int metric,
                                                       int mode, float scale, float alpha, float eps, float* __restrict__ out,
                                                       float* __restrict__ grad) {
    double l_acc = 0.0, p_acc = 0.0, a_acc = 0.0;
    for (long i = threadIdx.x; i < n; i += blockDim.x) pose_loss_row(pred, truth, i, metric, mode, scale, alpha, eps, grad, l_acc, p_acc, a_acc);
    pose_loss_finish(l_acc, p_acc, a_acc, scale, out);
}

// The same over the rows with valid[i] != 0 only (episodes of unequal length: a padded lane's output may be anything).  A masked row
// is left out by SELECTION -- neither its pred nor its truth is read, so a NaN there cannot reach a sum as 0 * NaN would -- and its
// gradient row is +0.  A valid row runs pose_loss_row in the thread and order pose_loss_kernel runs it: an all-ones mask gives its bits.
__global__ __launch_bounds__(256) void pose_loss_masked_kernel(const float* __restrict__ pred, const float* __restrict__ truth,
                                                              const unsigned char* __restrict__ valid, long n, int metric, int mode, float scale,
                                                              float alpha, float eps, float* __restrict__ out, float* __restrict__ grad) {
    double l_acc = 0.0, p_acc = 0.0, a_acc = 0.0;
    for (long i = threadIdx.x; i < n; i += blockDim.x) {
        if (valid[i]) {
            pose_loss_row(pred, truth, i, metric, mode, scale, alpha, eps, grad, l_acc, p_acc, a_acc);
        } else if (grad) {
#pragma unroll
            for (int k = 0; k < 7; ++k) grad[i * 7 + k] = 0.f;
        }
    }
    pose_loss_finish(l_acc, p_acc, a_acc, scale, out);
}

// ---------------------------------------------------------------------------------------------
// Per-sample validation errors (the "val" branch of PoseDistanceLoss, one sample per thread, grid-stride):
// pos_err[i] = sqrt(|dp_i|^2 + eps), ori_err[i] = |angle_i|, pose_unit[i] = (position, q / |q|).
// A NaN w (all-zero predicted quaternion) stays NaN, as np.clip / np.arccos keep it in the reference.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pose_errors_kernel(const float* __restrict__ pred, const float* __restrict__ truth, long n, float eps,
                                                         float* __restrict__ pos_err, float* __restrict__ ori_err, float* __restrict__ pose_unit) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float* p = pred + i * 7;
        const float* t = truth + i * 7;
        float d[3], h[4], mag, w;
        const float sq = pose_pos_sq(p, t, d);
        const float ip = pose_unit_quat(p, t, h, mag);
        const double ang = pose_val_angle(ip, t, &w);
        pos_err[i] = sqrtf(sq + eps);
        ori_err[i] = (w != w) ? w : (float)ang;
        if (pose_unit) {
            float* u = pose_unit + i * 7;
            u[0] = p[0]; u[1] = p[1]; u[2] = p[2];
            u[3] = h[0]; u[4] = h[1]; u[5] = h[2]; u[6] = h[3];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Statistics of an [E][T] fp32 error table in fp64, one workgroup, no atomics: every sum is taken in one fixed order, so two
// calls agree bit for bit.  out = { mean, population std, max, sum[E], mean[E] }.  Two passes like np.std: the mean first, then
// the squared deviations from it.  NaN propagates into every figure it takes part in (the max included).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double nan_max_d(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }

// sum over the block, the same value in every thread: lanes by the xor butterfly, then the four waves in index order
__device__ __forceinline__ double block_sum_d(double v, double* red) {
    v = wave_sum_d(v);
    __syncthreads();   // (red may still be read from the previous use)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void error_stats_kernel(const float* __restrict__ err, int E, int T, double* __restrict__ out) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long total = (long)E * T;
    double* row_sum = out + 3;
    double* row_mean = out + 3 + E;
    // per-episode sums: one wave per row, lanes stride over its T steps
    for (int e = wv; e < E; e += 4) {
        double s = 0.0;
        for (int t = lane; t < T; t += 64) s += (double)err[(long)e * T + t];
        s = wave_sum_d(s);
        if (lane == 0) { row_sum[e] = s; row_mean[e] = s / (double)T; }
    }
    __syncthreads();   // the row sums just stored are read back below by other threads of this workgroup
    double s = 0.0;
    for (int e = threadIdx.x; e < E; e += 256) s += row_sum[e];
    const double mean = block_sum_d(s, red) / (double)total;
    double q = 0.0, m = -INFINITY;
    for (long i = threadIdx.x; i < total; i += 256) {
        const double x = (double)err[i];
        const double dv = x - mean;
        q += dv * dv;
        m = nan_max_d(m, x);
    }
    q = block_sum_d(q, red);
    for (int o = 32; o > 0; o >>= 1) m = nan_max_d(m, __shfl_xor(m, o));
    __syncthreads();
    if (lane == 0) red[wv] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = mean;
        out[1] = sqrt(q / (double)total);
        out[2] = nan_max_d(nan_max_d(red[0], red[1]), nan_max_d(red[2], red[3]));
    }
}

// The same statistics over the first len_e = clamp(lengths[e], 0, T) values of every row only (episodes of unequal length; the rest of
// a row is padding and is never read into a sum or the maximum).  The walk is error_stats_kernel's -- the same threads meet the same
// elements in the same order and skip the padded ones -- so with every len_e == T the output has its bits.
__global__ __launch_bounds__(256) void error_stats_ragged_kernel(const float* __restrict__ err, int E, int T, const int* __restrict__ lengths,
                                                                double* __restrict__ out) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long total = (long)E * T;
    double* row_sum = out + 3;
    double* row_mean = out + 3 + E;
    for (int e = wv; e < E; e += 4) {
        const int len = min(max(lengths[e], 0), T);
        double s = 0.0;
        for (int t = lane; t < len; t += 64) s += (double)err[(long)e * T + t];
        s = wave_sum_d(s);
        if (lane == 0) { row_sum[e] = s; row_mean[e] = s / (double)len; }
    }
    __syncthreads();   // the row sums just stored are read back below by other threads of this workgroup
    double s = 0.0, c = 0.0;   // (the count of valid values as a double: integers below 2^53, so the sum is exact in any order)
    for (int e = threadIdx.x; e < E; e += 256) { s += row_sum[e]; c += (double)min(max(lengths[e], 0), T); }
    const double count = block_sum_d(c, red);
    const double mean = block_sum_d(s, red) / count;
    double q = 0.0, m = -INFINITY;
    for (long i = threadIdx.x; i < total; i += 256) {
        const long e = i / T;
        if ((int)(i - e * T) >= lengths[e]) continue;
        const double x = (double)err[i];
        const double dv = x - mean;
        q += dv * dv;
        m = nan_max_d(m, x);
    }
    q = block_sum_d(q, red);
    for (int o = 32; o > 0; o >>= 1) m = nan_max_d(m, __shfl_xor(m, o));
    __syncthreads();
    if (lane == 0) red[wv] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = mean;
        out[1] = sqrt(q / count);
        out[2] = nan_max_d(nan_max_d(red[0], red[1]), nan_max_d(red[2], red[3]));
    }
}

// ---------------------------------------------------------------------------------------------
// Adam over flat fp32 buffers (torch.optim.Adam defaults: no amsgrad, no weight decay)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                  long n, float lr, float omb1, float b2, float omb2, float eps, float bc1, float bc2_sqrt) {
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4 pp = ((f32x4*)p)[i], gg = ((const f32x4*)g)[i], mm = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mm[k] = mm[k] + (gg[k] - mm[k]) * omb1;
            vv[k] = vv[k] * b2 + gg[k] * gg[k] * omb2;
            const float denom = sqrtf(vv[k]) / bc2_sqrt + eps;
            pp[k] -= (lr / bc1) * (mm[k] / denom);
        }
        ((f32x4*)p)[i] = pp; ((f32x4*)m)[i] = mm; ((f32x4*)v)[i] = vv;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = (n4 << 2) + threadIdx.x;
        const float gi = g[i];
        const float mi = m[i] + (gi - m[i]) * omb1;
        const float vi = v[i] * b2 + gi * gi * omb2;
        m[i] = mi; v[i] = vi;
        p[i] -= (lr / bc1) * (mi / (sqrtf(vi) / bc2_sqrt + eps));
    }
}

// ---------------------------------------------------------------------------------------------
// Dynamic loss scaling for the fp16 compute path (config C5).  All state lives in one device array so that a train step
// never synchronises the host:  st[0] scale, st[1] 1/scale, st[2] found_inf (set by the unscale pass), st[3] skip (this
// step's decision, read by the Adam kernel), st[4] consecutive finite steps, st[5] optimizer steps taken.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void amp_unscale_kernel(float* __restrict__ g, long n, float* __restrict__ st) {
    const float inv = st[1];
    bool bad = false;
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4 v = ((f32x4*)g)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] *= inv; bad |= !(fabsf(v[k]) <= 3.4028234e38f); }   // inf or NaN
        ((f32x4*)g)[i] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = (n4 << 2) + threadIdx.x;
        const float v = g[i] * inv;
        g[i] = v;
        bad |= !(fabsf(v) <= 3.4028234e38f);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) st[2] = 1.f;   // same value from every writer: a plain store is enough
}

__global__ void amp_update_kernel(float* __restrict__ st, float growth, float backoff, int interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (st[2] != 0.f) {
        st[0] = fmaxf(st[0] * backoff, 1.f); st[1] = 1.f / st[0];
        st[3] = 1.f; st[4] = 0.f;
    } else {
        st[3] = 0.f; st[5] += 1.f;
        const float t = st[4] + 1.f;
        if (t >= (float)interval) { st[0] = fminf(st[0] * growth, 16777216.f); st[1] = 1.f / st[0]; st[4] = 0.f; }
        else st[4] = t;
    }
    st[2] = 0.f;
}

// Adam whose step count and skip decision live on the device (same update rule as adam_kernel)
__global__ __launch_bounds__(256) void adam_amp_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                      long n, float lr, double b1, double b2, float eps, const float* __restrict__ st) {
    if (st[3] != 0.f) return;   // non-finite gradients this step: parameters and moments stay as they are
    const double step = (double)st[5];
    const float bc1 = (float)(1.0 - pow(b1, step)), bc2_sqrt = (float)sqrt(1.0 - pow(b2, step));
    const float omb1 = (float)(1.0 - b1), omb2 = (float)(1.0 - b2), fb2 = (float)b2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float gi = g[i];
        const float mi = m[i] + (gi - m[i]) * omb1;
        const float vi = v[i] * fb2 + gi * gi * omb2;
        m[i] = mi; v[i] = vi;
        p[i] -= (lr / bc1) * (mi / (sqrtf(vi) / bc2_sqrt + eps));
    }
}

// ---------------------------------------------------------------------------------------------
// Global gradient-norm clipping + decoupled weight decay (torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW over the arena).
// st[6] gradient norm and st[7] clip coefficient join the state block above.  Three launches, nothing read by the host:
//   grad_sumsq_kernel   per segment: fp64 sum of squares as one partial row per block (plain stores, no atomics, no fences: the
//                       launch boundary publishes the rows).  The grid is a function of n alone (grad_sumsq_rows), so two
//                       data-parallel ranks, whatever their devices, add the same numbers in the same order.
//   clip_coef_kernel    one workgroup adds the rows in a fixed order and writes norm and coefficient.
//   adamw_clip_kernel   the update; g is read, never written.
// ---------------------------------------------------------------------------------------------
constexpr long kSumsqMaxRows = 1024;      // blocks (= partial rows) per segment at most
constexpr long kSumsqBlockElems = 1024;   // elements one block takes per grid-stride trip: 256 threads x one 16-byte load

static inline long grad_sumsq_rows(long n) {
    long r = (n + kSumsqBlockElems - 1) / kSumsqBlockElems;
    return r < 1 ? 1 : (r > kSumsqMaxRows ? kSumsqMaxRows : r);
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long n, double* __restrict__ part) {
    __shared__ double red[4];
    const long n4 = n >> 2;
    double acc = 0.0;
#pragma unroll 4
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 gg = ((const f32x4*)g)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double x = (double)gg[k];   // widened BEFORE the square: 1e20 does not overflow, 1e-20 does not underflow
            acc += x * x;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const double x = (double)g[(n4 << 2) + threadIdx.x];
        acc += x * x;
    }
    acc = block_sum_d(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void clip_coef_kernel(const double* __restrict__ part, long rows, double max_norm, float* __restrict__ st) {
    __shared__ double red[4];
    double acc = 0.0;
    for (long i = threadIdx.x; i < rows; i += 256) acc += part[i];
    const double norm = sqrt(block_sum_d(acc, red));
    if (threadIdx.x != 0) return;
    double coef = 1.0;
    if (max_norm > 0.0 && max_norm <= 1.7976931348623157e308) {   // else (<= 0, +inf, NaN): measure only
        const double c = max_norm / (norm + 1e-6);
        coef = (c > 1.0) ? 1.0 : c;   // not fmin: a NaN norm stays a NaN coefficient (torch, error_if_nonfinite=False); inf -> 0
    }
    st[6] = (float)norm;
    st[7] = (float)coef;
}

// adam_amp_kernel's device-side step count and skip flag, adam_kernel's 4-wide body; decay = 1 - lr weight_decay multiplies the
// OLD p (torch.optim.AdamW's order), coef = st[7] scales the gradient on its way into both moments
__global__ __launch_bounds__(256) void adamw_clip_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                        long n, float lr, double b1, double b2, float eps, float decay, const float* __restrict__ st,
                                                        int use_clip) {
    if (st[3] != 0.f) return;   // non-finite gradients this step: parameters and moments stay as they are
    const double step = (double)st[5];
    const float bc1 = (float)(1.0 - pow(b1, step)), bc2_sqrt = (float)sqrt(1.0 - pow(b2, step));
    const float omb1 = (float)(1.0 - b1), omb2 = (float)(1.0 - b2), fb2 = (float)b2;
    const float coef = use_clip ? st[7] : 1.f;   // (g * 1.f is g)
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4 pp = ((f32x4*)p)[i], gg = ((const f32x4*)g)[i], mm = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gc = gg[k] * coef;
            mm[k] = mm[k] + (gc - mm[k]) * omb1;
            vv[k] = vv[k] * fb2 + gc * gc * omb2;
            const float denom = sqrtf(vv[k]) / bc2_sqrt + eps;
            pp[k] = pp[k] * decay - (lr / bc1) * (mm[k] / denom);
        }
        ((f32x4*)p)[i] = pp; ((f32x4*)m)[i] = mm; ((f32x4*)v)[i] = vv;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = (n4 << 2) + threadIdx.x;
        const float gc = g[i] * coef;
        const float mi = m[i] + (gc - m[i]) * omb1;
        const float vi = v[i] * fb2 + gc * gc * omb2;
        m[i] = mi; v[i] = vi;
        p[i] = p[i] * decay - (lr / bc1) * (mi / (sqrtf(vi) / bc2_sqrt + eps));
    }
}

// ---------------------------------------------------------------------------------------------
// Learning-rate schedule on the device + weight EMA fused into the update.  sched: 4 floats of its own, sched[0] the factor that
// multiplies lr, sched[1] the optimizer steps taken before this one; the 8-float state block is read, never written.
//   lr_schedule_kernel  one thread, after the step bump: e = st[5] - 1, f(e) in fp64, rounded once.  A skipped fp16 step leaves
//                       sched as it was (st[5] did not advance either).
//   adamw_sched_kernel  adamw_clip_kernel with lr_eff = lr sched[0], and ema' = ema + (p' - ema)(1 - ema_decay) from the register
//                       that holds the new p.
//   swap_f32_kernel     in-place exchange of two buffers (the average into the arena and back).
// ---------------------------------------------------------------------------------------------
enum { kSchedConstant = 0, kSchedCosine = 1, kSchedStep = 2 };

__global__ void lr_schedule_kernel(const float* __restrict__ st, int kind, long W, double s, long T, double fmin, long step_size, double gamma,
                                   float* __restrict__ sched) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (st[3] != 0.f) return;   // a skipped step does not advance the schedule
    long e = (long)st[5] - 1;
    if (e < 0) e = 0;
    double f = 1.0;
    if (e < W) {
        f = s + (1.0 - s) * (double)e / (double)W;
    } else if (kind == kSchedCosine) {
        const long ec = e < T ? e : T;   // beyond T: hold fmin
        f = fmin + (1.0 - fmin) * (1.0 + cos(3.141592653589793 * (double)(ec - W) / (double)(T - W))) / 2.0;
    } else if (kind == kSchedStep) {
        f = pow(gamma, (double)((e - W) / step_size));
    }
    sched[0] = (float)f;
    sched[1] = (float)e;
}

// the two scalars rpe_adamw_step_clip forms on the host, formed here from lr sched[0]: product and difference rounded separately (no
// fused multiply-add), so that a factor of exactly 1 gives the host's bits
__device__ inline void sched_rate(double lr, double wd, float factor, float* lr_eff, float* decay) {
#pragma clang fp contract(off)
    const double r = lr * (double)factor;
    const double prod = r * wd;
    *lr_eff = (float)r;
    *decay = (float)(1.0 - prod);
}

template <bool EMA>
__global__ __launch_bounds__(256) void adamw_sched_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                         float* __restrict__ ema, long n, double lr_base, double b1, double b2, float eps, double wd,
                                                         float omd, const float* __restrict__ st, const float* __restrict__ sched, int use_clip) {
    if (st[3] != 0.f) return;   // non-finite gradients this step: parameters, moments and average stay as they are
    const double step = (double)st[5];
    const float bc1 = (float)(1.0 - pow(b1, step)), bc2_sqrt = (float)sqrt(1.0 - pow(b2, step));
    const float omb1 = (float)(1.0 - b1), omb2 = (float)(1.0 - b2), fb2 = (float)b2;
    const float coef = use_clip ? st[7] : 1.f;   // (g * 1.f is g)
    float lr, decay;
    sched_rate(lr_base, wd, sched[0], &lr, &decay);
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4 pp = ((f32x4*)p)[i], gg = ((const f32x4*)g)[i], mm = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gc = gg[k] * coef;
            mm[k] = mm[k] + (gc - mm[k]) * omb1;
            vv[k] = vv[k] * fb2 + gc * gc * omb2;
            const float denom = sqrtf(vv[k]) / bc2_sqrt + eps;
            pp[k] = pp[k] * decay - (lr / bc1) * (mm[k] / denom);
        }
        ((f32x4*)p)[i] = pp; ((f32x4*)m)[i] = mm; ((f32x4*)v)[i] = vv;
        if (EMA) {
            f32x4 ee = ((f32x4*)ema)[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) ee[k] = ee[k] + (pp[k] - ee[k]) * omd;
            ((f32x4*)ema)[i] = ee;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = (n4 << 2) + threadIdx.x;
        const float gc = g[i] * coef;
        const float mi = m[i] + (gc - m[i]) * omb1;
        const float vi = v[i] * fb2 + gc * gc * omb2;
        m[i] = mi; v[i] = vi;
        const float pi = p[i] * decay - (lr / bc1) * (mi / (sqrtf(vi) / bc2_sqrt + eps));
        p[i] = pi;
        if (EMA) ema[i] = ema[i] + (pi - ema[i]) * omd;
    }
}

__global__ __launch_bounds__(256) void swap_f32_kernel(float* __restrict__ a, float* __restrict__ b, long n) {
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 x = ((f32x4*)a)[i], y = ((f32x4*)b)[i];
        ((f32x4*)a)[i] = y; ((f32x4*)b)[i] = x;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = (n4 << 2) + threadIdx.x;
        const float x = a[i], y = b[i];
        a[i] = y; b[i] = x;
    }
}

// ---------------------------------------------------------------------------------------------
// weight packing / small utilities
// ---------------------------------------------------------------------------------------------
// w: [Co][R][S][Ci] fp32 (channels_last storage of an OIHW parameter)
//   -> fwd  [Co][R*S*Ci]   (T, only when T != float: the fp32 master already has this layout)
//   -> dgrad [Ci][R][S][Co] (T)
template <typename T>
__global__ __launch_bounds__(256) void pack_conv_weight_kernel(const float* __restrict__ w, T* __restrict__ wf, T* __restrict__ wd, int Co, int RS, int Ci) {
    const long total = (long)Co * RS * Ci;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int ci = (int)(i % Ci);
        const long t = i / Ci;
        const int rs = (int)(t % RS), co = (int)(t / RS);
        const float v = w[i];
        if (wf) wf[i] = Elem<T>::from_f(v);
        if (wd) wd[((long)ci * RS + rs) * Co + co] = Elem<T>::from_f(v);
    }
}

template <typename T> __device__ inline void store4(T* o, float a, float b, float c, float d);
template <> __device__ inline void store4<float>(float* o, float a, float b, float c, float d) { *(f32x4*)o = f32x4{a, b, c, d}; }
template <> __device__ inline void store4<bf16>(bf16* o, float a, float b, float c, float d) {
    u32x2 v; v.x = pack_bf16x2(a, b); v.y = pack_bf16x2(c, d);
    *(u32x2*)o = v;
}
template <> __device__ inline void store4<f16>(f16* o, float a, float b, float c, float d) {
    u32x2 v; v.x = pack_f16x2(a, b); v.y = pack_f16x2(c, d);
    *(u32x2*)o = v;
}

// all conv layers of a trunk in ONE launch: a table of per-layer descriptors, flat element index space.
// Layers whose Co and Ci are multiples of 64 (every trunk conv) go 64x64 tile by tile through LDS, so both the source read
// and the two destination writes (forward layout = source order; data-gradient layout = [Ci][RS][Co], a transpose) move
// whole 128/256-byte rows; other layers fall back to element-wise scatter.
constexpr int kPackMaxLayers = 255;
template <typename T>
__global__ __launch_bounds__(256) void pack_conv_weights_multi_kernel(const rpe_pack_desc* __restrict__ tab, int nlayers, long total) {
    __shared__ long starts[kPackMaxLayers + 1];   // (ResNet-152 has 154 packed convs)
    __shared__ float tile[64][65];
    for (int i = threadIdx.x; i <= nlayers && i <= kPackMaxLayers; i += blockDim.x) starts[i] = i < nlayers ? tab[i].start : total;
    __syncthreads();
    const long chunk = 4096;   // one 64x64 tile; layer starts are multiples of it whenever Co, Ci are multiples of 64
    const int tr = threadIdx.x >> 4, tc = (threadIdx.x & 15) * 4;
    for (long base = (long)blockIdx.x * chunk; base < total; base += (long)gridDim.x * chunk) {
        int l = 0;
        while (l + 1 < nlayers && starts[l + 1] <= base) ++l;
        const rpe_pack_desc d = tab[l];
        const bool tiled = (d.Co % 64 == 0) && (d.Ci % 64 == 0) && (d.start % chunk == 0) && starts[l + 1] >= base + chunk;
        if (tiled) {
            const long t = (base - d.start) / chunk;
            const int cit = d.Ci / 64;
            const int ci0 = (int)(t % cit) * 64;
            const int rs = (int)((t / cit) % d.RS);
            const int co0 = (int)(t / ((long)cit * d.RS)) * 64;
            __syncthreads();   // previous tile fully consumed
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int co = tr + 16 * it;
                const long j = ((long)(co0 + co) * d.RS + rs) * d.Ci + ci0 + tc;
                f32x4 v = *(const f32x4*)(d.src + j);
                tile[co][tc] = v.x; tile[co][tc + 1] = v.y; tile[co][tc + 2] = v.z; tile[co][tc + 3] = v.w;
                if (d.wf) {
                    if (d.scale) { const float sc = d.scale[co0 + co]; v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc; }   // tile[] keeps the unscaled value for wd
                    store4<T>((T*)d.wf + j, v.x, v.y, v.z, v.w);
                }
            }
            __syncthreads();
            if (d.wd) {
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const int ci = tr + 16 * it;
                    store4<T>((T*)d.wd + ((long)(ci0 + ci) * d.RS + rs) * d.Co + co0 + tc, tile[tc][ci], tile[tc + 1][ci], tile[tc + 2][ci],
                              tile[tc + 3][ci]);
                }
            }
            continue;
        }
        for (long i = base + threadIdx.x; i < base + chunk && i < total; i += blockDim.x) {
            int ll = l;
            while (ll + 1 < nlayers && starts[ll + 1] <= i) ++ll;
            const rpe_pack_desc e = tab[ll];
            const long j = i - e.start;
            const int ci = (int)(j % e.Ci);
            const long t = j / e.Ci;
            const int rs = (int)(t % e.RS), co = (int)(t / e.RS);
            const float v = e.src[j];
            if (e.wf) ((T*)e.wf)[j] = Elem<T>::from_f(e.scale ? v * e.scale[co] : v);
            if (e.wd) ((T*)e.wd)[((long)ci * e.RS + rs) * e.Co + co] = Elem<T>::from_f(v);
        }
    }
}

// stem: OIHW [64][3][7][7] fp32 -> [64][8][8][4] T (taps and channel zero padded)
template <typename T>
__global__ void pack_stem_weight_kernel(const float* __restrict__ w, const float* __restrict__ scale, T* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 64 * 256) return;
    const int c = i & 3, s = (i >> 2) & 7, r = (i >> 5) & 7, co = i >> 8;
    float v = 0.f;
    if (c < 3 && s < 7 && r < 7) v = w[((co * 3 + c) * 7 + r) * 7 + s];
    if (scale) v *= scale[co];
    out[i] = Elem<T>::from_f(v);
}
__global__ void unpack_stem_grad_kernel(const float* __restrict__ d, float* __restrict__ dw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 64 * 3 * 49) return;
    const int s = i % 7, r = (i / 7) % 7, c = (i / 49) % 3, co = i / 147;
    dw[i] = d[((co * 8 + r) * 8 + s) * 4 + c];
}

// out[c][r] = in[r][c]  (fp32, out leading dimension ldo >= rows, zero padded)
__global__ __launch_bounds__(256) void transpose_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int rows, int cols, int ldi, int ldo) {
    __shared__ float tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int k = ty; k < 32; k += 8) {
        const int r = by + k, c = bx + tx;
        tile[k][tx] = (r < rows && c < cols) ? in[(long)r * ldi + c] : 0.f;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int c = bx + k, r = by + tx;
        if (c < cols && r < ldo) out[(long)c * ldo + r] = (r < rows) ? tile[tx][k] : 0.f;
    }
}

// dy *= (out > 0)
__global__ __launch_bounds__(256) void relu_bwd_kernel(const float* __restrict__ out, const float* __restrict__ dy, float* __restrict__ dx, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) dx[i] = out[i] > 0.f ? dy[i] : 0.f;
}

// db[c] (+)= sum_r x[r][c]
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ x, long rows, int cols, int ld, float* __restrict__ out, int accumulate) {
    __shared__ float sh[8][32];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    float s = 0.f;
    if (c < cols)
        for (long r = rl; r < rows; r += 8) s += x[r * ld + c];
    sh[rl][cl] = s;
    __syncthreads();
    if (rl == 0 && c < cols) {
        for (int i = 1; i < 8; ++i) s += sh[i][cl];
        out[c] = accumulate ? out[c] + s : s;
    }
}

// dst[r][off + c] = src[r][c]  (fp32 strided copy used to assemble the fused feature rows)
__global__ __launch_bounds__(256) void copy2d_kernel(const float* __restrict__ src, int lds_, float* __restrict__ dst, int ldd, long rows, int cols) {
    const long total = rows * cols;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cols;
        const int c = (int)(i - r * cols);
        dst[r * ldd + c] = src[r * lds_ + c];
    }
}

static inline int ew_grid(long n, int per_block = 256) {
    long g = (n + per_block - 1) / per_block;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace rpe

using namespace rpe;

extern "C" {

int rpe_aux_head_fwd(int dtype, const void* a1, const float* w, const float* bias, const float* depth_feat, float* out, long ld_out,
                     float* raw, unsigned char* idx, int B, int H, int W, void* stream) {
    if ((H | W) & 1) return rpe_set_error(RPE_ERR_SHAPE, "aux_head: H and W must be even");
    const long total = (long)B * (H / 2) * (W / 2);
    if (dtype == RPE_F32) hipLaunchKernelGGL((aux_fwd_kernel<float>), dim3(ew_grid(total, 16)), dim3(256), 0, (hipStream_t)stream, (const float*)a1, w, bias, depth_feat, out, ld_out, raw, idx, B, H, W);
    else if (dtype == RPE_BF16) hipLaunchKernelGGL((aux_fwd_kernel<bf16>), dim3(ew_grid(total, 32)), dim3(256), 0, (hipStream_t)stream, (const bf16*)a1, w, bias, depth_feat, out, ld_out, raw, idx, B, H, W);
    else if (dtype == RPE_F16) hipLaunchKernelGGL((aux_fwd_kernel<f16>), dim3(ew_grid(total, 32)), dim3(256), 0, (hipStream_t)stream, (const f16*)a1, w, bias, depth_feat, out, ld_out, raw, idx, B, H, W);
    else return rpe_set_error(RPE_ERR_DTYPE, "aux_head: unsupported dtype");
    RPE_CHECK_LAUNCH();
    return 0;
}

static int aux_bwd_launch(int dtype, const float* dout, long ld_dout, const void* a1, const float* w, const float* depth_feat, const float* raw,
                          const unsigned char* idx, void* d_a1, float* dw, float* dbias, float* d_depth_feat, int B, int H, int W, float* part,
                          long part_floats, void* stream, const float* bn_scale = nullptr, const float* bn_shift = nullptr);

long rpe_aux_head_bwd_workspace_floats(int dtype, int B, int H, int W) {
    const long total = (long)B * (H / 2) * (W / 2);
    return (long)ew_grid(total, (dtype == RPE_F32 ? 16 : 32) * 4) * 65;
}

/* deterministic form: per-block partial sums through the workspace, added in a fixed order; dw / dbias are OVERWRITTEN */
int rpe_aux_head_bwd_det(int dtype, const float* dout, long ld_dout, const void* a1, const float* w, const float* depth_feat, const float* raw,
                         const unsigned char* idx, void* d_a1, float* dw, float* dbias, float* d_depth_feat, int B, int H, int W, float* workspace,
                         long workspace_floats, void* stream) {
    if (!workspace || workspace_floats < rpe_aux_head_bwd_workspace_floats(dtype, B, H, W))
        return rpe_set_error(RPE_ERR_WORKSPACE, "aux_head_bwd_det: workspace smaller than rpe_aux_head_bwd_workspace_floats()");
    return aux_bwd_launch(dtype, dout, ld_dout, a1, w, depth_feat, raw, idx, d_a1, dw, dbias, d_depth_feat, B, H, W, workspace, workspace_floats, stream);
}

int rpe_aux_head_bwd(int dtype, const float* dout, long ld_dout, const void* a1, const float* w, const float* depth_feat, const float* raw,
                     const unsigned char* idx, void* d_a1, float* dw, float* dbias, float* d_depth_feat, int B, int H, int W, void* stream) {
    return aux_bwd_launch(dtype, dout, ld_dout, a1, w, depth_feat, raw, idx, d_a1, dw, dbias, d_depth_feat, B, H, W, nullptr, 0, stream);
}

/* the same from the RAW stem conv output y and bn1's scale / shift: the activated tensor a1 was never written (rpe_bn_apply_maxpool3x3s2_aux
 * with a = NULL); compact form only (the stem backward gathers the a1 gradient itself: rpe_stem_bwd) */
int rpe_aux_head_bwd_det_y(int dtype, const float* dout, long ld_dout, const void* y, const float* bn_scale, const float* bn_shift, const float* w,
                           const float* depth_feat, const float* raw, const unsigned char* idx, float* dw, float* dbias, float* d_depth_feat, int B, int H,
                           int W, float* workspace, long workspace_floats, void* stream) {
    if (!y || !bn_scale || !bn_shift) return rpe_set_error(RPE_ERR_SHAPE, "aux_head_bwd_det_y: y, scale and shift are required");
    if (!workspace || workspace_floats < rpe_aux_head_bwd_workspace_floats(dtype, B, H, W))
        return rpe_set_error(RPE_ERR_WORKSPACE, "aux_head_bwd_det_y: workspace smaller than rpe_aux_head_bwd_workspace_floats()");
    return aux_bwd_launch(dtype, dout, ld_dout, y, w, depth_feat, raw, idx, nullptr, dw, dbias, d_depth_feat, B, H, W, workspace, workspace_floats, stream, bn_scale, bn_shift);
}

static int aux_bwd_launch(int dtype, const float* dout, long ld_dout, const void* a1, const float* w, const float* depth_feat, const float* raw,
                          const unsigned char* idx, void* d_a1, float* dw, float* dbias, float* d_depth_feat, int B, int H, int W, float* part,
                          long part_floats, void* stream, const float* bn_scale, const float* bn_shift) {
    const long total = (long)B * (H / 2) * (W / 2);
    // the gather is latency-bound (winner index -> winner pixel): many short blocks when their sums leave as plain stores (part);
    // with global atomics every block ends in 65 adds on the same 65 addresses, which is what then bounds the launch: fewer blocks
    int g = ew_grid(total, (dtype == RPE_F32 ? 16 : 32) * 4);
    if (!part && g > 1024) g = 1024;
    if (dtype == RPE_F32) hipLaunchKernelGGL((aux_bwd_kernel<float>), dim3(g), dim3(256), 0, (hipStream_t)stream, dout, ld_dout, (const float*)a1, w, depth_feat, raw, idx, (float*)d_a1, dw, dbias, d_depth_feat, B, H, W, part, bn_scale, bn_shift);
    else if (dtype == RPE_BF16) hipLaunchKernelGGL((aux_bwd_kernel<bf16>), dim3(g), dim3(256), 0, (hipStream_t)stream, dout, ld_dout, (const bf16*)a1, w, depth_feat, raw, idx, (bf16*)d_a1, dw, dbias, d_depth_feat, B, H, W, part, bn_scale, bn_shift);
    else if (dtype == RPE_F16) hipLaunchKernelGGL((aux_bwd_kernel<f16>), dim3(g), dim3(256), 0, (hipStream_t)stream, dout, ld_dout, (const f16*)a1, w, depth_feat, raw, idx, (f16*)d_a1, dw, dbias, d_depth_feat, B, H, W, part, bn_scale, bn_shift);
    else return rpe_set_error(RPE_ERR_DTYPE, "aux_head: unsupported dtype");
    RPE_CHECK_LAUNCH();
    if (part) {
        hipLaunchKernelGGL(aux_bwd_reduce_kernel, dim3(65), dim3(256), 0, (hipStream_t)stream, (const float*)part, g, dw, dbias);
        RPE_CHECK_LAUNCH();
    }
    return 0;
}

int rpe_depth_head_fwd(const float* depth, const float* w, const float* b, float* feat, float* xhat, int B, int H, int W, void* stream) {
    if ((H | W) & 3) return rpe_set_error(RPE_ERR_SHAPE, "depth_head: H and W must be multiples of 4");
    const size_t sh = (size_t)(H / 4) * (W / 4) * sizeof(float);
    hipLaunchKernelGGL(depth_fwd_kernel, dim3(B), dim3(256), sh, (hipStream_t)stream, depth, w, b, feat, xhat, H, W);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_tensor_add(int dtype, void* dst, const void* src, long n, void* stream) {
    const int ce = dtype == RPE_F32 ? 4 : 8;
    if (n <= 0 || (n % ce) || !dst || !src) return rpe_set_error(RPE_ERR_SHAPE, "tensor_add: n must be a positive multiple of the 16-byte chunk");
    const int g = ew_grid(n / ce);
    if (dtype == RPE_F32) hipLaunchKernelGGL((tensor_add_kernel<float>), dim3(g), dim3(256), 0, (hipStream_t)stream, (float*)dst, (const float*)src, n / ce);
    else if (dtype == RPE_BF16) hipLaunchKernelGGL((tensor_add_kernel<bf16>), dim3(g), dim3(256), 0, (hipStream_t)stream, (bf16*)dst, (const bf16*)src, n / ce);
    else if (dtype == RPE_F16) hipLaunchKernelGGL((tensor_add_kernel<f16>), dim3(g), dim3(256), 0, (hipStream_t)stream, (f16*)dst, (const f16*)src, n / ce);
    else return rpe_set_error(RPE_ERR_DTYPE, "tensor_add: unsupported dtype");
    RPE_CHECK_LAUNCH();
    return 0;
}

static int hook_shape_ok(int dtype, int C, int H, int W) {
    const int ce = dtype == RPE_F32 ? 4 : 8;
    if (C < ce || (C % ce) || C > 1024 || H < 2 || W < 2) return 0;
    const int cpp = C / ce;
    return (cpp & (cpp - 1)) == 0;   // lanes per pixel = min(64, chunks per pixel) must be a power of two
}

int rpe_aux_head_fwd_c(int dtype, const void* x, int C, const float* w, const float* bias, const float* depth_feat, float* out, long ld_out,
                       float* raw, unsigned char* idx, int B, int H, int W, void* stream) {
    if (!hook_shape_ok(dtype, C, H, W)) return rpe_set_error(RPE_ERR_SHAPE, "aux_head_fwd_c: C must be 16-byte chunks, a power of two of them, <= 1024");
    const long total = (long)B * (H / 2) * (W / 2);
    const int g = ew_grid(total, 4);
    if (dtype == RPE_F32) hipLaunchKernelGGL((auxc_fwd_kernel<float>), dim3(g), dim3(256), 0, (hipStream_t)stream, (const float*)x, C, w, bias, depth_feat, out, ld_out, raw, idx, B, H, W);
    else if (dtype == RPE_BF16) hipLaunchKernelGGL((auxc_fwd_kernel<bf16>), dim3(g), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, C, w, bias, depth_feat, out, ld_out, raw, idx, B, H, W);
    else if (dtype == RPE_F16) hipLaunchKernelGGL((auxc_fwd_kernel<f16>), dim3(g), dim3(256), 0, (hipStream_t)stream, (const f16*)x, C, w, bias, depth_feat, out, ld_out, raw, idx, B, H, W);
    else return rpe_set_error(RPE_ERR_DTYPE, "aux_head_fwd_c: unsupported dtype");
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_aux_head_bwd_c(int dtype, const float* dout, long ld_dout, const void* x, int C, const float* w, const float* depth_feat, const float* raw,
                       const unsigned char* idx, void* d_x, float* dw, float* dbias, float* d_depth_feat, int B, int H, int W, void* stream) {
    if (!hook_shape_ok(dtype, C, H, W) || !d_x) return rpe_set_error(RPE_ERR_SHAPE, "aux_head_bwd_c: bad shape or null gradient tensor");
    const long total = (long)B * (H / 2) * (W / 2);
    const size_t bytes = (size_t)B * H * W * C * (dtype == RPE_F32 ? 4 : 2);
    if (hipError_t he = hipMemsetAsync(d_x, 0, bytes, (hipStream_t)stream)) return rpe_set_error_hip(he, __FILE__, __LINE__);
    const int g = ew_grid(total, 4 * 8);
    const size_t sh = (size_t)(C + 1) * sizeof(float);
    if (dtype == RPE_F32) hipLaunchKernelGGL((auxc_bwd_kernel<float>), dim3(g), dim3(256), sh, (hipStream_t)stream, dout, ld_dout, (const float*)x, C, w, depth_feat, raw, idx, (float*)d_x, dw, dbias, d_depth_feat, B, H, W);
    else if (dtype == RPE_BF16) hipLaunchKernelGGL((auxc_bwd_kernel<bf16>), dim3(g), dim3(256), sh, (hipStream_t)stream, dout, ld_dout, (const bf16*)x, C, w, depth_feat, raw, idx, (bf16*)d_x, dw, dbias, d_depth_feat, B, H, W);
    else if (dtype == RPE_F16) hipLaunchKernelGGL((auxc_bwd_kernel<f16>), dim3(g), dim3(256), sh, (hipStream_t)stream, dout, ld_dout, (const f16*)x, C, w, depth_feat, raw, idx, (f16*)d_x, dw, dbias, d_depth_feat, B, H, W);
    else return rpe_set_error(RPE_ERR_DTYPE, "aux_head_bwd_c: unsupported dtype");
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_depth_head_fwd_pools(const float* depth, const float* w, const float* b, float* feat, float* xhat, int B, int H, int W, int pools, void* stream) {
    if (pools < 1 || pools > 6 || (H >> pools) < 1 || (W >> pools) < 1) return rpe_set_error(RPE_ERR_SHAPE, "depth_head_fwd_pools: 1..6 pooling steps, non-empty output");
    const size_t sh = (size_t)(H >> pools) * (W >> pools) * sizeof(float);
    hipLaunchKernelGGL(depth_pools_fwd_kernel, dim3(B), dim3(256), sh, (hipStream_t)stream, depth, w, b, feat, xhat, H, W, pools);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_depth_head_bwd(const float* d_feat, const float* xhat, long n, float* dw, float* db, void* stream) {
    hipLaunchKernelGGL(depth_bwd_kernel, dim3(ew_grid(n, 256 * 16)), dim3(256), 0, (hipStream_t)stream, d_feat, xhat, n, dw, db);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_lstm_cell_fwd(float* gates, const float* b_ih, const float* b_hh, const float* c_prev, float* c_out, float* h_out, int N, int Hd,
                      void* stream) {
    hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(ew_grid((long)N * Hd)), dim3(256), 0, (hipStream_t)stream, gates, b_ih, b_hh, c_prev, c_out, h_out, N, Hd);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_lstm_cell_bwd(const float* gates_act, const float* c_prev, const float* c_cur, const float* dh, float* dc_io, float* dgates, int N,
                      int Hd, void* stream) {
    hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(ew_grid((long)N * Hd)), dim3(256), 0, (hipStream_t)stream, gates_act, c_prev, c_cur, dh, dc_io, dgates, N, Hd);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_pose_loss(const float* pred, const float* truth, long n, int metric, int mode, float scale, float alpha, float eps, float* out3,
                  float* grad, void* stream) {
    if (metric < 0 || metric > 3 || mode < 0 || mode > 1) return rpe_set_error(RPE_ERR_SHAPE, "pose_loss: invalid metric/mode");
    if (n <= 0) return rpe_set_error(RPE_ERR_SHAPE, "pose_loss: empty batch");
    hipLaunchKernelGGL(pose_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, pred, truth, n, metric, mode, scale, alpha, eps, out3, grad);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_pose_loss_masked(const float* pred, const float* truth, const unsigned char* valid, long n, int metric, int mode, float scale, float alpha,
                         float eps, float* out3, float* grad, void* stream) {
    if (metric < 0 || metric > 3 || mode < 0 || mode > 1) return rpe_set_error(RPE_ERR_SHAPE, "pose_loss_masked: invalid metric/mode");
    if (n <= 0) return rpe_set_error(RPE_ERR_SHAPE, "pose_loss_masked: empty batch");
    if (!pred || !truth || !valid || !out3) return rpe_set_error(RPE_ERR_SHAPE, "pose_loss_masked: pred, truth, valid and out3 are required");
    hipLaunchKernelGGL(pose_loss_masked_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, pred, truth, valid, n, metric, mode, scale, alpha, eps, out3,
                       grad);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_pose_errors(const float* pred, const float* truth, long n, float eps, float* pos_err, float* ori_err, float* pose_unit, void* stream) {
    if (n <= 0) return rpe_set_error(RPE_ERR_SHAPE, "pose_errors: empty batch");
    if (!pred || !truth || !pos_err || !ori_err) return rpe_set_error(RPE_ERR_SHAPE, "pose_errors: pred, truth, pos_err and ori_err are required");
    hipLaunchKernelGGL(pose_errors_kernel, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, pred, truth, n, eps, pos_err, ori_err, pose_unit);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_error_stats(const float* err, int E, int T, double* out, void* stream) {
    if (E <= 0 || T <= 0) return rpe_set_error(RPE_ERR_SHAPE, "error_stats: E and T must be positive");
    if (!err || !out) return rpe_set_error(RPE_ERR_SHAPE, "error_stats: err and out are required");
    hipLaunchKernelGGL(error_stats_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, err, E, T, out);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_error_stats_ragged(const float* err, int E, int T, const int* lengths, double* out, void* stream) {
    if (E <= 0 || T <= 0) return rpe_set_error(RPE_ERR_SHAPE, "error_stats_ragged: E and T must be positive");
    if (!err || !lengths || !out) return rpe_set_error(RPE_ERR_SHAPE, "error_stats_ragged: err, lengths and out are required");
    hipLaunchKernelGGL(error_stats_ragged_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, err, E, T, lengths, out);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_adam_step(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2, double eps, int step, void* stream) {
    if (n <= 0) return 0;
    if ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) return rpe_set_error(RPE_ERR_ALIGN, "adam: buffers must be 16-byte aligned");
    // scalars in double, as torch.optim.Adam computes them on the host (1 - 0.999f != 0.001f)
    const double b1d = beta1, b2d = beta2;
    const float bc1 = (float)(1.0 - pow(b1d, (double)step));
    const float bc2s = (float)sqrt(1.0 - pow(b2d, (double)step));
    hipLaunchKernelGGL(adam_kernel, dim3(ew_grid(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, (float)lr, (float)(1.0 - b1d),
                       (float)beta2, (float)(1.0 - b2d), (float)eps, bc1, bc2s);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_amp_unscale(float* grads, long n, float* state, void* stream) {
    if (n <= 0) return 0;
    if (!grads || !state || (((uintptr_t)grads) & 15)) return rpe_set_error(RPE_ERR_ALIGN, "amp_unscale: gradient buffer must be 16-byte aligned");
    hipLaunchKernelGGL(amp_unscale_kernel, dim3(ew_grid(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, grads, n, state);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_amp_update(float* state, float growth_factor, float backoff_factor, int growth_interval, void* stream) {
    if (!state || growth_interval <= 0) return rpe_set_error(RPE_ERR_SHAPE, "amp_update: bad arguments");
    hipLaunchKernelGGL(amp_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, growth_factor, backoff_factor, growth_interval);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_adam_step_amp(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2, double eps, const float* state,
                      void* stream) {
    if (n <= 0) return 0;
    if (!state) return rpe_set_error(RPE_ERR_SHAPE, "adam_step_amp: null state");
    hipLaunchKernelGGL(adam_amp_kernel, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, (float)lr, beta1, beta2, (float)eps, state);
    RPE_CHECK_LAUNCH();
    return 0;
}

long rpe_grad_sumsq_rows(long n) { return grad_sumsq_rows(n); }

int rpe_grad_sumsq(const float* g, long n, double* partials, void* stream) {
    if (n <= 0 || !g || !partials) return rpe_set_error(RPE_ERR_SHAPE, "grad_sumsq: n >= 1, g and partials are required");
    if ((((uintptr_t)g) & 15) || (((uintptr_t)partials) & 7)) return rpe_set_error(RPE_ERR_ALIGN, "grad_sumsq: g must be 16-byte aligned, partials 8-byte");
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)grad_sumsq_rows(n)), dim3(256), 0, (hipStream_t)stream, g, n, partials);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_clip_coef(const double* partials, long rows, double max_norm, float* state, void* stream) {
    if (!state || rows < 0 || (rows > 0 && !partials)) return rpe_set_error(RPE_ERR_SHAPE, "clip_coef: bad arguments");
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, rows, max_norm, state);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_adamw_step_clip(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2, double eps,
                        double weight_decay, const float* state, int use_clip, void* stream) {
    if (n <= 0) return 0;
    if (!state) return rpe_set_error(RPE_ERR_SHAPE, "adamw_step_clip: null state");
    if ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) return rpe_set_error(RPE_ERR_ALIGN, "adamw_step_clip: buffers must be 16-byte aligned");
    hipLaunchKernelGGL(adamw_clip_kernel, dim3(ew_grid(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, (float)lr, beta1, beta2, (float)eps,
                       (float)(1.0 - lr * weight_decay), state, use_clip);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_lr_schedule(const float* state, int kind, long warmup_steps, double warmup_start_factor, long total_steps, double min_factor,
                    long step_size, double gamma, float* sched, void* stream) {
    if (!state || !sched) return rpe_set_error(RPE_ERR_SHAPE, "lr_schedule: null state or sched");
    if (kind != kSchedConstant && kind != kSchedCosine && kind != kSchedStep) return rpe_set_error(RPE_ERR_SHAPE, "lr_schedule: kind must be 0 (constant), 1 (cosine) or 2 (step)");
    if (warmup_steps < 0) return rpe_set_error(RPE_ERR_SHAPE, "lr_schedule: warmup_steps >= 0");
    if (!(warmup_start_factor >= 0.0 && warmup_start_factor <= 1.0)) return rpe_set_error(RPE_ERR_SHAPE, "lr_schedule: warmup_start_factor in [0, 1]");
    if (!(min_factor >= 0.0 && min_factor <= 1.0)) return rpe_set_error(RPE_ERR_SHAPE, "lr_schedule: min_factor in [0, 1]");
    if (kind == kSchedCosine && total_steps <= warmup_steps) return rpe_set_error(RPE_ERR_SHAPE, "lr_schedule: cosine needs total_steps > warmup_steps");
    if (step_size < 1) return rpe_set_error(RPE_ERR_SHAPE, "lr_schedule: step_size >= 1");
    if (!(gamma > 0.0 && gamma <= 1.0)) return rpe_set_error(RPE_ERR_SHAPE, "lr_schedule: gamma in (0, 1]");
    hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, kind, warmup_steps, warmup_start_factor, total_steps,
                       min_factor, step_size, gamma, sched);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_adamw_step_sched(float* p, const float* g, float* m, float* v, float* ema, long n, double lr, double beta1, double beta2, double eps,
                         double weight_decay, double ema_decay, const float* state, const float* sched, int use_clip, void* stream) {
    if (n <= 0) return 0;
    if (!state || !sched) return rpe_set_error(RPE_ERR_SHAPE, "adamw_step_sched: null state or sched");
    if (ema && !(ema_decay >= 0.0 && ema_decay < 1.0)) return rpe_set_error(RPE_ERR_SHAPE, "adamw_step_sched: ema_decay in [0, 1)");
    if ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v) | ((uintptr_t)ema)) & 15)
        return rpe_set_error(RPE_ERR_ALIGN, "adamw_step_sched: buffers must be 16-byte aligned");
    const dim3 grid(ew_grid(n / 4 + 1));
    if (ema)
        hipLaunchKernelGGL((adamw_sched_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, n, lr, beta1, beta2, (float)eps, weight_decay,
                           (float)(1.0 - ema_decay), state, sched, use_clip);
    else
        hipLaunchKernelGGL((adamw_sched_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, n, lr, beta1, beta2, (float)eps, weight_decay,
                           0.f, state, sched, use_clip);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_swap_f32(float* a, float* b, long n, void* stream) {
    if (n <= 0) return 0;
    if (!a || !b) return rpe_set_error(RPE_ERR_SHAPE, "swap_f32: null buffer");
    if ((((uintptr_t)a) | ((uintptr_t)b)) & 15) return rpe_set_error(RPE_ERR_ALIGN, "swap_f32: buffers must be 16-byte aligned");
    if (a < b + n && b < a + n) return rpe_set_error(RPE_ERR_SHAPE, "swap_f32: the buffers overlap");
    hipLaunchKernelGGL(swap_f32_kernel, dim3(ew_grid(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, a, b, n);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_pack_conv_weight(int dtype, const float* w_krsc, void* w_fwd, void* w_dgrad, int Co, int R, int S, int Ci, void* stream) {
    const long n = (long)Co * R * S * Ci;
    if (dtype == RPE_F32) hipLaunchKernelGGL((pack_conv_weight_kernel<float>), dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, w_krsc, (float*)w_fwd, (float*)w_dgrad, Co, R * S, Ci);
    else if (dtype == RPE_BF16) hipLaunchKernelGGL((pack_conv_weight_kernel<bf16>), dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, w_krsc, (bf16*)w_fwd, (bf16*)w_dgrad, Co, R * S, Ci);
    else if (dtype == RPE_F16) hipLaunchKernelGGL((pack_conv_weight_kernel<f16>), dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, w_krsc, (f16*)w_fwd, (f16*)w_dgrad, Co, R * S, Ci);
    else return rpe_set_error(RPE_ERR_DTYPE, "pack_conv_weight: unsupported dtype");
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_pack_conv_weights_multi(int dtype, const rpe_pack_desc* table_dev, int nlayers, long total, void* stream) {
    note_kernel("pack_conv_weights_multi_kernel");
    if (nlayers <= 0 || nlayers > kPackMaxLayers || total <= 0) return rpe_set_error(RPE_ERR_SHAPE, "pack_conv_weights_multi: bad table (1..255 layers)");
    const int grid = (int)((total + 4095) / 4096 < 8192 ? (total + 4095) / 4096 : 8192);
    if (dtype == RPE_F32) hipLaunchKernelGGL((pack_conv_weights_multi_kernel<float>), dim3(grid), dim3(256), 0, (hipStream_t)stream, table_dev, nlayers, total);
    else if (dtype == RPE_BF16) hipLaunchKernelGGL((pack_conv_weights_multi_kernel<bf16>), dim3(grid), dim3(256), 0, (hipStream_t)stream, table_dev, nlayers, total);
    else if (dtype == RPE_F16) hipLaunchKernelGGL((pack_conv_weights_multi_kernel<f16>), dim3(grid), dim3(256), 0, (hipStream_t)stream, table_dev, nlayers, total);
    else return rpe_set_error(RPE_ERR_DTYPE, "pack_conv_weights_multi: unsupported dtype");
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_pack_stem_weight(int dtype, const float* w_oihw, const float* scale, void* out, void* stream) {
    note_kernel("pack_stem_weight_kernel");
    if (dtype == RPE_F32) hipLaunchKernelGGL((pack_stem_weight_kernel<float>), dim3(64), dim3(256), 0, (hipStream_t)stream, w_oihw, scale, (float*)out);
    else if (dtype == RPE_BF16) hipLaunchKernelGGL((pack_stem_weight_kernel<bf16>), dim3(64), dim3(256), 0, (hipStream_t)stream, w_oihw, scale, (bf16*)out);
    else if (dtype == RPE_F16) hipLaunchKernelGGL((pack_stem_weight_kernel<f16>), dim3(64), dim3(256), 0, (hipStream_t)stream, w_oihw, scale, (f16*)out);
    else return rpe_set_error(RPE_ERR_DTYPE, "pack_stem_weight: unsupported dtype");
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_unpack_stem_grad(const float* d_packed, float* dw_oihw, void* stream) {
    hipLaunchKernelGGL(unpack_stem_grad_kernel, dim3((64 * 147 + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_packed, dw_oihw);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_transpose_f32(const float* in, float* out, int rows, int cols, int ldi, int ldo, void* stream) {
    hipLaunchKernelGGL(transpose_f32_kernel, dim3((cols + 31) / 32, (ldo + 31) / 32), dim3(256), 0, (hipStream_t)stream, in, out, rows, cols, ldi, ldo);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_relu_bwd(const float* out, const float* dy, float* dx, long n, void* stream) {
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, out, dy, dx, n);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_colsum(const float* x, long rows, int cols, int ld, float* out, int accumulate, void* stream) {
    hipLaunchKernelGGL(colsum_kernel, dim3((cols + 31) / 32), dim3(256), 0, (hipStream_t)stream, x, rows, cols, ld, out, accumulate);
    RPE_CHECK_LAUNCH();
    return 0;
}

int rpe_copy2d(const float* src, int ld_src, float* dst, int ld_dst, long rows, int cols, void* stream) {
    hipLaunchKernelGGL(copy2d_kernel, dim3(ew_grid(rows * cols)), dim3(256), 0, (hipStream_t)stream, src, ld_src, dst, ld_dst, rows, cols);
    RPE_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
