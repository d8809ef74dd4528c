// Layer-activation capture (util/model_utils.py: capture_layer / render_layer / visualize_layer).
//   feature_planes_kernel : NHWC activations in the compute dtype -> (C, H, W) fp32 planes + per-channel min / max over finite values
//   feature_mosaic_kernel : planes + ranges -> one uint8 colour-INDEX image, a grid of per-channel autoscaled tiles
// Both are exact: the widening has no rounding, and the mosaic is one correctly rounded fp32 operation per step.
#include "common.h"
#include "minmax.h"

namespace rpe {

constexpr int kPlaneTP = 64;             // pixels per tile: one wave writes one 256-byte run of a plane
constexpr int kPlaneTC = 32;             // channels per tile
constexpr int kPlanePitch = kPlaneTP + 1;   // LDS row pitch in dwords: the transposing writes of a 32-lane half land on 32 different banks

// (finite_f, atomic_min_f, atomic_max_f: minmax.h)

__global__ void __launch_bounds__(256) minmax_init_kernel(float* minmax, long n_channels) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n_channels) {
        minmax[2 * i] = __uint_as_float(0x7f800000u);
        minmax[2 * i + 1] = __uint_as_float(0xff800000u);
    }
}

// grid (pixel tiles, channel tiles, images).  Read: 16-byte chunks along C (lanes of one pixel are adjacent: CPP x 16 contiguous
// bytes), widened into a padded LDS tile [channel][pixel].  Write: wave w takes channels w, w + 4, ..; lane = pixel, so every store
// instruction is one contiguous run of a plane.  The tile's per-channel range is reduced across the wave and merged with two atomics.
template <typename T, bool kVec>
__global__ void __launch_bounds__(256) feature_planes_kernel(const T* __restrict__ x, float* __restrict__ out, float* __restrict__ minmax, int HW, int C) {
    constexpr int K = Elem<T>::kChunk;
    constexpr int CPP = kPlaneTC / K;   // chunks per pixel inside a tile
    __shared__ float tile[kPlaneTC][kPlanePitch];
    const int p0 = blockIdx.x * kPlaneTP, c0 = blockIdx.y * kPlaneTC;
    const long img = blockIdx.z;
    const T* xi = x + img * (long)HW * C;
    if (kVec) {
        for (int i = threadIdx.x; i < kPlaneTP * CPP; i += 256) {
            const int p = i / CPP, q = i % CPP;
            const int c = c0 + q * K;
            float f[K];
            if (p0 + p < HW && c < C) {   // (C is a whole number of chunks here: a chunk is inside or outside as a whole)
                const u32x4 v = *reinterpret_cast<const u32x4*>(xi + (long)(p0 + p) * C + c);
                chunk_to_f<T>(v, f);
            } else {
#pragma unroll
                for (int j = 0; j < K; ++j) f[j] = 0.f;
            }
#pragma unroll
            for (int j = 0; j < K; ++j) tile[q * K + j][p] = f[j];
        }
    } else {   // any C (the heads' single-channel maps): element loads
        for (int i = threadIdx.x; i < kPlaneTP * kPlaneTC; i += 256) {
            const int p = i / kPlaneTC, cc = i % kPlaneTC;
            float f = 0.f;
            if (p0 + p < HW && c0 + cc < C) f = Elem<T>::to_f(xi[(long)(p0 + p) * C + c0 + cc]);
            tile[cc][p] = f;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool in = p0 + lane < HW;
    for (int cc = wave; cc < kPlaneTC; cc += 4) {
        const int c = c0 + cc;
        if (c >= C) break;   // (uniform across the wave)
        const float v = tile[cc][lane];
        if (in) out[(img * C + c) * (long)HW + p0 + lane] = v;
        const bool ok = in && finite_f(v);
        float lo = ok ? v : __uint_as_float(0x7f800000u), hi = ok ? v : __uint_as_float(0xff800000u);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, o));
            hi = fmaxf(hi, __shfl_xor(hi, o));
        }
        if (lane == 0 && lo <= hi) {   // (a tile without a finite value contributes nothing)
            // fminf / fmaxf may return either zero of a (-0, +0) pair; the atomics below settle the sign (see atomic_min_f)
            atomic_min_f(minmax + 2 * (img * C + c), lo);
            atomic_max_f(minmax + 2 * (img * C + c) + 1, hi);
        }
    }
}

// one thread per pixel of the index image
__global__ void __launch_bounds__(256) feature_mosaic_kernel(const float* __restrict__ planes, const float* __restrict__ minmax, int C, int H, int W, int cols,
                                                            int gutter, int flip_y, int OH, int OW, unsigned char* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)OH * OW) return;
    const int oy = (int)(i / OW), ox = (int)(i % OW);
    const int ph = H + gutter, pw = W + gutter;
    const int tr = oy / ph, r = oy % ph, tc = ox / pw, q = ox % pw;
    const int c = tr * cols + tc;
    unsigned char idx = 0;
    if (r < H && q < W && c < C) {
        const float lo = minmax[2 * c], hi = minmax[2 * c + 1];
        const float v = planes[((long)c * H + (flip_y ? H - 1 - r : r)) * W + q];
        if (finite_f(v) && hi != lo) {   // (an all-NaN channel keeps lo = +inf, hi = -inf, and has no finite pixel)
            // matplotlib's Normalize + 256-entry lookup, one correctly rounded fp32 operation each (t * 256 is exact)
            const float t = __fdiv_rn(__fsub_rn(v, lo), __fsub_rn(hi, lo));
            const int k = (int)__fmul_rn(t, 256.0f);
            idx = (unsigned char)(k > 255 ? 255 : k);
        }
    }
    out[i] = idx;
}

template <typename T>
static int planes_launch(const void* x, int B, int HW, int C, float* out, float* minmax, hipStream_t s) {
    const dim3 grid((HW + kPlaneTP - 1) / kPlaneTP, (C + kPlaneTC - 1) / kPlaneTC, B);
    const bool vec = (C % Elem<T>::kChunk) == 0 && (((uintptr_t)x) & 15) == 0;
    if (vec) hipLaunchKernelGGL((feature_planes_kernel<T, true>), grid, dim3(256), 0, s, (const T*)x, out, minmax, HW, C);
    else hipLaunchKernelGGL((feature_planes_kernel<T, false>), grid, dim3(256), 0, s, (const T*)x, out, minmax, HW, C);
    return 0;
}

}  // namespace rpe

using namespace rpe;

extern "C" int rpe_feature_planes_batch(int dtype, const void* x_nhwc, int B, int H, int W, int C, float* out_bchw_f32, float* minmax, void* stream) {
    if (!x_nhwc || !out_bchw_f32 || !minmax) return rpe_set_error(RPE_ERR_SHAPE, "feature_planes: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || B > 65535 || (long)H * W > (1L << 24) || C > 65535 * kPlaneTC)
        return rpe_set_error(RPE_ERR_SHAPE, "feature_planes: B, H, W, C must be positive (B <= 65535, H*W <= 2^24)");
    if (dtype != RPE_F32 && dtype != RPE_BF16 && dtype != RPE_F16) return rpe_set_error(RPE_ERR_DTYPE, "feature_planes: unsupported dtype");
    const long nch = (long)B * C;
    note_kernel("minmax_init_kernel");
    hipLaunchKernelGGL(minmax_init_kernel, dim3((unsigned)((nch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, minmax, nch);
    RPE_CHECK_LAUNCH();
    prof_split((hipStream_t)stream, "feature_planes_kernel");
    if (dtype == RPE_F32) planes_launch<float>(x_nhwc, B, H * W, C, out_bchw_f32, minmax, (hipStream_t)stream);
    else if (dtype == RPE_BF16) planes_launch<bf16>(x_nhwc, B, H * W, C, out_bchw_f32, minmax, (hipStream_t)stream);
    else planes_launch<f16>(x_nhwc, B, H * W, C, out_bchw_f32, minmax, (hipStream_t)stream);
    RPE_CHECK_LAUNCH();
    return 0;
}

extern "C" int rpe_feature_planes(int dtype, const void* x_nhwc, int image, int H, int W, int C, float* out_chw_f32, float* minmax, void* stream) {
    if (!x_nhwc || image < 0 || H <= 0 || W <= 0 || C <= 0) return rpe_set_error(RPE_ERR_SHAPE, "feature_planes: bad image index or shape");
    const size_t esz = dtype == RPE_F32 ? 4 : 2;
    return rpe_feature_planes_batch(dtype, (const char*)x_nhwc + (size_t)image * H * W * C * esz, 1, H, W, C, out_chw_f32, minmax, stream);
}

extern "C" int rpe_feature_mosaic(const float* planes, const float* minmax, int C, int H, int W, int cols, int gutter, int flip_y, unsigned char* out_u8,
                                  void* stream) {
    if (!planes || !minmax || !out_u8) return rpe_set_error(RPE_ERR_SHAPE, "feature_mosaic: null pointer");
    if (C <= 0 || H <= 0 || W <= 0 || cols <= 0 || gutter < 0) return rpe_set_error(RPE_ERR_SHAPE, "feature_mosaic: C, H, W, cols must be positive, gutter >= 0");
    const long rows = (C + cols - 1) / cols;
    const long OH = rows * (H + gutter) - gutter, OW = (long)cols * (W + gutter) - gutter;
    if (OH > (1 << 20) || OW > (1 << 20) || OH * OW > (1L << 31)) return rpe_set_error(RPE_ERR_SHAPE, "feature_mosaic: index image too large");
    note_kernel("feature_mosaic_kernel");
    hipLaunchKernelGGL(feature_mosaic_kernel, dim3((unsigned)((OH * OW + 255) / 256)), dim3(256), 0, (hipStream_t)stream, planes, minmax, C, H, W, cols, gutter,
                       flip_y != 0, (int)OH, (int)OW, out_u8);
    RPE_CHECK_LAUNCH();
    return 0;
}
