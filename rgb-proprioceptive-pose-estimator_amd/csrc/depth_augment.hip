// Depth-sensor augmentation of raw fp32 depth frames on the device (ops.augment_depth_f32, util.data_utils.DepthAugment):
// range-dependent noise, quantisation, clamp, pixel dropout, hole rectangles and the occluder shared with the RGB frames,
// float32 [B][Hs][Ws] -> float32 of the same shape, run IN FRONT of rpe_stage_depth_f32_resized, which stays as it is.  DESIGN.md
// "Depth augmentation" has the specification; tests/_depth_augment_oracle.py restates it in numpy fp64 and the kernels are compared
// with it bit pattern for bit pattern.
//   depth_augment_params_kernel : reads the step counter state[0], draws every stream's hole count and four rectangles into `params`,
//                                 advances the counter -- the only reader and writer of `state`, so a captured launch draws fresh
//                                 numbers at every replay
//   depth_augment_apply_kernel  : the six stages per pixel
// Stages 1-3 are fp64 from the input pixel with ONE rounding to fp32 at the store, and use only +, *, rint, comparisons and integer
// operations: no division, logarithm, cosine or square root (the host folds 1 / sqrt(Var T) into n0..n2 and hands 1 / q over).
// Contraction to fused multiply-adds is off for this file (depth_stage.hip records why __dmul_rn / __dadd_rn do not help), so every
// product and every sum is its own correctly rounded operation.  Random numbers: Philox4x32-10 keyed by the seed, counter
// (a, b, step, purpose) with three purposes of this file's own.
// The apply kernel walks the batch as ONE flat array of B * P pixels: a thread takes 4 consecutive pixels = one 16-byte load and one
// 16-byte store (a frame boundary may fall inside a group; the stream's rectangles are re-read there), and the last (B * P) % 4 pixels
// -- or all of them when a pointer is not 16-byte aligned -- go one per thread.
#include "common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace rpe {

static_assert(sizeof(rpe_depth_augment_desc) == 104, "rpe_depth_augment_desc: _lib.DepthAugmentDesc mirrors this layout");

constexpr unsigned kDepthCountPurpose = 0x44455048u;   // "DEPH": a stream's number of holes
constexpr unsigned kDepthRectPurpose = 0x44455052u;    // "DEPR": one hole rectangle of a stream
constexpr unsigned kDepthPixelPurpose = 0x44455058u;   // "DEPX": a pixel's noise and dropout words
constexpr int kDepthRow = 17;                          // ints per stream in `params`: count, 4 x (top, left, h, w)

// bounded draw over n values: (r * n) >> 32
__device__ inline int ddraw(unsigned r, unsigned n) { return (int)__umulhi(r, n); }

// one block; G streams
__global__ void __launch_bounds__(256) depth_augment_params_kernel(unsigned* __restrict__ state, int* __restrict__ params, int G, int Hs, int Ws,
                                                                  rpe_depth_augment_desc d) {
    const unsigned step = state[0];
    __syncthreads();   // every thread has read the counter before it moves
    const unsigned k0 = (unsigned)d.seed, k1 = (unsigned)(d.seed >> 32);
    for (int g = threadIdx.x; g < G; g += 256) {
        unsigned r[4];
        int* q = params + 1 + kDepthRow * g;
        philox4x32_10((unsigned)g, 0u, step, kDepthCountPurpose, k0, k1, r);
        q[0] = d.hole_lo + ddraw(r[0], (unsigned)(d.hole_hi - d.hole_lo + 1));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            philox4x32_10((unsigned)g, (unsigned)j, step, kDepthRectPurpose, k0, k1, r);
            const int h = d.hh_lo + ddraw(r[0], (unsigned)(d.hh_hi - d.hh_lo + 1));
            const int w = d.hw_lo + ddraw(r[1], (unsigned)(d.hw_hi - d.hw_lo + 1));
            q[1 + 4 * j] = ddraw(r[2], (unsigned)(Hs - h + 1));
            q[2 + 4 * j] = ddraw(r[3], (unsigned)(Ws - w + 1));
            q[3 + 4 * j] = h;
            q[4 + 4 * j] = w;
        }
    }
    if (threadIdx.x == 0) {
        params[0] = (int)step;
        state[0] = step + 1u;   // wraps at 2^32
    }
}

// what the apply kernel needs to know besides the descriptor: which stages are on (decided once, on the host)
struct DepthStages {
    int noise, quant, clamp, drop, holes, occl;
};

// the rectangles of one stream: its holes and, with a shared occluder, the RGB table's rectangle
struct DepthRects {
    int count, top[4], left[4], h[4], w[4];
    int erase, etop, eleft, eh, ew;
};
__device__ inline int depth_stream_of(int b, int group) { return group > 0 ? b % group : b; }
__device__ inline DepthRects depth_rects(const int* __restrict__ params, const int* __restrict__ rgb_params, const DepthStages& st, int group, int b) {
    DepthRects f;
    const int g = depth_stream_of(b, group);
    f.count = 0;
    f.erase = 0;
    if (st.holes) {
        const int* q = params + 1 + kDepthRow * g;
        f.count = q[0];
#pragma unroll
        for (int j = 0; j < 4; ++j) { f.top[j] = q[1 + 4 * j]; f.left[j] = q[2 + 4 * j]; f.h[j] = q[3 + 4 * j]; f.w[j] = q[4 + 4 * j]; }
    }
    if (st.occl) {
        const int* q = rgb_params + 1 + 8 * g;   // rpe_augment_frames_u8's row: qb qc qs erase top left h w
        f.erase = q[3]; f.etop = q[4]; f.eleft = q[5]; f.eh = q[6]; f.ew = q[7];
    }
    return f;
}

// one pixel: bit pattern in -> bit pattern out
__device__ inline unsigned depth_pixel(unsigned bits, unsigned p, int b, int y, int x, unsigned step, unsigned k0, unsigned k1, const DepthRects& f,
                                       const DepthStages& st, const rpe_depth_augment_desc& d) {
    unsigned r[4] = {0u, 0u, 0u, 0u};
    if (st.noise || st.drop) philox4x32_10(p, (unsigned)b, step, kDepthPixelPurpose, k0, k1, r);
    unsigned o = bits;
    const float din = __uint_as_float(bits);
    if ((st.noise || st.quant || st.clamp) && (bits & 0x7f800000u) != 0x7f800000u) {   // a non-finite input keeps its bit pattern
        const double dd = (double)din;
        double v = dd;
        if (st.noise) {
            const int hsum = (int)((r[0] & 0xffffu) + (r[0] >> 16) + (r[1] & 0xffffu) + (r[1] >> 16) + (r[2] & 0xffffu) + (r[2] >> 16));
            const int T = 2 * hsum - 6 * 65535;
            const double sd = (d.n0 + d.n1 * dd) + (d.n2 * dd) * dd;
            v = dd + sd * (double)T;
        }
        if (st.quant) v = rint(v * d.inv_q) * d.q;
        if (st.clamp) {   // max(v, lo) then min(., hi), written as selects: a signed zero equal to a bound stays as it is
            v = v < d.lo ? d.lo : v;
            v = v > d.hi ? d.hi : v;
        }
        o = __float_as_uint((float)v);
    }
    if (st.drop && r[3] < d.drop_thresh) o = __float_as_uint(d.hole_value);
    bool hole = false;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        hole = hole || (j < f.count && y >= f.top[j] && y < f.top[j] + f.h[j] && x >= f.left[j] && x < f.left[j] + f.w[j]);
    if (hole) o = __float_as_uint(d.hole_value);
    if (f.erase && y >= f.etop && y < f.etop + f.eh && x >= f.eleft && x < f.eleft + f.ew) o = __float_as_uint(d.occluder_value);
    return o;
}

// flat pixel index -> (frame, pixel in the frame); 32-bit division while the index allows it
__device__ inline void depth_split_pixel(long first, unsigned P, int& b, unsigned& p) {
    if (first <= 0xffffffffL) {
        const unsigned q = (unsigned)first / P;
        b = (int)q; p = (unsigned)first - q * P;
    } else {
        const long q = first / (long)P;
        b = (int)q; p = (unsigned)(first - q * (long)P);
    }
}

template <int N> __device__ inline void depth_apply_pixels(const float* in, float* out, long first, unsigned P, int Ws, int group, const int* __restrict__ params,
                                                           const int* __restrict__ rgb_params, const DepthStages& st, const rpe_depth_augment_desc& d) {
    unsigned w[4];
    if (N == 4) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(in + first);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
        w[0] = __float_as_uint(in[first]);
    }
    int b;
    unsigned p;
    depth_split_pixel(first, P, b, p);
    int y = (int)(p / (unsigned)Ws), x = (int)(p - (unsigned)y * (unsigned)Ws);
    const unsigned step = (unsigned)params[0], k0 = (unsigned)d.seed, k1 = (unsigned)(d.seed >> 32);
    DepthRects f = depth_rects(params, rgb_params, st, group, b);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        w[j] = depth_pixel(w[j], p, b, y, x, step, k0, k1, f, st, d);
        if (N > 1 && j + 1 < N) {
            if (++x == Ws) { x = 0; ++y; }
            if (++p == P) {   // the next pixel opens the next frame (first + N <= B P: it exists)
                p = 0; y = 0; ++b;
                f = depth_rects(params, rgb_params, st, group, b);
            }
        }
    }
    if (N == 4) {
        u32x4 t; t.x = w[0]; t.y = w[1]; t.z = w[2]; t.w = w[3];
        *reinterpret_cast<u32x4*>(out + first) = t;
    } else {
        out[first] = __uint_as_float(w[0]);
    }
}

// in and out may be the same buffer (no __restrict__ on either): a thread reads all of its pixels before it writes them, and no
// thread reads another's
__global__ void __launch_bounds__(256) depth_augment_apply_kernel(const float* in, float* out, long nvec, long npix, unsigned P, int Ws, int group,
                                                                 const int* __restrict__ params, const int* __restrict__ rgb_params, DepthStages st,
                                                                 rpe_depth_augment_desc d) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const bool vec = i < nvec;
    const long first = vec ? i * 4 : nvec * 4 + (i - nvec);
    if (first >= npix) return;
    if (vec) depth_apply_pixels<4>(in, out, first, P, Ws, group, params, rgb_params, st, d);
    else depth_apply_pixels<1>(in, out, first, P, Ws, group, params, rgb_params, st, d);
}

}  // namespace rpe

using namespace rpe;

static bool coef_ok(double v) { return v >= 0.0 && !std::isinf(v); }   // false for a NaN as well

extern "C" int rpe_augment_depth_f32(const float* in, float* out, int B, int Hs, int Ws, const rpe_depth_augment_desc* d, unsigned* state, int* params,
                                     const int* rgb_params, int rgb_group, void* stream) {
    if (!in || !out || !d || !state || !params) return rpe_set_error(RPE_ERR_SHAPE, "augment_depth_f32: null pointer");
    if (B <= 0 || Hs <= 0 || Ws <= 0 || (long)Hs * Ws >= (1L << 32)) return rpe_set_error(RPE_ERR_SHAPE, "augment_depth_f32: bad shape (Hs * Ws must be below 2^32)");
    if (!coef_ok(d->n0) || !coef_ok(d->n1) || !coef_ok(d->n2)) return rpe_set_error(RPE_ERR_SHAPE, "augment_depth_f32: a noise coefficient must be finite and not negative");
    if (!coef_ok(d->q) || !coef_ok(d->inv_q)) return rpe_set_error(RPE_ERR_SHAPE, "augment_depth_f32: q and inv_q must be finite and not negative");
    if (!(d->lo <= d->hi)) return rpe_set_error(RPE_ERR_SHAPE, "augment_depth_f32: the clamp range needs lo <= hi, neither a NaN");
    if (d->hole_lo < 0 || d->hole_lo > d->hole_hi || d->hole_hi > 4) return rpe_set_error(RPE_ERR_SHAPE, "augment_depth_f32: the hole count needs 0 <= lo <= hi <= 4");
    if (d->hole_hi > 0 && (d->hh_lo < 1 || d->hh_lo > d->hh_hi || d->hh_hi > Hs || d->hw_lo < 1 || d->hw_lo > d->hw_hi || d->hw_hi > Ws))
        return rpe_set_error(RPE_ERR_SHAPE, "augment_depth_f32: the rectangle bounds need 1 <= lo <= hi <= Hs / Ws");
    if (d->group < 0) return rpe_set_error(RPE_ERR_SHAPE, "augment_depth_f32: group must not be negative");
    if (rgb_params && rgb_group != d->group) return rpe_set_error(RPE_ERR_SHAPE, "augment_depth_f32: the RGB table was drawn with another group");
    const long P = (long)Hs * Ws, npix = (long)B * P;
    const uintptr_t bytes = (uintptr_t)npix * 4u;
    if (in != out && (uintptr_t)in < (uintptr_t)out + bytes && (uintptr_t)out < (uintptr_t)in + bytes)
        return rpe_set_error(RPE_ERR_SHAPE, "augment_depth_f32: in and out overlap (the same buffer is allowed)");
    const bool aligned = (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
    const long nvec = aligned ? npix / 4 : 0, nthreads = nvec + (npix - nvec * 4), nblocks = (nthreads + 255) / 256;
    if (nblocks > 0x7fffffffL) return rpe_set_error(RPE_ERR_SHAPE, "augment_depth_f32: too many pixels for one launch");
    const int G = d->group > 0 ? d->group : B;
    DepthStages st;
    st.noise = d->n0 != 0.0 || d->n1 != 0.0 || d->n2 != 0.0;
    st.quant = d->q > 0.0;
    st.clamp = !(std::isinf(d->lo) && d->lo < 0.0 && std::isinf(d->hi) && d->hi > 0.0);
    st.drop = d->drop_thresh != 0u;
    st.holes = d->hole_hi > 0;
    st.occl = rgb_params != nullptr;
    hipStream_t s = (hipStream_t)stream;
    note_kernel("depth_augment_params_kernel");
    hipLaunchKernelGGL(depth_augment_params_kernel, dim3(1), dim3(256), 0, s, state, params, G, Hs, Ws, *d);
    RPE_CHECK_LAUNCH();
    prof_split(s, "depth_augment_apply_kernel");
    hipLaunchKernelGGL(depth_augment_apply_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, in, out, nvec, npix, (unsigned)P, Ws, d->group, (const int*)params,
                       rgb_params, st, *d);
    RPE_CHECK_LAUNCH();
    return 0;
}
