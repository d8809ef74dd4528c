// Label-preserving augmentation of raw uint8 camera frames on the device (ops.augment_frames_u8, util.data_utils.FrameAugment):
// brightness / contrast / saturation jitter, sensor noise and random erasing, uint8 [B][Hs][Ws][3] -> uint8 of the same shape, run IN
// FRONT of the staging kernels (rpe_stage_frames_u8[_resized]), which stay as they are.  DESIGN.md "Frame augmentation" has the
// specification; tests/_augment_oracle.py restates it in numpy and the kernels are compared with it for equality.
//   augment_params_kernel : reads the step counter state[0], draws every stream's parameters into `params`, zeroes `sums`, advances the
//                           counter -- the only reader of `state`, so a captured launch draws fresh numbers at every replay
//   augment_sum_kernel    : sums[b] = sum over the frame of grey(brightness(v)) (the contrast stage's mean; skipped when contrast is off)
//   augment_apply_kernel  : the five stages per pixel
// All arithmetic is integer (Q16 factors, floor shifts, a clamp after every stage): the sums are exact in any order, so the result does
// not depend on the launch geometry.  Random numbers: Philox4x32-10 keyed by the seed, counter (a, b, step, purpose).
// The two pixel kernels walk the batch as ONE flat array of B * P pixels: a thread takes 16 consecutive pixels = 48 bytes = three
// 16-byte loads (the flat array keeps every such group aligned whatever the frame size; a frame boundary may fall inside a group, the
// per-frame parameters are re-read there), and the last (B * P) % 16 pixels -- or all of them when a pointer is not 16-byte aligned --
// go one per thread.
#include "common.h"

namespace rpe {

typedef unsigned long long u64;
static_assert(sizeof(rpe_augment_desc) == 72, "rpe_augment_desc: _lib.AugmentDesc mirrors this layout");

// bounded draw over n values: (r * n) >> 32
__device__ inline int draw(unsigned r, unsigned n) { return (int)__umulhi(r, n); }

__device__ inline int clamp255(int v) { return min(max(v, 0), 255); }
__device__ inline int grey(int r, int g, int b) { return (77 * r + 150 * g + 29 * b + 128) >> 8; }
__device__ inline int byte_sum(unsigned w) { return (int)((w & 255u) + ((w >> 8) & 255u) + ((w >> 16) & 255u) + (w >> 24)); }

// one block; G streams, B frames
__global__ void __launch_bounds__(256) augment_params_kernel(unsigned* __restrict__ state, int* __restrict__ params, u64* __restrict__ sums, int B, int G,
                                                            int Hs, int Ws, rpe_augment_desc d) {
    const unsigned step = state[0];
    __syncthreads();   // every thread has read the counter before it moves
    const unsigned k0 = (unsigned)d.seed, k1 = (unsigned)(d.seed >> 32);
    for (int g = threadIdx.x; g < G; g += 256) {
        unsigned r[4];
        int* q = params + 1 + 8 * g;
        philox4x32_10((unsigned)g, 0u, step, 0u, k0, k1, r);
        q[0] = d.qb_lo + draw(r[0], (unsigned)(d.qb_hi - d.qb_lo + 1));
        q[1] = d.qc_lo + draw(r[1], (unsigned)(d.qc_hi - d.qc_lo + 1));
        q[2] = d.qs_lo + draw(r[2], (unsigned)(d.qs_hi - d.qs_lo + 1));
        q[3] = r[3] < d.erase_thresh ? 1 : 0;
        philox4x32_10((unsigned)g, 0u, step, 1u, k0, k1, r);
        const int h = d.eh_lo + draw(r[0], (unsigned)(d.eh_hi - d.eh_lo + 1));
        const int w = d.ew_lo + draw(r[1], (unsigned)(d.ew_hi - d.ew_lo + 1));
        q[4] = draw(r[2], (unsigned)(Hs - h + 1));
        q[5] = draw(r[3], (unsigned)(Ws - w + 1));
        q[6] = h;
        q[7] = w;
    }
    if (sums)
        for (int b = threadIdx.x; b < B; b += 256) sums[b] = 0;
    if (threadIdx.x == 0) {
        params[0] = (int)step;
        state[0] = step + 1u;
    }
}

// the 16-pixel group / single pixel of thread i: first flat pixel, and whether it is a vector group
struct Span {
    long first;
    bool vec;
    bool any;
};
__device__ inline Span thread_span(long nvec, long npix) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    Span s;
    s.vec = i < nvec;
    s.first = s.vec ? i * 16 : nvec * 16 + (i - nvec);
    s.any = s.first < npix;
    return s;
}

template <int N> __device__ inline void load_pixels(const unsigned char* in, long first, unsigned (&w)[12]) {
    if (N == 16) {
        const u32x4* p = reinterpret_cast<const u32x4*>(in + first * 3);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const u32x4 v = p[k];
            w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
        }
    } else {
        const unsigned char* p = in + first * 3;
        w[0] = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
    }
}
__device__ inline int get_byte(const unsigned (&w)[12], int k) { return (int)((w[k >> 2] >> (8 * (k & 3))) & 255u); }

// flat pixel index -> (frame, pixel in the frame); 32-bit division while the index allows it
__device__ inline void split_pixel(long first, unsigned P, int& b, unsigned& p) {
    if (first <= 0xffffffffL) {
        const unsigned q = (unsigned)first / P;
        b = (int)q; p = (unsigned)first - q * P;
    } else {
        const long q = first / (long)P;
        b = (int)q; p = (unsigned)(first - q * (long)P);
    }
}
__device__ inline int stream_of(int b, int group) { return group > 0 ? b % group : b; }

// sum of grey(brightness(v)) over the thread's N pixels -> (b, s): the frame the thread ended in and its share of that frame's sum; a
// group that crosses a frame boundary adds the finished part to its own frame at once
template <int N> __device__ inline void sum_pixels(const unsigned char* in, long first, unsigned P, int group, const int* __restrict__ params, u64* sums,
                                                   int& b, unsigned& s) {
    unsigned w[12], p;
    load_pixels<N>(in, first, w);
    split_pixel(first, P, b, p);
    int qb = params[1 + 8 * stream_of(b, group)];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int r = clamp255((get_byte(w, 3 * j) * qb + 32768) >> 16), g = clamp255((get_byte(w, 3 * j + 1) * qb + 32768) >> 16),
                  bl = clamp255((get_byte(w, 3 * j + 2) * qb + 32768) >> 16);
        s += (unsigned)grey(r, g, bl);
        if (N > 1 && j + 1 < N && ++p == P) {   // the next pixel opens the next frame (first + N <= B P: it exists)
            atomicAdd(&sums[b], (u64)s);
            s = 0; p = 0; ++b;
            qb = params[1 + 8 * stream_of(b, group)];
        }
    }
}

__global__ void __launch_bounds__(256) augment_sum_kernel(const unsigned char* in, long nvec, long npix, unsigned P, int group, const int* __restrict__ params,
                                                         u64* sums) {
    const Span sp = thread_span(nvec, npix);
    int b = 0;
    unsigned s = 0;
    if (sp.any) {
        if (sp.vec) sum_pixels<16>(in, sp.first, P, group, params, sums, b, s);
        else sum_pixels<1>(in, sp.first, P, group, params, sums, b, s);
    }
    // every lane of the wave is here again.  One atomic per wave where its lanes ended in one frame (a lane without pixels holds 0)
    const u64 have = __ballot(sp.any);
    if (have == 0) return;
    const int b0 = __shfl(b, __ffsll((long long)have) - 1);
    if (__all(!sp.any || b == b0)) {
        unsigned t = s;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);   // at most 64 x 16 x 255: no overflow
        if ((threadIdx.x & 63) == 0) atomicAdd(&sums[b0], (u64)t);
    } else if (sp.any) {
        atomicAdd(&sums[b], (u64)s);
    }
}

struct FrameParams {
    int qb, qc, qs, erase, top, left, h, w, m;
};
__device__ inline FrameParams frame_params(const int* __restrict__ params, const u64* __restrict__ sums, unsigned P, int group, int b) {
    const int* q = params + 1 + 8 * stream_of(b, group);
    FrameParams f;
    f.qb = q[0]; f.qc = q[1]; f.qs = q[2]; f.erase = q[3]; f.top = q[4]; f.left = q[5]; f.h = q[6]; f.w = q[7];
    f.m = sums ? (int)((sums[b] + P / 2) / P) : 0;   // contrast off: qc = 65536 and m has the factor 0
    return f;
}

template <int N> __device__ inline void apply_pixels(const unsigned char* in, unsigned char* out, long first, unsigned P, int Ws, int group,
                                                     const int* __restrict__ params, const u64* __restrict__ sums, const rpe_augment_desc& d) {
    unsigned w[12], o[12];
    load_pixels<N>(in, first, w);
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = 0;
    int b;
    unsigned p;
    split_pixel(first, P, b, p);
    const unsigned step = (unsigned)params[0], k0 = (unsigned)d.seed, k1 = (unsigned)(d.seed >> 32);
    FrameParams f = frame_params(params, sums, P, group, b);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        int v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = clamp255((get_byte(w, 3 * j + c) * f.qb + 32768) >> 16);                       // brightness
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = clamp255((v[c] * f.qc + f.m * (65536 - f.qc) + 32768) >> 16);                  // contrast
        const int g = grey(v[0], v[1], v[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = clamp255((v[c] * f.qs + g * (65536 - f.qs) + 32768) >> 16);                    // saturation
        bool inside = false;
        if (f.erase) {
            const int y = (int)(p / (unsigned)Ws), x = (int)(p - (unsigned)y * (unsigned)Ws);
            inside = y >= f.top && y < f.top + f.h && x >= f.left && x < f.left + f.w;
        }
        if (d.noise_q != 0 || (inside && d.fill_mode == 1)) {
            unsigned r[4];
            philox4x32_10(p, (unsigned)b, step, 2u, k0, k1, r);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = clamp255(v[c] + (((byte_sum(r[c]) - 510) * d.noise_q + 32768) >> 16));    // noise
            if (inside && d.fill_mode == 1) { v[0] = (int)(r[3] & 255u); v[1] = (int)((r[3] >> 8) & 255u); v[2] = (int)((r[3] >> 16) & 255u); }
        }
        if (inside && d.fill_mode == 0) { v[0] = d.fill_rgb[0]; v[1] = d.fill_rgb[1]; v[2] = d.fill_rgb[2]; }           // erase
#pragma unroll
        for (int c = 0; c < 3; ++c) o[(3 * j + c) >> 2] |= (unsigned)v[c] << (8 * ((3 * j + c) & 3));
        if (N > 1 && j + 1 < N && ++p == P) {   // the next pixel opens the next frame (first + N <= B P: it exists)
            p = 0; ++b;
            f = frame_params(params, sums, P, group, b);
        }
    }
    if (N == 16) {
        u32x4* q = reinterpret_cast<u32x4*>(out + first * 3);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            u32x4 t; t.x = o[4 * k]; t.y = o[4 * k + 1]; t.z = o[4 * k + 2]; t.w = o[4 * k + 3];
            q[k] = t;
        }
    } else {
        unsigned char* q = out + first * 3;
        q[0] = (unsigned char)(o[0] & 255u); q[1] = (unsigned char)((o[0] >> 8) & 255u); q[2] = (unsigned char)((o[0] >> 16) & 255u);
    }
}

// in and out may be the same buffer: a thread reads all of its pixels before it writes them, and no thread reads another's
__global__ void __launch_bounds__(256) augment_apply_kernel(const unsigned char* in, unsigned char* out, long nvec, long npix, unsigned P, int Ws, int group,
                                                           const int* __restrict__ params, const u64* __restrict__ sums, rpe_augment_desc d) {
    const Span sp = thread_span(nvec, npix);
    if (!sp.any) return;
    if (sp.vec) apply_pixels<16>(in, out, sp.first, P, Ws, group, params, sums, d);
    else apply_pixels<1>(in, out, sp.first, P, Ws, group, params, sums, d);
}

}  // namespace rpe

using namespace rpe;

static bool q16_range_ok(int lo, int hi) { return 0 <= lo && lo <= hi && hi <= 4 * 65536; }

extern "C" int rpe_augment_frames_u8(const unsigned char* in, unsigned char* out, int B, int Hs, int Ws, const rpe_augment_desc* d, unsigned* state,
                                     int* params, unsigned long long* sums, void* stream) {
    if (!in || !out || !d || !state || !params || !sums) return rpe_set_error(RPE_ERR_SHAPE, "augment_frames_u8: null pointer");
    if (B <= 0 || Hs <= 0 || Ws <= 0 || (long)Hs * Ws >= (1L << 32)) return rpe_set_error(RPE_ERR_SHAPE, "augment_frames_u8: bad shape (Hs * Ws must be below 2^32)");
    if (!q16_range_ok(d->qb_lo, d->qb_hi) || !q16_range_ok(d->qc_lo, d->qc_hi) || !q16_range_ok(d->qs_lo, d->qs_hi))
        return rpe_set_error(RPE_ERR_SHAPE, "augment_frames_u8: a Q16 factor range needs 0 <= lo <= hi <= 4 * 65536");
    if (d->noise_q < 0 || d->noise_q > 4 * 65536) return rpe_set_error(RPE_ERR_SHAPE, "augment_frames_u8: noise_q must lie in [0, 4 * 65536]");
    if (d->eh_lo < 1 || d->eh_lo > d->eh_hi || d->eh_hi > Hs || d->ew_lo < 1 || d->ew_lo > d->ew_hi || d->ew_hi > Ws)
        return rpe_set_error(RPE_ERR_SHAPE, "augment_frames_u8: the rectangle bounds need 1 <= lo <= hi <= Hs / Ws");
    if (d->fill_mode != 0 && d->fill_mode != 1) return rpe_set_error(RPE_ERR_SHAPE, "augment_frames_u8: fill_mode is 0 (constant) or 1 (random bytes)");
    if (d->group < 0) return rpe_set_error(RPE_ERR_SHAPE, "augment_frames_u8: group must not be negative");
    const long P = (long)Hs * Ws, npix = (long)B * P, bytes = npix * 3;
    if (in != out && (uintptr_t)in < (uintptr_t)out + (uintptr_t)bytes && (uintptr_t)out < (uintptr_t)in + (uintptr_t)bytes) return rpe_set_error(RPE_ERR_SHAPE, "augment_frames_u8: in and out overlap (the same buffer is allowed)");
    const bool aligned = (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
    const long nvec = aligned ? npix / 16 : 0, nthreads = nvec + (npix - nvec * 16), nblocks = (nthreads + 255) / 256;
    if (nblocks > 0x7fffffffL) return rpe_set_error(RPE_ERR_SHAPE, "augment_frames_u8: too many pixels for one launch");
    const int G = d->group > 0 ? d->group : B;
    const bool contrast = !(d->qc_lo == 65536 && d->qc_hi == 65536);
    hipStream_t s = (hipStream_t)stream;
    note_kernel("augment_params_kernel");
    hipLaunchKernelGGL(augment_params_kernel, dim3(1), dim3(256), 0, s, state, params, contrast ? sums : nullptr, B, G, Hs, Ws, *d);
    RPE_CHECK_LAUNCH();
    if (contrast) {
        prof_split(s, "augment_sum_kernel");
        hipLaunchKernelGGL(augment_sum_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, in, nvec, npix, (unsigned)P, d->group, params, sums);
        RPE_CHECK_LAUNCH();
    }
    prof_split(s, "augment_apply_kernel");
    hipLaunchKernelGGL(augment_apply_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, in, out, nvec, npix, (unsigned)P, Ws, d->group, params,
                       contrast ? sums : nullptr, *d);
    RPE_CHECK_LAUNCH();
    return 0;
}
