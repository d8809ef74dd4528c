// Occlusion-sensitivity maps (util/model_utils.py: occlusion_sensitivity / render_saliency / visualize_saliency).  DESIGN.md
// "Occlusion sensitivity" has the specification; tests/_saliency_oracle.py restates it in numpy and the kernels are compared with it
// for equality.
//   occlude_grid_kernel       : one raw uint8 frame -> B copies, copy r >= 1 with rectangle k0 + r - 1 of the grid set to the fill colour
//   pose_displacement_kernel  : per predicted pose, distance and rotation angle to a reference pose; double arithmetic, rounded once
//   saliency_map_kernel       : per-rectangle scores -> per-pixel mean over the covering rectangles (+ the map's finite range)
//   saliency_overlay_kernel   : frame + map + range + colour table -> blended uint8 picture, integer arithmetic behind the index
// The grid (shared by all of them and by rpe_occlusion_grid): Gy = ceil((Hs - ph) / sy) + 1 rows of rectangles, row gy at
// top = min(gy sy, Hs - ph); columns alike.  The tops never decrease and the last one is Hs - ph.
#include "common.h"
#include "minmax.h"

namespace rpe {

static_assert(sizeof(rpe_occlusion_desc) == 28, "rpe_occlusion_desc: _lib.OcclusionDesc mirrors this layout");

struct OccGrid { int Gy, Gx; long K; };

__host__ __device__ inline OccGrid occ_grid(const rpe_occlusion_desc& d) {
    OccGrid g;
    g.Gy = (d.Hs - d.ph + d.sy - 1) / d.sy + 1;
    g.Gx = (d.Ws - d.pw + d.sx - 1) / d.sx + 1;
    g.K = (long)g.Gy * g.Gx;
    return g;
}
__device__ inline int occ_min(int a, int b) { return a < b ? a : b; }

// ---------------------------------------------------------------------------------------------------------------- occluded batch
constexpr int kOccLoads = 4;                  // independent loads in flight per thread
constexpr int kOccTile = 256 * kOccLoads;     // units per tile; a tile lies inside one output row

// the bytes of `v`, which start at byte `c0` of the frame, that lie inside the rectangle become the fill colour.  [lo_b, hi_b) is the
// byte span from the rectangle's first to its last byte: a unit outside it (nearly all of them) costs two compares.
template <typename V>
__device__ inline V occ_unit(V v, int c0, int lo_b, int hi_b, int pitch, int top, int bot, int xb0, int xb1, const rpe_occlusion_desc& d) {
    if (c0 + (int)sizeof(V) <= lo_b || c0 >= hi_b) return v;
    unsigned char b[sizeof(V)];
    __builtin_memcpy(b, &v, sizeof(V));
#pragma unroll
    for (int j = 0; j < (int)sizeof(V); ++j) {
        const int cb = c0 + j, y = cb / pitch, xb = cb - y * pitch;
        if (y >= top && y < bot && xb >= xb0 && xb < xb1) {
            const int c = xb % 3;
            b[j] = c == 0 ? d.fill_rgb[0] : (c == 1 ? d.fill_rgb[1] : d.fill_rgb[2]);
        }
    }
    __builtin_memcpy(&v, b, sizeof(V));
    return v;
}

// V: the unit (u32x4, unsigned, unsigned char), chosen by the host from the alignment; C units per frame
template <typename V>
__global__ void __launch_bounds__(256) occlude_grid_kernel(const V* __restrict__ frame, V* __restrict__ out, int C, int tiles_per_row, long ntiles, int k0,
                                                          rpe_occlusion_desc d, int Gx, long K) {
    const int pitch = d.Ws * 3;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long r = tile / tiles_per_row;
        const int base = (int)(tile - r * tiles_per_row) * kOccTile;
        const long k = (long)k0 + r - 1;
        int top = d.Hs, left = 0;                     // no rectangle: row 0 and the padding rows of the last chunk
        if (r >= 1 && k < K) {
            const int gy = (int)(k / Gx), gx = (int)(k - (long)gy * Gx);
            top = occ_min(gy * d.sy, d.Hs - d.ph);
            left = occ_min(gx * d.sx, d.Ws - d.pw);
        }
        const int bot = top + d.ph, xb0 = left * 3, xb1 = (left + d.pw) * 3;
        const int lo_b = top * pitch + xb0, hi_b = top < d.Hs ? (bot - 1) * pitch + xb1 : lo_b;
        const V* __restrict__ p = frame + base + threadIdx.x;
        V* __restrict__ q = out + r * C + base + threadIdx.x;
        const int u0 = base + (int)threadIdx.x;
        if (base + kOccTile <= C) {   // a whole tile (the same for every thread): the four loads issue back to back
            V v[kOccLoads];
#pragma unroll
            for (int j = 0; j < kOccLoads; ++j) v[j] = p[j * 256];
#pragma unroll
            for (int j = 0; j < kOccLoads; ++j) q[j * 256] = occ_unit<V>(v[j], (u0 + j * 256) * (int)sizeof(V), lo_b, hi_b, pitch, top, bot, xb0, xb1, d);
        } else {                      // the last tile of a row that is no multiple of the tile
            for (int u = u0, j = 0; u < C; u += 256, j += 256) q[j] = occ_unit<V>(p[j], u * (int)sizeof(V), lo_b, hi_b, pitch, top, bot, xb0, xb1, d);
        }
    }
}

template <typename V> static int launch_occlude(const void* frame, void* out, long row_bytes, int B, int k0, const rpe_occlusion_desc& d, hipStream_t s) {
    const OccGrid g = occ_grid(d);
    const int C = (int)(row_bytes / (long)sizeof(V)), tiles_per_row = (C + kOccTile - 1) / kOccTile;
    const long ntiles = (long)tiles_per_row * B;
    const unsigned grid = (unsigned)(ntiles < 8192 ? ntiles : 8192);
    hipLaunchKernelGGL(occlude_grid_kernel<V>, dim3(grid), dim3(256), 0, s, (const V*)frame, (V*)out, C, tiles_per_row, ntiles, k0, d, g.Gx, g.K);
    RPE_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- scoring
// Rotation angle between unit quaternions a and b, blind to their signs: with dm = |a - b| and dp = |a + b| (dm^2 + dp^2 = 4) the
// half-angle between a and +-b has tangent min / max, so the angle is 4 atan2(min, max) -- exactly 0 for a == +-b, where 2 acos(<a, b>)
// has an infinite slope and turns one ulp of the inner product into 7e-4 rad.
__global__ void __launch_bounds__(256) pose_displacement_kernel(const float* __restrict__ pred, const float* __restrict__ ref, long n,
                                                               float* __restrict__ pos, float* __restrict__ ori) {
    double r[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) r[k] = (double)ref[k];
    const double nb = sqrt(r[3] * r[3] + r[4] * r[4] + r[5] * r[5] + r[6] * r[6]);
    const double b0 = r[3] / nb, b1 = r[4] / nb, b2 = r[5] / nb, b3 = r[6] / nb;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float* p = pred + i * 7;
        const double dx = (double)p[0] - r[0], dy = (double)p[1] - r[1], dz = (double)p[2] - r[2];
        const double q0 = p[3], q1 = p[4], q2 = p[5], q3 = p[6];
        const double na = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
        const double a0 = q0 / na, a1 = q1 / na, a2 = q2 / na, a3 = q3 / na;   // (an all-zero quaternion: NaN, in ori only)
        const double m0 = a0 - b0, m1 = a1 - b1, m2 = a2 - b2, m3 = a3 - b3;
        const double s0 = a0 + b0, s1 = a1 + b1, s2 = a2 + b2, s3 = a3 + b3;
        const double dm = sqrt(m0 * m0 + m1 * m1 + m2 * m2 + m3 * m3), dp = sqrt(s0 * s0 + s1 * s1 + s2 * s2 + s3 * s3);
        const bool lt = dm < dp;
        pos[i] = (float)sqrt(dx * dx + dy * dy + dz * dz);
        ori[i] = (float)(4.0 * atan2(lt ? dm : dp, lt ? dp : dm));
    }
}

// ---------------------------------------------------------------------------------------------------------------- per-pixel map
__global__ void __launch_bounds__(256) saliency_minmax_init_kernel(float* minmax, int M) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < M) {
        minmax[2 * i] = __uint_as_float(0x7f800000u);
        minmax[2 * i + 1] = __uint_as_float(0xff800000u);
    }
}

// first rectangle row / column that can still reach coordinate c: rectangles g <= (c - p) / s end at or before c
__device__ inline int occ_first(int c, int p, int s, int G) { return c >= p ? occ_min((c - p) / s + 1, G - 1) : 0; }

// grid (pixel blocks, maps).  A thread owns VEC adjacent pixels of one row (VEC = 4: one 16-byte store; Ws % 4 == 0).  The covering
// rectangles are visited by ascending gy, then ascending gx, one correctly rounded add each; then one correctly rounded division.
template <int VEC>
__global__ void __launch_bounds__(256) saliency_map_kernel(const float* __restrict__ scores, int M, rpe_occlusion_desc d, int Gy, int Gx,
                                                          float* __restrict__ maps, float* __restrict__ minmax) {
    const int Wv = d.Ws / VEC, nvec = d.Hs * Wv;
    const long K = (long)Gy * Gx;
    for (int m = blockIdx.y; m < M; m += gridDim.y) {
        const float* __restrict__ s = scores + (long)m * K;
        float lo = __uint_as_float(0x7f800000u), hi = __uint_as_float(0xff800000u);
        for (int start = blockIdx.x * 256; start < nvec; start += gridDim.x * 256) {
            const int i = start + (int)threadIdx.x;
            if (i >= nvec) continue;
            const int y = i / Wv, x0 = (i - y * Wv) * VEC;
            float acc[VEC];
            int cnt[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) { acc[v] = 0.f; cnt[v] = 0; }
            for (int gy = occ_first(y, d.ph, d.sy, Gy); gy < Gy; ++gy) {
                const int top = occ_min(gy * d.sy, d.Hs - d.ph);
                if (y < top) break;              // (the tops never decrease)
                if (y >= top + d.ph) continue;
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const int x = x0 + v;
                    for (int gx = occ_first(x, d.pw, d.sx, Gx); gx < Gx; ++gx) {
                        const int left = occ_min(gx * d.sx, d.Ws - d.pw);
                        if (x < left) break;
                        if (x >= left + d.pw) continue;
                        acc[v] = __fadd_rn(acc[v], s[(long)gy * Gx + gx]);
                        ++cnt[v];
                    }
                }
            }
            float o[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                o[v] = __fdiv_rn(acc[v], (float)cnt[v]);   // (cnt >= 1: the strides do not exceed the rectangle)
                if (finite_f(o[v])) { lo = fminf(lo, o[v]); hi = fmaxf(hi, o[v]); }
            }
            float* q = maps + ((long)m * d.Hs + y) * d.Ws + x0;
            if (VEC == 4) {
                f32x4 w; w.x = o[0]; w.y = o[VEC > 1 ? 1 : 0]; w.z = o[VEC > 2 ? 2 : 0]; w.w = o[VEC > 3 ? 3 : 0];
                *reinterpret_cast<f32x4*>(q) = w;
            } else {
                q[0] = o[0];
            }
        }
        // (every lane arrives here: the loop above has no early exit)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, off));
            hi = fmaxf(hi, __shfl_xor(hi, off));
        }
        if ((threadIdx.x & 63) == 0 && lo <= hi) {   // (a wave without a finite value contributes nothing)
            atomic_min_f(minmax + 2 * m, lo);
            atomic_max_f(minmax + 2 * m + 1, hi);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- overlay
struct OverlayArgs { int alpha_q8, fade; };

__device__ inline void overlay_px(const unsigned char* f, float v, float lo, float hi, const unsigned char* tab, OverlayArgs a, unsigned char* o) {
    if (!finite_f(v)) { o[0] = f[0]; o[1] = f[1]; o[2] = f[2]; return; }
    int k = 0;
    if (hi != lo) {
        // rpe_feature_mosaic's rule: one correctly rounded fp32 operation each (t * 256 is exact)
        const float t = __fdiv_rn(__fsub_rn(v, lo), __fsub_rn(hi, lo));
        if (t >= 1.0f) k = 255;
        else if (t > 0.0f) k = (int)__fmul_rn(t, 256.0f);   // (a range that is not the map's own: clamped, NaN -> 0)
    }
    const int al = a.fade ? (a.alpha_q8 * k) >> 8 : a.alpha_q8;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (unsigned char)(((int)f[c] * (256 - al) + (int)tab[3 * k + c] * al + 128) >> 8);
}

struct u32x3 { unsigned x, y, z; };

// threads [0, nvec): four pixels each -- 12 frame bytes as three dwords, one 16-byte map load, three dword stores; threads
// [nvec, nvec + tail): one pixel each, byte by byte (every pixel when the pointers are not aligned for the wide form)
__global__ void __launch_bounds__(256) saliency_overlay_kernel(const unsigned char* __restrict__ frame, const float* __restrict__ map,
                                                              const float* __restrict__ minmax, const unsigned char* __restrict__ table, int npix, int nvec,
                                                              OverlayArgs a, unsigned char* __restrict__ out) {
    __shared__ unsigned char tab[768];
    for (int i = threadIdx.x; i < 768; i += 256) tab[i] = table[i];
    __syncthreads();
    const float lo = minmax[0], hi = minmax[1];
    const int total = nvec + (npix - 4 * nvec);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        if (i < nvec) {
            const u32x3 w = reinterpret_cast<const u32x3*>(frame)[i];
            const f32x4 v4 = reinterpret_cast<const f32x4*>(map)[i];
            unsigned char f[12], o[12];
            __builtin_memcpy(f, &w, 12);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int p = 0; p < 4; ++p) overlay_px(f + 3 * p, v[p], lo, hi, tab, a, o + 3 * p);
            u32x3 r;
            __builtin_memcpy(&r, o, 12);
            reinterpret_cast<u32x3*>(out)[i] = r;
        } else {
            const int p = 4 * nvec + (i - nvec);
            overlay_px(frame + 3L * p, map[p], lo, hi, tab, a, out + 3L * p);
        }
    }
}

static const char* occ_desc_error(const rpe_occlusion_desc* d) {
    if (d->Hs < 1 || d->Ws < 1) return "the frame size Hs, Ws must be positive";
    if (d->ph < 1 || d->pw < 1 || d->ph > d->Hs || d->pw > d->Ws) return "the rectangle needs 1 <= ph <= Hs and 1 <= pw <= Ws";
    if (d->sy < 1 || d->sx < 1 || d->sy > d->ph || d->sx > d->pw) return "the strides need 1 <= sy <= ph and 1 <= sx <= pw (every pixel is covered)";
    if ((long)d->Hs * d->Ws * 3 >= (1L << 31)) return "Hs * Ws must stay below 2^31 / 3";
    return nullptr;
}

static int occ_refuse(const char* fn, const char* why) {
    char msg[192];
    snprintf(msg, sizeof(msg), "%s: %s", fn, why);
    return rpe_set_error(RPE_ERR_SHAPE, msg);
}

}  // namespace rpe

using namespace rpe;

extern "C" long rpe_occlusion_grid(const rpe_occlusion_desc* d, int* gy, int* gx) {
    const char* why = !d ? "null descriptor" : occ_desc_error(d);
    if (why) { occ_refuse("occlusion_grid", why); return -1; }
    const OccGrid g = occ_grid(*d);
    if (gy) *gy = g.Gy;
    if (gx) *gx = g.Gx;
    return g.K;
}

extern "C" int rpe_occlude_grid_u8(const unsigned char* frame, unsigned char* out, int B, int k0, const rpe_occlusion_desc* d, void* stream) {
    if (!frame || !out || !d) return occ_refuse("occlude_grid_u8", "null pointer");
    if (const char* why = occ_desc_error(d)) return occ_refuse("occlude_grid_u8", why);
    if (B < 1 || k0 < 0) return occ_refuse("occlude_grid_u8", "B must be at least 1 and k0 at least 0");
    const long row_bytes = (long)d->Hs * d->Ws * 3;
    const uintptr_t both = (uintptr_t)frame | (uintptr_t)out;
    hipStream_t s = (hipStream_t)stream;
    note_kernel("occlude_grid_kernel");
    if (row_bytes % 16 == 0 && (both & 15) == 0) return launch_occlude<u32x4>(frame, out, row_bytes, B, k0, *d, s);
    if (row_bytes % 4 == 0 && (both & 3) == 0) return launch_occlude<unsigned>(frame, out, row_bytes, B, k0, *d, s);
    return launch_occlude<unsigned char>(frame, out, row_bytes, B, k0, *d, s);
}

extern "C" int rpe_pose_displacement(const float* pred, const float* ref, long n, float* pos, float* ori, void* stream) {
    if (!pred || !ref || !pos || !ori) return occ_refuse("pose_displacement", "null pointer");
    if (n < 1) return occ_refuse("pose_displacement", "n must be at least 1");
    const long blocks = (n + 255) / 256;
    note_kernel("pose_displacement_kernel");
    hipLaunchKernelGGL(pose_displacement_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, pred, ref, n, pos, ori);
    RPE_CHECK_LAUNCH();
    return 0;
}

extern "C" int rpe_saliency_map(const float* scores, int M, const rpe_occlusion_desc* d, float* maps, float* minmax, void* stream) {
    if (!scores || !d || !maps || !minmax) return occ_refuse("saliency_map", "null pointer");
    if (const char* why = occ_desc_error(d)) return occ_refuse("saliency_map", why);
    if (M < 1) return occ_refuse("saliency_map", "M must be at least 1");
    const OccGrid g = occ_grid(*d);
    hipStream_t s = (hipStream_t)stream;
    note_kernel("saliency_minmax_init_kernel");
    hipLaunchKernelGGL(saliency_minmax_init_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, minmax, M);
    RPE_CHECK_LAUNCH();
    prof_split(s, "saliency_map_kernel");
    const bool vec = d->Ws % 4 == 0 && (((uintptr_t)maps) & 15) == 0;
    const long nvec = (long)d->Hs * (vec ? d->Ws / 4 : d->Ws), blocks = (nvec + 255) / 256;
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096), (unsigned)(M < 65535 ? M : 65535));
    if (vec) hipLaunchKernelGGL(saliency_map_kernel<4>, grid, dim3(256), 0, s, scores, M, *d, g.Gy, g.Gx, maps, minmax);
    else hipLaunchKernelGGL(saliency_map_kernel<1>, grid, dim3(256), 0, s, scores, M, *d, g.Gy, g.Gx, maps, minmax);
    RPE_CHECK_LAUNCH();
    return 0;
}

extern "C" int rpe_saliency_overlay_u8(const unsigned char* frame, const float* map, const float* minmax, const unsigned char* table, int Hs, int Ws,
                                       int alpha_q8, int fade, unsigned char* out, void* stream) {
    if (!frame || !map || !minmax || !table || !out) return occ_refuse("saliency_overlay_u8", "null pointer");
    if (Hs < 1 || Ws < 1) return occ_refuse("saliency_overlay_u8", "the frame size Hs, Ws must be positive");
    if ((long)Hs * Ws * 3 >= (1L << 31)) return occ_refuse("saliency_overlay_u8", "Hs * Ws must stay below 2^31 / 3");
    if (alpha_q8 < 0 || alpha_q8 > 256) return occ_refuse("saliency_overlay_u8", "alpha_q8 lies in [0, 256]");
    const int npix = Hs * Ws;
    const bool wide = ((((uintptr_t)frame) | ((uintptr_t)out)) & 3) == 0 && (((uintptr_t)map) & 15) == 0;
    const int nvec = wide ? npix / 4 : 0, total = nvec + (npix - 4 * nvec);
    const long blocks = ((long)total + 255) / 256;
    OverlayArgs a;
    a.alpha_q8 = alpha_q8;
    a.fade = fade != 0;
    note_kernel("saliency_overlay_kernel");
    hipLaunchKernelGGL(saliency_overlay_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, (hipStream_t)stream, frame, map, minmax, table,
                       npix, nvec, a, out);
    RPE_CHECK_LAUNCH();
    return 0;
}
