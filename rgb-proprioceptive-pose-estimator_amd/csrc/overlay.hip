// Pose overlay (util/learn_utils.py: render_episodes): estimated and true poses drawn on the recorded uint8 frames.  DESIGN.md "Pose
// overlay" and include/rpe_hip.h have the specification; tests/_overlay_oracle.py restates it in numpy and the kernels are compared
// with it for equality.
//   project_poses_kernel : poses + camera matrices -> an integer draw list (Q4 points, bar lengths); fp64, nothing contracted
//   draw_poses_kernel    : frames + draw list + styles -> annotated frames; integer arithmetic only.  A copy with rare touched
//                          pixels, built like occlude_grid_kernel (saliency.hip): units of 16 / 4 / 1 bytes, tiles of 1024 units inside
//                          one frame, four loads in flight, and per tile a table of one bounding box per pose set (computed from
//                          block-uniform addresses, so with scalar loads) that a unit is tested against with two compares per box
#include <math.h>

#include "common.h"

namespace rpe {

static_assert(sizeof(rpe_overlay_style) == 32, "rpe_overlay_style: _lib.OverlayStyle mirrors this layout");

constexpr int kInvalid = RPE_OVERLAY_INVALID;

// ---------------------------------------------------------------------------------------------------------------- projection
struct ProjPoint { int u, v; };

// (the order of operations is the specification: include/rpe_hip.h)
__device__ inline ProjPoint project_point(const double* __restrict__ P, double x, double y, double z) {
#pragma clang fp contract(off)
    const double uw = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
    const double vw = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
    const double w = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
    ProjPoint r = {kInvalid, kInvalid};
    if (!(isfinite(uw) && isfinite(vw) && isfinite(w)) || !(w > RPE_OVERLAY_NEAR)) return r;
    const double lim = (double)RPE_OVERLAY_CLAMP_Q4;
    const double a = floor(16.0 * (uw / w) + 0.5), b = floor(16.0 * (vw / w) + 0.5);
    r.u = (int)fmin(fmax(a, -lim), lim);
    r.v = (int)fmin(fmax(b, -lim), lim);
    return r;
}

__device__ inline int bar_length(float err, double full, int width) {
#pragma clang fp contract(off)
    const double v = ((double)err / full) * (double)width;
    if (!(v == v)) return 0;
    return (int)fmin(fmax(floor(v), 0.0), (double)width);
}

__global__ void __launch_bounds__(256) project_poses_kernel(const float* __restrict__ poses, const double* __restrict__ cam, const int* __restrict__ cam_index,
                                                           long n, int G, int C, double axis_len, const float* __restrict__ pos_err,
                                                           const float* __restrict__ ori_err, double pos_full, double ori_full, int width,
                                                           int* __restrict__ points, int* __restrict__ bars) {
#pragma clang fp contract(off)
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long f = i / G;
        int* out = points + i * 8;
        if (i - f * G == 0) {
            bars[2 * f] = pos_err ? bar_length(pos_err[f], pos_full, width) : 0;
            bars[2 * f + 1] = pos_err ? bar_length(ori_err[f], ori_full, width) : 0;
        }
        const int ci = cam_index[f];
        if (ci < 0 || ci >= C) {
#pragma unroll
            for (int k = 0; k < 8; ++k) out[k] = kInvalid;
            continue;
        }
        const double* P = cam + (long)ci * 12;
        const float* p = poses + i * 7;
        const double x = p[0], y = p[1], z = p[2], qx = p[3], qy = p[4], qz = p[5], qw = p[6];
        const ProjPoint c = project_point(P, x, y, z);
        out[0] = c.u;
        out[1] = c.v;
        const double nn = sqrt(((qx * qx + qy * qy) + qz * qz) + qw * qw);
        const bool tips = c.u != kInvalid && nn > 0.0 && nn < (double)INFINITY;
        const double a = qx / nn, b = qy / nn, cc = qz / nn, d = qw / nn;
        const double col[3][3] = {{1.0 - 2.0 * (b * b + cc * cc), 2.0 * (a * b + cc * d), 2.0 * (a * cc - b * d)},
                                  {2.0 * (a * b - cc * d), 1.0 - 2.0 * (a * a + cc * cc), 2.0 * (b * cc + a * d)},
                                  {2.0 * (a * cc + b * d), 2.0 * (b * cc - a * d), 1.0 - 2.0 * (a * a + b * b)}};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ProjPoint t = {kInvalid, kInvalid};
            if (tips) {
                t = project_point(P, x + axis_len * col[k][0], y + axis_len * col[k][1], z + axis_len * col[k][2]);
                if (t.u != kInvalid) {
                    const int du = t.u - c.u, dv = t.v - c.v;   // (both within +-2^17: no overflow)
                    if (du > RPE_OVERLAY_AXIS_Q4 || du < -RPE_OVERLAY_AXIS_Q4 || dv > RPE_OVERLAY_AXIS_Q4 || dv < -RPE_OVERLAY_AXIS_Q4) t.u = t.v = kInvalid;
                }
            }
            out[2 + 2 * k] = t.u;
            out[3 + 2 * k] = t.v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- drawing
constexpr int kDrawLoads = 4;                  // independent loads in flight per thread
constexpr int kDrawTile = 256 * kDrawLoads;    // units per tile; a tile lies inside one frame

struct DrawArgs {
    const int* points;      // [F][G][4][2]
    const int* bars;        // [F][2]
    long first;             // the list's frame of frame 0
    int Hs, Ws, G, fpe, bar_px, flip;
    int upr;                // units per pixel row (flip: every unit lies inside one pixel row)
    unsigned char bar_rgb[6];
    rpe_overlay_style st[RPE_OVERLAY_MAX_SETS];
};

__device__ inline int dmin(int a, int b) { return a < b ? a : b; }
__device__ inline int dmax(int a, int b) { return a > b ? a : b; }
__device__ inline bool point_ok(int u, int v) {
    return u != kInvalid && v != kInvalid && u >= -RPE_OVERLAY_CLAMP_Q4 && u <= RPE_OVERLAY_CLAMP_Q4 && v >= -RPE_OVERLAY_CLAMP_Q4 && v <= RPE_OVERLAY_CLAMP_Q4;
}
__device__ inline bool axis_ok(int cu, int cv, int tu, int tv) {
    if (!point_ok(cu, cv) || !point_ok(tu, tv)) return false;
    const int du = tu - cu, dv = tv - cv;
    return du <= RPE_OVERLAY_AXIS_Q4 && du >= -RPE_OVERLAY_AXIS_Q4 && dv <= RPE_OVERLAY_AXIS_Q4 && dv >= -RPE_OVERLAY_AXIS_Q4;
}

// the pixels a shape within [lo, hi] (Q4) can touch: every pixel with a subsample 16 x +- 4 in the range, and at most one more a side
struct PixBox { int x0, x1, y0, y1; };   // inclusive; empty when x0 > x1
__device__ inline void box_add(PixBox& b, int ulo, int uhi, int vlo, int vhi) {
    b.x0 = dmin(b.x0, (ulo - 4) >> 4);
    b.x1 = dmax(b.x1, (uhi + 4 + 15) >> 4);
    b.y0 = dmin(b.y0, (vlo - 4) >> 4);
    b.y1 = dmax(b.y1, (vhi + 4 + 15) >> 4);
}

// what a tile knows about its frame: per pose set the box of everything the set draws there, as a byte span [lo_b, hi_b) from the box's
// first to its last byte (a unit outside it costs two compares) and as pixels; the same for the rows of the error bars
struct TileTable {
    int lo_b[RPE_OVERLAY_MAX_SETS], hi_b[RPE_OVERLAY_MAX_SETS];
    PixBox box[RPE_OVERLAY_MAX_SETS];
    int band_lo, band_hi;
    int t;            // the frame's step inside its episode
};

__device__ inline void tile_table(const DrawArgs& a, long gf, TileTable& T) {
    const int pitch = a.Ws * 3;
    T.t = (int)(gf % a.fpe);
#pragma unroll
    for (int g = 0; g < RPE_OVERLAY_MAX_SETS; ++g) {
        PixBox b = {1 << 30, -(1 << 30), 1 << 30, -(1 << 30)};
        if (g < a.G && a.st[g].alpha_q8 > 0) {
            const rpe_overlay_style& s = a.st[g];
            const int* p = a.points + (gf * a.G + g) * 8;
            const int cu = p[0], cv = p[1];
            if (point_ok(cu, cv)) box_add(b, cu - s.r_q4, cu + s.r_q4, cv - s.r_q4, cv + s.r_q4);
            for (int k = 0; k < 3; ++k) {
                const int tu = p[2 + 2 * k], tv = p[3 + 2 * k];
                if (axis_ok(cu, cv, tu, tv)) box_add(b, dmin(cu, tu) - s.hw_q4, dmax(cu, tu) + s.hw_q4, dmin(cv, tv) - s.hw_q4, dmax(cv, tv) + s.hw_q4);
            }
            if ((s.alpha_q8 >> 1) > 0) {
                const int last = dmin(s.trail, T.t);
                for (int k = 1; k <= last; ++k) {
                    const int* q = a.points + ((gf - k) * a.G + g) * 8;
                    const int u = q[0], v = q[1];
                    if (point_ok(u, v)) box_add(b, u - s.trail_r_q4, u + s.trail_r_q4, v - s.trail_r_q4, v + s.trail_r_q4);
                }
            }
        }
        b.x0 = dmax(b.x0, 0);
        b.y0 = dmax(b.y0, 0);
        b.x1 = dmin(b.x1, a.Ws - 1);
        b.y1 = dmin(b.y1, a.Hs - 1);
        const bool some = b.x0 <= b.x1 && b.y0 <= b.y1;
        T.box[g] = b;
        T.lo_b[g] = some ? b.y0 * pitch + 3 * b.x0 : 0;
        T.hi_b[g] = some ? b.y1 * pitch + 3 * (b.x1 + 1) : 0;
    }
    // stored rows of the two bands: the last 2 bar_px output rows
    const int rows = 2 * a.bar_px;
    T.band_lo = (a.flip ? 0 : a.Hs - rows) * pitch;
    T.band_hi = rows > 0 ? T.band_lo + rows * pitch : T.band_lo;
}

__device__ inline void blend3(unsigned char* px, const unsigned char* k, int w) {
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = (unsigned char)(((int)px[c] * (1024 - w) + (int)k[c] * w + 512) >> 10);
}

// subsamples of the pixel at Q4 (sx, sy) inside the disc (cu, cv, r), as a 4-bit mask
__device__ inline int disc_mask(int sx, int sy, int cu, int cv, int r) {
    const int dx0 = sx - cu, dy0 = sy - cv;
    if (dx0 - 4 > r || dx0 + 4 < -r || dy0 - 4 > r || dy0 + 4 < -r) return 0;
    const long rr = (long)r * r;
    int m = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const long dx = dx0 + ((s & 1) ? 4 : -4), dy = dy0 + ((s & 2) ? 4 : -4);
        if (dx * dx + dy * dy <= rr) m |= 1 << s;
    }
    return m;
}

// coverage of the pixel by the capsule from (cu, cv) to (tu, tv) of half-width hw.  Behind the box test |v| <= 2^13 + 2^8 + 8 per
// component and |e| <= 2^13, so |t|, |v x e| <= 2 * 2^13 * (2^13 + 2^9) < 2^28, (v x e)^2 < 2^56, hw^2 L <= 2^16 * 2^27 = 2^43: all int64
__device__ inline int capsule_cov(int sx, int sy, int cu, int cv, int tu, int tv, int hw) {
    if (sx + 4 < dmin(cu, tu) - hw || sx - 4 > dmax(cu, tu) + hw || sy + 4 < dmin(cv, tv) - hw || sy - 4 > dmax(cv, tv) + hw) return 0;
    const long ex = tu - cu, ey = tv - cv, L = ex * ex + ey * ey, hh = (long)hw * hw;
    int cov = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const long vx = sx + ((s & 1) ? 4 : -4) - cu, vy = sy + ((s & 2) ? 4 : -4) - cv;
        const long t = vx * ex + vy * ey;
        bool in;
        if (t <= 0) in = vx * vx + vy * vy <= hh;
        else if (t >= L) in = (vx - ex) * (vx - ex) + (vy - ey) * (vy - ey) <= hh;
        else { const long x = vx * ey - vy * ex; in = x * x <= hh * L; }
        cov += in ? 1 : 0;
    }
    return cov;
}

// everything drawn on pixel (x, y) of the list's frame gf, in the order of the specification
__device__ inline void draw_pixel(const DrawArgs& a, const TileTable& T, long gf, int x, int y, unsigned char* px) {
    const int sx = 16 * x, sy = 16 * y;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int g = 0; g < RPE_OVERLAY_MAX_SETS; ++g) {
            const PixBox& b = T.box[g];
            if (x < b.x0 || x > b.x1 || y < b.y0 || y > b.y1) continue;   // (a set past G has an empty box)
            const rpe_overlay_style& s = a.st[g];
            const int* p = a.points + (gf * a.G + g) * 8;
            if (pass == 0) {
                int m = 0;
                const int last = dmin(s.trail, T.t);
                for (int k = 1; k <= last; ++k) {
                    const int* q = a.points + ((gf - k) * a.G + g) * 8;
                    const int u = q[0], v = q[1];
                    if (point_ok(u, v)) m |= disc_mask(sx, sy, u, v, s.trail_r_q4);
                }
                if (m) blend3(px, s.rgb, __popc(m) * (s.alpha_q8 >> 1));
            } else {
                const int cu = p[0], cv = p[1];
                for (int k = 0; k < 3; ++k) {
                    const int tu = p[2 + 2 * k], tv = p[3 + 2 * k];
                    if (!axis_ok(cu, cv, tu, tv)) continue;
                    const int cov = capsule_cov(sx, sy, cu, cv, tu, tv, s.hw_q4);
                    if (cov) blend3(px, s.axis_rgb + 3 * k, cov * s.alpha_q8);
                }
                if (point_ok(cu, cv)) {
                    const int m = disc_mask(sx, sy, cu, cv, s.r_q4);
                    if (m) blend3(px, s.rgb, __popc(m) * s.alpha_q8);
                }
            }
        }
    }
    if (a.bar_px > 0) {
        const int yo = a.flip ? a.Hs - 1 - y : y, r = yo - (a.Hs - 2 * a.bar_px);
        if (r >= 0) {
            const int band = r >= a.bar_px ? 1 : 0;
            const bool on = x < a.bars[2 * gf + band];
#pragma unroll
            for (int c = 0; c < 3; ++c) px[c] = on ? a.bar_rgb[3 * band + c] : (unsigned char)(px[c] >> 1);
        }
    }
}

// byte j of a unit held as W dwords, and its replacement; the dword is picked with selects, so that the loop over a unit's pixels need
// not be unrolled (unrolled, with the drawing inlined per pixel, the kernel was 150 KB of code: more than the instruction cache)
template <int W> __device__ inline unsigned unit_byte(const unsigned* w, int j) {
    unsigned word = w[0];
#pragma unroll
    for (int k = 1; k < W; ++k) word = (j >> 2) == k ? w[k] : word;
    return (word >> ((j & 3) * 8)) & 255u;
}
template <int W> __device__ inline void set_unit_byte(unsigned* w, int j, unsigned b) {
    const int sh = (j & 3) * 8;
#pragma unroll
    for (int k = 0; k < W; ++k) w[k] = (j >> 2) == k ? (w[k] & ~(255u << sh)) | (b << sh) : w[k];
}

// the unit's bytes pixel by pixel: the pixels p0 .. that own a byte of it, each channel taken from and put back into the unit where it
// lies inside
template <typename V>
__device__ inline V draw_unit(V v, int c0, const DrawArgs& a, const TileTable& T, long gf) {
    constexpr int S = (int)sizeof(V), W = (S + 3) / 4;
    unsigned w[W] = {};
    __builtin_memcpy(w, &v, S);
    const int p0 = c0 / 3, r = c0 - 3 * p0, np = (S + r + 2) / 3;
#pragma unroll 1
    for (int i = 0; i < np; ++i) {
        const int p = p0 + i, y = p / a.Ws, x = p - y * a.Ws, j0 = 3 * i - r;   // j0: where the pixel's first channel lies in the unit
        unsigned char px[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = j0 + c >= 0 && j0 + c < S ? (unsigned char)unit_byte<W>(w, j0 + c) : 0;
        draw_pixel(a, T, gf, x, y, px);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (j0 + c >= 0 && j0 + c < S) set_unit_byte<W>(w, j0 + c, px[c]);
    }
    __builtin_memcpy(&v, w, S);
    return v;
}

// whether the bytes [c0, c0 + len) of the frame can be touched: two compares per box
__device__ inline bool span_hit(int c0, int len, const TileTable& T) {
    bool hit = c0 + len > T.band_lo && c0 < T.band_hi;
#pragma unroll
    for (int g = 0; g < RPE_OVERLAY_MAX_SETS; ++g) hit = hit || (c0 + len > T.lo_b[g] && c0 < T.hi_b[g]);
    return hit;
}

// where unit u of a frame goes: with flip, the same place in the mirrored pixel row
__device__ inline int dest_unit(int u, const DrawArgs& a) {
    if (!a.flip) return u;
    const int y = u / a.upr;
    return (a.Hs - 1 - y) * a.upr + (u - y * a.upr);
}

// V: the unit (u32x4, unsigned, unsigned char), chosen by the host from the alignment; C units per frame
template <typename V>
__global__ void __launch_bounds__(256) draw_poses_kernel(const V* __restrict__ frames, V* __restrict__ out, int C, int tiles_per_frame, long ntiles, DrawArgs a) {
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long f = tile / tiles_per_frame;
        const int base = (int)(tile - f * tiles_per_frame) * kDrawTile;
        const long gf = a.first + f;
        TileTable T;
        tile_table(a, gf, T);
        const V* __restrict__ p = frames + f * C + base + threadIdx.x;
        V* __restrict__ q = out + f * C;
        const int u0 = base + (int)threadIdx.x;
        // the copy: untouched units (nearly all of them) are load-and-store only
        if (base + kDrawTile <= C) {   // a whole tile (the same for every thread): the four loads issue back to back
            V v[kDrawLoads];
#pragma unroll
            for (int j = 0; j < kDrawLoads; ++j) v[j] = p[j * 256];
#pragma unroll
            for (int j = 0; j < kDrawLoads; ++j) q[dest_unit(u0 + j * 256, a)] = v[j];
        } else {                       // the last tile of a frame that is no multiple of the tile
            for (int u = u0, j = 0; u < C; u += 256, j += 256) q[dest_unit(u, a)] = p[j];
        }
        // the units that intersect a box, in the few tiles that do: read again (from the cache) and written again by the thread that copied them
        const int end = base + kDrawTile < C ? base + kDrawTile : C;
        if (!span_hit(base * (int)sizeof(V), (end - base) * (int)sizeof(V), T)) continue;
#pragma unroll 1
        for (int u = u0, j = 0; u < end; u += 256, j += 256) {
            const int c0 = u * (int)sizeof(V);
            if (span_hit(c0, (int)sizeof(V), T)) q[dest_unit(u, a)] = draw_unit<V>(p[j], c0, a, T, gf);
        }
    }
}

template <typename V> static int launch_draw(const void* frames, void* out, long n, long frame_bytes, DrawArgs& a, hipStream_t s) {
    const int C = (int)(frame_bytes / (long)sizeof(V)), tiles_per_frame = (C + kDrawTile - 1) / kDrawTile;
    const long ntiles = (long)tiles_per_frame * n;
    const unsigned grid = (unsigned)(ntiles < 8192 ? ntiles : 8192);
    a.upr = a.Ws * 3 / (int)sizeof(V);
    hipLaunchKernelGGL(draw_poses_kernel<V>, dim3(grid), dim3(256), 0, s, (const V*)frames, (V*)out, C, tiles_per_frame, ntiles, a);
    RPE_CHECK_LAUNCH();
    return 0;
}

static int overlay_refuse(const char* fn, const char* why) {
    char msg[192];
    snprintf(msg, sizeof(msg), "%s: %s", fn, why);
    return rpe_set_error(RPE_ERR_SHAPE, msg);
}

static const char* style_error(const rpe_overlay_style& s) {
    if (s.alpha_q8 < 0 || s.alpha_q8 > 256) return "alpha_q8 lies in [0, 256]";
    if (s.r_q4 < 0 || s.r_q4 > RPE_OVERLAY_MAX_RADIUS_Q4 || s.hw_q4 < 0 || s.hw_q4 > RPE_OVERLAY_MAX_RADIUS_Q4 || s.trail_r_q4 < 0 ||
        s.trail_r_q4 > RPE_OVERLAY_MAX_RADIUS_Q4)
        return "r_q4, hw_q4 and trail_r_q4 lie in [0, 256]";
    if (s.trail < 0 || s.trail > RPE_OVERLAY_MAX_TRAIL) return "the trail length lies in [0, 64]";
    return nullptr;
}

}  // namespace rpe

using namespace rpe;

extern "C" int rpe_project_poses(const float* poses, const double* cam, const int* cam_index, long F, int G, int C, double axis_len, const float* pos_err,
                                 const float* ori_err, double pos_full, double ori_full, int width, int* points, int* bars, void* stream) {
    if (!poses || !cam || !cam_index || !points || !bars) return overlay_refuse("project_poses", "null pointer");
    if ((pos_err == nullptr) != (ori_err == nullptr)) return overlay_refuse("project_poses", "pos_err and ori_err come together");
    if (F < 1 || G < 1 || G > RPE_OVERLAY_MAX_SETS || C < 1) return overlay_refuse("project_poses", "F and C must be at least 1 and G in [1, 4]");
    if (!(pos_full > 0.0) || !(ori_full > 0.0) || !std::isfinite(pos_full) || !std::isfinite(ori_full) || !std::isfinite(axis_len))
        return overlay_refuse("project_poses", "pos_full and ori_full must be positive and finite, axis_len finite");
    if (width < 0 || width > RPE_OVERLAY_MAX_SIDE) return overlay_refuse("project_poses", "the width lies in [0, 4096]");
    const long n = F * G, blocks = (n + 255) / 256;
    note_kernel("project_poses_kernel");
    hipLaunchKernelGGL(project_poses_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, poses, cam, cam_index, n, G, C,
                       axis_len, pos_err, ori_err, pos_full, ori_full, width, points, bars);
    RPE_CHECK_LAUNCH();
    return 0;
}

extern "C" int rpe_draw_poses_u8(const unsigned char* frames, unsigned char* out, long n, int Hs, int Ws, const int* points, const int* bars, long first,
                                 int G, const rpe_overlay_style* styles, int frames_per_episode, int bar_px, const unsigned char* bar_rgb, int flip,
                                 void* stream) {
    if (!frames || !out || !points || !bars || !styles) return overlay_refuse("draw_poses_u8", "null pointer");
    if (n < 1 || first < 0) return overlay_refuse("draw_poses_u8", "n must be at least 1 and first at least 0");
    if (Hs < 1 || Ws < 1 || Hs > RPE_OVERLAY_MAX_SIDE || Ws > RPE_OVERLAY_MAX_SIDE) return overlay_refuse("draw_poses_u8", "Hs and Ws lie in [1, 4096]");
    if (G < 1 || G > RPE_OVERLAY_MAX_SETS) return overlay_refuse("draw_poses_u8", "G lies in [1, 4]");
    if (frames_per_episode < 1) return overlay_refuse("draw_poses_u8", "frames_per_episode must be at least 1");
    if (bar_px < 0 || 2 * (long)bar_px > Hs || (bar_px > 0 && !bar_rgb)) return overlay_refuse("draw_poses_u8", "the bars need 0 <= 2 bar_px <= Hs and their colours");
    DrawArgs a;
    for (int g = 0; g < RPE_OVERLAY_MAX_SETS; ++g) {
        a.st[g] = styles[g < G ? g : 0];
        if (const char* why = style_error(a.st[g])) return overlay_refuse("draw_poses_u8", why);
    }
    a.points = points;
    a.bars = bars;
    a.first = first;
    a.Hs = Hs; a.Ws = Ws; a.G = G; a.fpe = frames_per_episode; a.bar_px = bar_px; a.flip = flip != 0;
    for (int i = 0; i < 6; ++i) a.bar_rgb[i] = bar_px > 0 ? bar_rgb[i] : 0;
    const long pitch = (long)Ws * 3, frame_bytes = pitch * Hs;   // (< 2^26)
    const long fit = a.flip ? (pitch | frame_bytes) : frame_bytes;   // with flip a unit must not straddle two pixel rows
    const uintptr_t both = (uintptr_t)frames | (uintptr_t)out;
    hipStream_t s = (hipStream_t)stream;
    note_kernel("draw_poses_kernel");
    if (fit % 16 == 0 && (both & 15) == 0) return launch_draw<u32x4>(frames, out, n, frame_bytes, a, s);
    if (fit % 4 == 0 && (both & 3) == 0) return launch_draw<unsigned>(frames, out, n, frame_bytes, a, s);
    return launch_draw<unsigned char>(frames, out, n, frame_bytes, a, s);
}
