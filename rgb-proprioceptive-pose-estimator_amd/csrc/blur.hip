// Blur of raw uint8 camera frames on the device (ops.blur_frames_u8, util.data_utils.FrameAugment): defocus (separable Gaussian) and
// linear motion blur, uint8 [B][Hs][Ws][3] -> uint8 of the same shape, run IN FRONT of rpe_augment_frames_u8 (optics first, then
// photometry, noise and the occluder).  DESIGN.md "Frame blur" has the specification; tests/_blur_oracle.py restates it in numpy and
// the kernels are compared with it for equality.
//   blur_params_kernel : reads the step counter state[0] and draws every stream's kind, level, length and direction into `params`.
//                        It does NOT advance the counter: the augment_params_kernel that follows in the same call does
//   blur_tile_kernel   : one block per tile of 32 x 32 pixels inside one frame; the frame's kind is uniform over the block
//                          kind 0: the tile is copied
//                          kind 1: the tile and its halo of clamped pixels go to LDS once (bytes, as in memory), the Gaussian runs
//                                  horizontally into an LDS intermediate (exact, <= 255 * 2048) and then vertically out of it
//                          kind 2: the same LDS tile; every output byte gathers its L taps from it
// All arithmetic is integer, so the result does not depend on the launch geometry.  The replicate border costs nothing after the
// load: the halo holds the clamped pixels, and every global read index is clamped into the frame BEFORE the address is formed.
// A pixel row of the tile is handled as bytes: byte j of a row is channel j % 3 of pixel j / 3, the horizontal neighbour k pixels away
// is byte j + 3 k, and a thread works on the bytes of whole dwords (12 in the horizontal pass, 4 elsewhere) -- 4-byte global loads and
// stores where both pointers are 4-byte aligned and Ws % 4 == 0 (then every pixel row and every tile row starts on a dword), single
// bytes otherwise.  LDS per block: 7104 + 18432 bytes, so 6 blocks share a CU.
#include "common.h"

namespace rpe {

typedef unsigned long long u64;
static_assert(sizeof(rpe_blur_desc) == 480, "rpe_blur_desc: _lib.BlurDesc mirrors this layout");

constexpr unsigned kBlurPurpose = 0x424C5552u;   // "BLUR": counter word 3, apart from augment.hip's 0..2 and the purposes of sample.hip,
                                                 // dropout.hip, depth_augment.hip and measure.hip
constexpr int kBlurTile = 32;                        // pixels per tile side
constexpr int kBlurHalo = 8;                         // the largest radius; the motion blur reaches 7
constexpr int kBlurSide = kBlurTile + 2 * kBlurHalo; // 48 rows / pixels with the halo
constexpr int kBlurRowD = kBlurSide * 3 / 4;         // 36 dwords = 144 bytes per LDS row of the tile
constexpr int kBlurPitchD = kBlurRowD + 1;           // 37: an odd dword pitch, so that a change of row inside a wave shifts the banks
constexpr int kBlurOutB = kBlurTile * 3;             // 96 bytes per tile row without the halo
constexpr int kBlurOutD = kBlurOutB / 4;             // 24 dwords

// one block; G streams
__global__ void __launch_bounds__(256) blur_params_kernel(const unsigned* __restrict__ state, int* __restrict__ params, int G, rpe_blur_desc d) {
    const unsigned step = state[0];
    const unsigned k0 = (unsigned)d.seed, k1 = (unsigned)(d.seed >> 32);
    for (int g = threadIdx.x; g < G; g += 256) {
        unsigned r[4];
        philox4x32_10((unsigned)g, 0u, step, kBlurPurpose, k0, k1, r);
        int* q = params + 1 + 4 * g;
        q[0] = r[0] < d.gauss_thresh ? 1 : ((u64)r[0] < (u64)d.gauss_thresh + d.motion_thresh ? 2 : 0);
        q[1] = (int)__umulhi(r[1], (unsigned)d.n_levels);
        q[2] = 3 + 2 * (int)__umulhi(r[2], (unsigned)d.n_lengths);
        q[3] = (int)__umulhi(r[3], (unsigned)d.n_dirs);
    }
    if (threadIdx.x == 0) params[0] = (int)step;
}

__device__ inline unsigned byte_of(const unsigned* a, int o) { return (a[o >> 2] >> (8 * (o & 3))) & 255u; }

// the 4 bytes `v` of dword g of a tile row whose first `valid` bytes lie in the frame (wide: valid % 4 == 0 and p is dword aligned)
__device__ inline void store_dword(unsigned char* p, int g, unsigned v, bool wide, int valid) {
    if (4 * g >= valid) return;
    if (wide) {
        *reinterpret_cast<unsigned*>(p + 4 * g) = v;
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (4 * g + t < valid) p[4 * g + t] = (unsigned char)(v >> (8 * t));
    }
}

__global__ void __launch_bounds__(256) blur_tile_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, int Hs, int Ws, int tiles_x,
                                                       int tiles_y, int wide_i, const int* __restrict__ params, rpe_blur_desc d) {
    __shared__ unsigned s_in[kBlurSide * kBlurPitchD];                            // 7104 bytes: the tile with its halo, bytes as in memory
    __shared__ __attribute__((aligned(16))) unsigned s_h[kBlurSide * kBlurOutB];  // 18432 bytes: the horizontal pass, one dword per byte
    const int tid = threadIdx.x;
    const bool wide = wide_i != 0;
    const unsigned tpf = (unsigned)tiles_x * (unsigned)tiles_y;
    const unsigned b = blockIdx.x / tpf, tq = blockIdx.x - b * tpf;
    const int ty = (int)(tq / (unsigned)tiles_x), tx = (int)(tq - (unsigned)ty * (unsigned)tiles_x);
    const int x0 = tx * kBlurTile, y0 = ty * kBlurTile;
    const int* q = params + 1 + 4 * (d.group > 0 ? (int)(b % (unsigned)d.group) : (int)b);
    const int kind = q[0];
    const long rowbytes = 3L * Ws;
    const long frame = (long)b * Hs * rowbytes;
    const unsigned char* fin = in + frame;
    unsigned char* fout = out + frame + (long)y0 * rowbytes + 3L * x0;   // the tile's first byte; row y of the tile is fout + y * rowbytes
    const int valid = (int)min(3L * (Ws - x0), (long)kBlurOutB);         // bytes of a tile row inside the frame
    const int rows = min(Hs - y0, kBlurTile);                            // tile rows inside the frame

    if (kind == 0) {   // copy
        if (wide) {    // a thread's three dwords are loaded before any is stored
            unsigned v[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int it = tid + 256 * i, y = it / kBlurOutD, g = it - y * kBlurOutD;
                v[i] = y < rows && 4 * g < valid ? *reinterpret_cast<const unsigned*>(fin + (long)(y0 + y) * rowbytes + 3L * x0 + 4 * g) : 0u;
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int it = tid + 256 * i, y = it / kBlurOutD, g = it - y * kBlurOutD;
                if (y < rows && 4 * g < valid) *reinterpret_cast<unsigned*>(fout + y * rowbytes + 4 * g) = v[i];
            }
        } else {
            for (int it = tid; it < kBlurTile * kBlurOutD; it += 256) {
                const int y = it / kBlurOutD, g = it - y * kBlurOutD;
                if (y >= rows) continue;
                const unsigned char* p = fin + (long)(y0 + y) * rowbytes + 3L * x0 + 4 * g;
                unsigned char* o = fout + y * rowbytes + 4 * g;
                for (int t = 0; t < 4 && 4 * g + t < valid; ++t) o[t] = p[t];
            }
        }
        return;
    }

    const int level = q[1];
    const int R = kind == 1 ? d.radius[level] : kBlurHalo - 1;   // rows the stencil reaches above and below the tile
    const int rlo = kBlurHalo - R, nrows = kBlurTile + 2 * R;

    // the tile and its halo: LDS row r holds pixel row clamp(y0 - 8 + r), its byte e is channel e % 3 of pixel clamp(x0 - 8 + e / 3) of
    // that row.  A thread keeps one dword column and walks down the rows, 7 rows of 36 dwords per round (threads 252 .. 255 rest), so
    // the clamped byte offsets are worked out once.  A dword that lies inside the pixel row is one load; the others (left and right
    // of the frame, or no alignment) are put together from four bytes, each at its clamped pixel
    {
        const int g = tid % kBlurRowD, slot = tid / kBlurRowD;
        if (slot < 7) {
            const long jb = 3L * (x0 - kBlurHalo) + 4 * g;
            const bool whole = wide && jb >= 0 && jb + 4 <= rowbytes;
            long off[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int e = 4 * g + t, p = e / 3, c = e - 3 * p;
                off[t] = 3L * min(max(x0 - kBlurHalo + p, 0), Ws - 1) + c;
            }
            // all of a thread's loads are issued before the first LDS store waits for one: at most 7 rounds (49 >= 48 rows); a round
            // past the last row loads the last row again and stores nothing
            unsigned v[7];
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                const int r = rlo + min(slot + 7 * i, nrows - 1);
                const unsigned char* row = fin + (long)min(max(y0 - kBlurHalo + r, 0), Hs - 1) * rowbytes;
                if (whole) {
                    v[i] = *reinterpret_cast<const unsigned*>(row + jb);
                } else {
                    v[i] = 0;
#pragma unroll
                    for (int t = 0; t < 4; ++t) v[i] |= (unsigned)row[off[t]] << (8 * t);
                }
            }
#pragma unroll
            for (int i = 0; i < 7; ++i)
                if (slot + 7 * i < nrows) s_in[(rlo + slot + 7 * i) * kBlurPitchD + g] = v[i];
        }
    }
    __syncthreads();

    if (kind == 1) {
        unsigned w[kBlurHalo + 1];
#pragma unroll
        for (int k = 0; k <= kBlurHalo; ++k) w[k] = k <= R ? (unsigned)d.taps[level][k] : 0u;   // block-uniform
        // horizontally: 12 bytes (4 pixels) of a row per thread from the 15 dwords that hold their taps, every byte taken out of its
        // dword once; the taps beyond the level's radius are skipped (a block-uniform branch)
        for (int it = tid; it < nrows * (kBlurOutD / 3); it += 256) {
            const int rr = it / (kBlurOutD / 3), g = it - rr * (kBlurOutD / 3), r = rlo + rr;
            unsigned a[15];
#pragma unroll
            for (int i = 0; i < 15; ++i) a[i] = s_in[r * kBlurPitchD + 3 * g + i];
            unsigned acc[12];
#pragma unroll
            for (int u = 0; u < 12; ++u) acc[u] = __umul24(byte_of(a, u + 3 * kBlurHalo), w[0]);
#pragma unroll
            for (int k = 1; k <= kBlurHalo; ++k) {
                if (k > R) break;
#pragma unroll
                for (int u = 0; u < 12; ++u)
                    acc[u] += __umul24(byte_of(a, u + 3 * kBlurHalo - 3 * k) + byte_of(a, u + 3 * kBlurHalo + 3 * k), w[k]);
            }
            u32x4* o = reinterpret_cast<u32x4*>(&s_h[r * kBlurOutB + 12 * g]);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                u32x4 v; v.x = acc[4 * i]; v.y = acc[4 * i + 1]; v.z = acc[4 * i + 2]; v.w = acc[4 * i + 3];
                o[i] = v;
            }
        }
        __syncthreads();
        // vertically: 4 rows x 4 bytes per thread, tap by tap over the level's radius (the weight comes from the descriptor: a scalar load)
        if (tid < (kBlurTile / 4) * kBlurOutD) {
            const int yq = tid / kBlurOutD, g = tid - yq * kBlurOutD;
            unsigned acc[4][4];
#pragma unroll
            for (int y = 0; y < 4; ++y)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[y][t] = 0u;
            for (int k = -R; k <= R; ++k) {
                const unsigned wk = (unsigned)d.taps[level][k < 0 ? -k : k];
#pragma unroll
                for (int y = 0; y < 4; ++y) {
                    const u32x4 v = *reinterpret_cast<const u32x4*>(&s_h[(4 * yq + y + kBlurHalo + k) * kBlurOutB + 4 * g]);
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[y][t] += __umul24(v[t], wk);   // h < 2^20, w <= 2^11
                }
            }
#pragma unroll
            for (int y = 0; y < 4; ++y) {
                if (4 * yq + y >= rows) continue;
                unsigned v = 0;
#pragma unroll
                for (int t = 0; t < 4; ++t) v |= ((acc[y][t] + (1u << 21)) >> 22) << (8 * t);
                store_dword(fout + (long)(4 * yq + y) * rowbytes, g, v, wide, valid);
            }
        }
    } else {
        const int L = q[2], dir = q[3], half = (L - 1) / 2;
        const int cx = d.dir_cx[dir], cy = d.dir_cy[dir];
        // n / (2 L) as (n M) >> 20 with M = 2^20 / (2 L) + 1: exact while n (M 2 L - 2^20) < 2^20, and n <= 2 * 15 * 255 + 15 = 7665 with
        // M 2 L - 2^20 <= 2 L <= 30 (n M < 2^32 as well)
        const unsigned M = (1u << 20) / (2u * (unsigned)L) + 1u;
        for (int it = tid; it < kBlurTile * kBlurOutD; it += 256) {
            const int y = it / kBlurOutD, g = it - y * kBlurOutD;
            if (y >= rows || 4 * g >= valid) continue;
            const int base = (y + kBlurHalo) * kBlurPitchD + g;
            unsigned lo = 0u, hi = 0u;   // the sums of the thread's bytes 0, 2 and 1, 3 in 16-bit halves (at most 15 * 255 each)
            for (int t = -half; t <= half; ++t) {
                const int dx = (t * cx + 128) >> 8, dy = (t * cy + 128) >> 8;   // floor shifts; |dx|, |dy| <= 7
                const int boff = 3 * (kBlurHalo + dx);                          // >= 3: the tap's 4 bytes start there, counted from dword g of the row
                const int at = base + dy * kBlurPitchD + (boff >> 2);
                const unsigned v = __builtin_amdgcn_alignbyte(s_in[at + 1], s_in[at], (unsigned)(boff & 3));   // 4 bytes off the dword grid
                lo += v & 0x00ff00ffu;
                hi += (v >> 8) & 0x00ff00ffu;
            }
            const unsigned s0 = lo & 0xffffu, s1 = hi & 0xffffu, s2 = lo >> 16, s3 = hi >> 16;
            const unsigned v = (((2u * s0 + (unsigned)L) * M) >> 20) | ((((2u * s1 + (unsigned)L) * M) >> 20) << 8) | ((((2u * s2 + (unsigned)L) * M) >> 20) << 16) |
                               ((((2u * s3 + (unsigned)L) * M) >> 20) << 24);
            store_dword(fout + (long)y * rowbytes, g, v, wide, valid);
        }
    }
}

}  // namespace rpe

using namespace rpe;

extern "C" int rpe_blur_frames_u8(const unsigned char* in, unsigned char* out, int B, int Hs, int Ws, const rpe_blur_desc* d, const unsigned* state,
                                  int* params, void* stream) {
    if (!in || !out || !d || !state || !params) return rpe_set_error(RPE_ERR_SHAPE, "blur_frames_u8: null pointer");
    if (B <= 0 || Hs <= 0 || Ws <= 0 || (long)Hs * Ws >= (1L << 32)) return rpe_set_error(RPE_ERR_SHAPE, "blur_frames_u8: bad shape (Hs * Ws must be below 2^32)");
    if (d->n_levels < 1 || d->n_levels > 8) return rpe_set_error(RPE_ERR_SHAPE, "blur_frames_u8: n_levels must lie in [1, 8]");
    for (int s = 0; s < d->n_levels; ++s) {
        if (d->radius[s] < 0 || d->radius[s] > kBlurHalo) return rpe_set_error(RPE_ERR_SHAPE, "blur_frames_u8: a radius must lie in [0, 8]");
        long sum = 0;
        for (int k = 0; k <= d->radius[s]; ++k) {
            if (d->taps[s][k] < 0) return rpe_set_error(RPE_ERR_SHAPE, "blur_frames_u8: a tap must not be negative");
            sum += (k ? 2L : 1L) * d->taps[s][k];
        }
        if (sum != 2048) return rpe_set_error(RPE_ERR_SHAPE, "blur_frames_u8: the taps of a level need w[0] + 2 (w[1] + .. + w[R]) = 2048");
    }
    if (d->n_lengths < 1 || d->n_lengths > 7) return rpe_set_error(RPE_ERR_SHAPE, "blur_frames_u8: n_lengths must lie in [1, 7] (lengths 3 .. 15)");
    if (d->n_dirs < 1 || d->n_dirs > 16) return rpe_set_error(RPE_ERR_SHAPE, "blur_frames_u8: n_dirs must lie in [1, 16]");
    for (int i = 0; i < d->n_dirs; ++i)
        if (d->dir_cx[i] < -256 || d->dir_cx[i] > 256 || d->dir_cy[i] < -256 || d->dir_cy[i] > 256)
            return rpe_set_error(RPE_ERR_SHAPE, "blur_frames_u8: a direction component must lie within +-256");
    if ((u64)d->gauss_thresh + d->motion_thresh > 0xffffffffull) return rpe_set_error(RPE_ERR_SHAPE, "blur_frames_u8: the thresholds' sum must not exceed 2^32 - 1");
    if (d->group < 0) return rpe_set_error(RPE_ERR_SHAPE, "blur_frames_u8: group must not be negative");
    const long bytes = (long)B * Hs * Ws * 3;
    if ((uintptr_t)in < (uintptr_t)out + (uintptr_t)bytes && (uintptr_t)out < (uintptr_t)in + (uintptr_t)bytes)
        return rpe_set_error(RPE_ERR_SHAPE, "blur_frames_u8: in and out overlap (a stencil cannot run in place)");
    const long tiles_x = ((long)Ws + kBlurTile - 1) / kBlurTile, tiles_y = ((long)Hs + kBlurTile - 1) / kBlurTile, nblocks = (long)B * tiles_x * tiles_y;
    if (nblocks > 0x7fffffffL) return rpe_set_error(RPE_ERR_SHAPE, "blur_frames_u8: too many tiles for one launch");
    const int wide = (((uintptr_t)in | (uintptr_t)out) & 3) == 0 && Ws % 4 == 0;
    const int G = d->group > 0 ? d->group : B;
    hipStream_t s = (hipStream_t)stream;
    note_kernel("blur_params_kernel");
    hipLaunchKernelGGL(blur_params_kernel, dim3(1), dim3(256), 0, s, state, params, G, *d);
    RPE_CHECK_LAUNCH();
    prof_split(s, "blur_tile_kernel");
    hipLaunchKernelGGL(blur_tile_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, in, out, Hs, Ws, (int)tiles_x, (int)tiles_y, wide, params, *d);
    RPE_CHECK_LAUNCH();
    return 0;
}
