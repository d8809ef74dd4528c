// Shuffled minibatches from recorded episodes resident in HBM (ops.sample_windows / ops.gather_rows, util.data_utils.WindowSampler),
// IN FRONT of the augmentation and the staging kernels, which stay as they are.  DESIGN.md "Minibatch sampling" has the specification;
// tests/_sampler_oracle.py restates it in numpy and the kernels are compared with it for equality.
//   sample_index_kernel : reads the step counter state[0], writes index[0] = step and the (episode, first timestep) of the step's N
//                         windows, advances the counter -- the only reader and writer of `state`, so a captured launch draws the next
//                         batch at every replay
//   sample_index_ragged_kernel : the same for episodes of unequal length; the window table is scanned on the device at every launch
//   gather_rows_kernel  : out row s N + n <- pool row episode[n] T + t0[n] + s, rows of row_bytes bytes; one kernel for frames, depth,
//                         poses and measurements
// All arithmetic is unsigned / 64-bit integer.  The shuffle is a keyed bijection of [0, M): a 4-round balanced Feistel network over
// 2h bits whose round function is word 0 of Philox4x32-10, cycle-walked back into [0, M).
// The gather walks TILES of 4 x 256 units (a unit = 16, 4 or 1 bytes, chosen by the host from the alignment): a tile lies inside one
// row, so the row arithmetic (two 64-bit divisions, two index reads) is per tile and wave-uniform; in a whole tile a thread issues
// its four loads, 256 units apart (every wave-instruction reads 64 consecutive units), before the first store; the last tile of a row
// that is no multiple of the tile copies unit by unit under a guard.
#include "common.h"

namespace rpe {

typedef unsigned long long u64;
static_assert(sizeof(rpe_sample_desc) == 32, "rpe_sample_desc: _lib.SampleDesc mirrors this layout");

constexpr unsigned kSamplePurpose = 0x53414D50u;   // "SAMP": counter word 3, apart from the augmentation's purposes 0..2

// one block; K start positions per episode, M = E K windows, h = half the width of the Feistel domain in bits
__global__ void __launch_bounds__(256) sample_index_kernel(unsigned* __restrict__ state, int* __restrict__ index, const int* __restrict__ sel,
                                                          rpe_sample_desc d, unsigned K, unsigned M, int h) {
    const unsigned step = state[0];
    __syncthreads();   // every thread has read the counter before it moves
    const unsigned k0 = (unsigned)d.seed, k1 = (unsigned)(d.seed >> 32), mask = (1u << h) - 1u;
    for (int i = threadIdx.x; i < d.N; i += 256) {
        const u64 g = (u64)step * (u64)d.N + (u64)i;
        const u64 epoch = g / M;
        unsigned w = (unsigned)(g - epoch * M);
        if (d.shuffle && M > 1) {
            do {   // ends: w lies on the cycle through pos < M
                unsigned L = w >> h, R = w & mask;
#pragma unroll
                for (unsigned r = 0; r < 4; ++r) {
                    unsigned f[4];
                    philox4x32_10(R, r, (unsigned)epoch, kSamplePurpose, k0, k1, f);
                    const unsigned t = L ^ (f[0] & mask);
                    L = R; R = t;
                }
                w = (L << h) | R;
            } while (w >= M);
        }
        const unsigned e = w / K;
        index[1 + 2 * i] = sel[e];
        index[2 + 2 * i] = (int)((w - e * K) * (unsigned)d.stride);
    }
    if (threadIdx.x == 0) {
        index[0] = (int)step;
        state[0] = step + 1u;
    }
}

// ---- episodes of unequal length ----------------------------------------------------------------------------------------------
// The same draw over windows that no longer form an E x K grid: episode e of the selection has len_e = clamp(lengths[sel[e]], 0, T)
// timesteps and K_e = len_e >= S ? (len_e - S) / stride + 1 : 0 start positions; P_e = K_0 + .. + K_{e-1} and M = P_E.  `lengths` and
// `sel` are read at every launch, so M -- and with it the domain of the keyed permutation -- belongs to the launch, not to the host:
// the block scans the K_e into LDS (every thread a run of consecutive episodes, the runs' totals through the wave and the four waves),
// takes the Feistel half width from this M, and finds a window's episode by binary search, the largest e with P_e <= w.
constexpr int kRaggedMaxEpisodes = 8192;   // the prefix table: 32 KB of LDS

__global__ void __launch_bounds__(256) sample_index_ragged_kernel(unsigned* __restrict__ state, int* __restrict__ index, const int* __restrict__ sel,
                                                                 const int* __restrict__ lengths, rpe_sample_desc d) {
    __shared__ unsigned P[kRaggedMaxEpisodes];   // P[e]: windows in front of episode e
    __shared__ unsigned wsum[4];
    const unsigned step = state[0];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int per = (d.E + 255) / 256, e0 = (int)threadIdx.x * per, e1 = e0 + per < d.E ? e0 + per : d.E;
    unsigned run = 0;
    for (int e = e0; e < e1; ++e) {
        int len = lengths[sel[e]];
        len = len < 0 ? 0 : (len > d.T ? d.T : len);
        P[e] = run;
        run += len >= d.S ? (unsigned)(len - d.S) / (unsigned)d.stride + 1u : 0u;
    }
    unsigned inc = run;   // inclusive scan of the runs' totals along the wave
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();   // the waves' totals are stored; every thread has read the counter before it moves
    unsigned base = inc - run;
    for (int w = 0; w < wv; ++w) base += wsum[w];
    for (int e = e0; e < e1; ++e) P[e] += base;
    const unsigned M = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();   // the table is complete
    const int bits = M > 1u ? 32 - __clz(M - 1u) : 0;   // bit length of M - 1
    const int h = ((bits > 2 ? bits : 2) + 1) / 2;
    const unsigned k0 = (unsigned)d.seed, k1 = (unsigned)(d.seed >> 32), mask = (1u << h) - 1u;
    for (int i = threadIdx.x; i < d.N; i += 256) {
        if (M == 0u) {   // no window at all: in bounds for the gather, and meaningless
            index[1 + 2 * i] = sel[0];
            index[2 + 2 * i] = 0;
            continue;
        }
        const u64 g = (u64)step * (u64)d.N + (u64)i;
        const u64 epoch = g / M;
        unsigned w = (unsigned)(g - epoch * M);
        if (d.shuffle && M > 1) {
            do {   // ends: w lies on the cycle through pos < M
                unsigned L = w >> h, R = w & mask;
#pragma unroll
                for (unsigned r = 0; r < 4; ++r) {
                    unsigned f[4];
                    philox4x32_10(R, r, (unsigned)epoch, kSamplePurpose, k0, k1, f);
                    const unsigned t = L ^ (f[0] & mask);
                    L = R; R = t;
                }
                w = (L << h) | R;
            } while (w >= M);
        }
        int lo = 0, hi = d.E - 1;   // P[lo] <= w throughout (P[0] = 0)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (P[mid] <= w) lo = mid; else hi = mid - 1;
        }
        index[1 + 2 * i] = sel[lo];
        index[2 + 2 * i] = (int)((w - P[lo]) * (unsigned)d.stride);
    }
    if (threadIdx.x == 0) {
        index[0] = (int)step;
        state[0] = step + 1u;
    }
}

constexpr int kGatherLoads = 4;                    // independent loads in flight per thread
constexpr long kGatherTile = 256 * kGatherLoads;   // units per tile

// V: the unit (u32x4, unsigned, unsigned char); C units per row; tiles_per_row = ceil(C / kGatherTile)
template <typename V>
__global__ void __launch_bounds__(256) gather_rows_kernel(const V* __restrict__ pool, V* __restrict__ out, long C, long T, const int* __restrict__ index, int N,
                                                         long tiles_per_row, long ntiles) {
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long row = tile / tiles_per_row;              // s N + n
        const long s = row / N, n = row - s * N;
        const long src = (long)index[1 + 2 * n] * T + (long)index[2 + 2 * n] + s;
        const long base = (tile - row * tiles_per_row) * kGatherTile;
        const V* __restrict__ p = pool + src * C + base + threadIdx.x;
        V* __restrict__ q = out + row * C + base + threadIdx.x;
        if (base + kGatherTile <= C) {   // a whole tile (the same for every thread): no guards, so the four loads issue back to back
            V v[kGatherLoads];
#pragma unroll
            for (int k = 0; k < kGatherLoads; ++k) v[k] = p[k * 256];
#pragma unroll
            for (int k = 0; k < kGatherLoads; ++k) q[k * 256] = v[k];
        } else {                         // the last tile of a row that is no multiple of the tile
            for (long c = base + threadIdx.x, k = 0; c < C; c += 256, k += 256) q[k] = p[k];
        }
    }
}

template <typename V> static int launch_gather(const void* pool, void* out, long row_bytes, long T, const int* index, int S, int N, hipStream_t s) {
    const long C = row_bytes / (long)sizeof(V), tiles_per_row = (C + kGatherTile - 1) / kGatherTile, ntiles = tiles_per_row * S * N;
    // a tile is 16 KiB of 16-byte units: one block each up to 8192 blocks (the flagship batch, 256 frames of 196,608 bytes, is 3,072),
    // a grid-stride walk beyond
    const unsigned grid = (unsigned)(ntiles < 8192 ? ntiles : 8192);
    hipLaunchKernelGGL(gather_rows_kernel<V>, dim3(grid), dim3(256), 0, s, (const V*)pool, (V*)out, C, T, index, N, tiles_per_row, ntiles);
    RPE_CHECK_LAUNCH();
    return 0;
}

}  // namespace rpe

using namespace rpe;

extern "C" int rpe_sample_windows(const rpe_sample_desc* d, const int* sel, unsigned* state, int* index, void* stream) {
    if (!d || !sel || !state || !index) return rpe_set_error(RPE_ERR_SHAPE, "sample_windows: null pointer");
    if (d->E < 1 || d->T < 1 || d->S < 1 || d->stride < 1 || d->N < 1) return rpe_set_error(RPE_ERR_SHAPE, "sample_windows: E, T, S, stride and N must be at least 1");
    if (d->S > d->T) return rpe_set_error(RPE_ERR_SHAPE, "sample_windows: a window of S timesteps needs S <= T");
    if (d->shuffle != 0 && d->shuffle != 1) return rpe_set_error(RPE_ERR_SHAPE, "sample_windows: shuffle is 0 (file order) or 1 (keyed permutation)");
    const long K = (long)(d->T - d->S) / d->stride + 1, M = (long)d->E * K;
    if (M >= (1L << 31)) return rpe_set_error(RPE_ERR_SHAPE, "sample_windows: E * K windows must stay below 2^31");
    int bits = 0;
    while (((M - 1) >> bits) != 0) ++bits;   // bit length of M - 1
    const int h = ((bits > 2 ? bits : 2) + 1) / 2;
    note_kernel("sample_index_kernel");
    hipLaunchKernelGGL(sample_index_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, state, index, sel, *d, (unsigned)K, (unsigned)M, h);
    RPE_CHECK_LAUNCH();
    return 0;
}

extern "C" int rpe_sample_windows_ragged(const rpe_sample_desc* d, const int* sel, const int* lengths, unsigned* state, int* index, void* stream) {
    if (!d || !sel || !lengths || !state || !index) return rpe_set_error(RPE_ERR_SHAPE, "sample_windows_ragged: null pointer");
    if (d->E < 1 || d->T < 1 || d->S < 1 || d->stride < 1 || d->N < 1) return rpe_set_error(RPE_ERR_SHAPE, "sample_windows_ragged: E, T, S, stride and N must be at least 1");
    if (d->S > d->T) return rpe_set_error(RPE_ERR_SHAPE, "sample_windows_ragged: a window of S timesteps needs S <= T");
    if (d->shuffle != 0 && d->shuffle != 1) return rpe_set_error(RPE_ERR_SHAPE, "sample_windows_ragged: shuffle is 0 (file order) or 1 (keyed permutation)");
    if (d->E > kRaggedMaxEpisodes) return rpe_set_error(RPE_ERR_SHAPE, "sample_windows_ragged: at most 8192 selected episodes (the prefix table lives in LDS)");
    const long K = (long)(d->T - d->S) / d->stride + 1;   // the most any episode can have
    if ((long)d->E * K >= (1L << 31)) return rpe_set_error(RPE_ERR_SHAPE, "sample_windows_ragged: E * max K windows must stay below 2^31");
    note_kernel("sample_index_ragged_kernel");
    hipLaunchKernelGGL(sample_index_ragged_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, state, index, sel, lengths, *d);
    RPE_CHECK_LAUNCH();
    return 0;
}

extern "C" int rpe_gather_rows(const void* pool, void* out, long row_bytes, long T, const int* index, int S, int N, void* stream) {
    if (!pool || !out || !index) return rpe_set_error(RPE_ERR_SHAPE, "gather_rows: null pointer");
    if (row_bytes < 1 || T < 1 || S < 1 || N < 1) return rpe_set_error(RPE_ERR_SHAPE, "gather_rows: row_bytes, T, S and N must be at least 1");
    if (S > T) return rpe_set_error(RPE_ERR_SHAPE, "gather_rows: a window of S timesteps needs S <= T");
    const uintptr_t both = (uintptr_t)pool | (uintptr_t)out;
    hipStream_t s = (hipStream_t)stream;
    note_kernel("gather_rows_kernel");
    if (row_bytes % 16 == 0 && (both & 15) == 0) return launch_gather<u32x4>(pool, out, row_bytes, T, index, S, N, s);
    if (row_bytes % 4 == 0 && (both & 3) == 0) return launch_gather<unsigned>(pool, out, row_bytes, T, index, S, N, s);
    return launch_gather<unsigned char>(pool, out, row_bytes, T, index, S, N, s);
}
