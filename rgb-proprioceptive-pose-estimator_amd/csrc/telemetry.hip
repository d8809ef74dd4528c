// Training telemetry (optim.FusedAdam(telemetry=K), util.learn_utils.telemetry_report): per-tensor gradient, weight and update
// statistics of one param group, measured over the flat arenas p, g, m, v after the update, without a host round trip.  Two
// launches whatever the number of tensors; DESIGN.md "Training telemetry" has the dataflow, tests/_telemetry_oracle.py restates
// the arithmetic in numpy.
//   param_stats_kernel           one workgroup per ROW: tensor t (table entry {offset, numel, first_row}) is cut into
//                                param_stats_rows(numel) rows of kStatsChunk elements, and row r of the table's row numbering reduces
//                                its chunk to kStatsPartCols fp64 values, written with plain stores to partials[r][..].  The tensor of
//                                a row is found by bisection over first_row.  Only elements [offset, offset + numel) are loaded: whole
//                                16-byte quads inside the tensor, then the numel % 4 tail one float at a time -- the arena's padding
//                                lanes never reach a register.
//   param_stats_finalize_kernel  one workgroup per tensor: lane c adds (or maximises) column c of the tensor's rows in ascending
//                                order and writes out[t][..].
// Both kernels begin with the gate (long)state[5] % every != 0 -> return, so a captured train step replays them at every step and
// the device decides which steps are measured.  No atomics: wave butterfly, four wave results through LDS added in a fixed order,
// rows added in ascending order -- two runs, and two data-parallel ranks, give the same bits.  Every element is widened to fp64
// before it is used and contraction to fused multiply-adds is off, so the sums are the ones the specification writes.
#include "common.h"

namespace rpe {

constexpr long kStatsChunk = 8192;   // elements per row: 256 threads x 8 trips of one 16-byte load per arena
constexpr int kStatsPartCols = 8;    // sum g^2, sum p^2, sum d^2, max|g|, max|p|, non-finite g, zero g, non-finite p
static_assert(RPE_PARAM_STATS_COLS == 10 && kStatsPartCols == RPE_PARAM_STATS_PART_COLS, "the finalize kernel writes 8 reduced columns, stamp and sticky step");
static_assert(kStatsChunk % 4 == 0, "rows start on a 16-byte boundary");

__host__ __device__ static inline long param_stats_rows(long n) {
    const long r = (n + kStatsChunk - 1) / kStatsChunk;
    return r < 1 ? 1 : r;
}

struct StatsEntry { long offset, numel, first_row; };   // = three int64 of the table

struct StatsAcc {
    double g2, p2, d2, gmax, pmax;
    int g_bad, g_zero, p_bad;
};

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }   // false for inf and NaN

__device__ __forceinline__ void stats_take(StatsAcc& a, float gf, float pf, float mf, float vf, double bc1, double bc2_sqrt, double eps) {
#pragma clang fp contract(off)
    const double g = (double)gf, p = (double)pf;
    if (finite_d(g)) {
        a.g2 += g * g;
        a.gmax = fmax(a.gmax, fabs(g));
        a.g_zero += g == 0.0;
    } else {
        a.g_bad += 1;
    }
    if (finite_d(p)) {
        a.p2 += p * p;
        a.pmax = fmax(a.pmax, fabs(p));
    } else {
        a.p_bad += 1;
    }
    const double d = ((double)mf / bc1) / (sqrt((double)vf) / bc2_sqrt + eps);   // the Adam direction of the update just applied
    if (finite_d(d)) a.d2 += d * d;
}

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(256) void param_stats_kernel(const float* __restrict__ p, const float* __restrict__ g, const float* __restrict__ m,
                                                         const float* __restrict__ v, const StatsEntry* __restrict__ table, int T,
                                                         double* __restrict__ part, double b1, double b2, double eps,
                                                         const float* __restrict__ st, long every) {
    if ((long)st[5] % every != 0) return;   // not a measured step: partials (and out) keep their contents
    __shared__ double red[4][kStatsPartCols];
    // the last tensor whose first_row <= this row (first_row ascends strictly: every tensor has at least one row)
    const long row = blockIdx.x;
    int lo = 0, hi = T - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_row <= row) lo = mid; else hi = mid - 1;
    }
    const StatsEntry e = table[lo];
    const long begin = (row - e.first_row) * kStatsChunk;                                       // within the tensor
    const long count = e.numel - begin < kStatsChunk ? e.numel - begin : kStatsChunk;           // <= 0 only for an empty tensor
    const long base = e.offset + begin;                                                         // a multiple of 4 floats
    const double step = (double)st[5];
    const double bc1 = 1.0 - pow(b1, step), bc2_sqrt = sqrt(1.0 - pow(b2, step));

    StatsAcc a = {0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0};
    const long quads = count > 0 ? count >> 2 : 0;
    const f32x4 *p4 = (const f32x4*)(p + base), *g4 = (const f32x4*)(g + base), *m4 = (const f32x4*)(m + base), *v4 = (const f32x4*)(v + base);
#pragma unroll 2
    for (long i = threadIdx.x; i < quads; i += 256) {
        const f32x4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) stats_take(a, gg[k], pp[k], mm[k], vv[k], bc1, bc2_sqrt, eps);
    }
    if (count > 0 && (long)threadIdx.x < (count & 3)) {   // the tensor's last 1..3 elements (last row only: a chunk is a multiple of 4)
        const long i = base + (quads << 2) + threadIdx.x;
        stats_take(a, g[i], p[i], m[i], v[i], bc1, bc2_sqrt, eps);
    }

    double r[kStatsPartCols];
    r[0] = wave_sum_d(a.g2); r[1] = wave_sum_d(a.p2); r[2] = wave_sum_d(a.d2);
    r[3] = wave_max_d(a.gmax); r[4] = wave_max_d(a.pmax);
    r[5] = wave_sum_d((double)a.g_bad); r[6] = wave_sum_d((double)a.g_zero); r[7] = wave_sum_d((double)a.p_bad);   // counts: exact in fp64
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < kStatsPartCols; ++c) red[threadIdx.x >> 6][c] = r[c];
    }
    __syncthreads();
    if (threadIdx.x < kStatsPartCols) {
        const int c = threadIdx.x;
        const bool is_max = c == 3 || c == 4;
        const double x = is_max ? fmax(fmax(red[0][c], red[1][c]), fmax(red[2][c], red[3][c])) : ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
        part[row * kStatsPartCols + c] = x;
    }
}

__global__ __launch_bounds__(64) void param_stats_finalize_kernel(const double* __restrict__ part, const StatsEntry* __restrict__ table,
                                                                 double* __restrict__ out, const float* __restrict__ st, long every) {
    if ((long)st[5] % every != 0) return;
    const StatsEntry e = table[blockIdx.x];
    const long rows = param_stats_rows(e.numel);
    const int c = threadIdx.x & (kStatsPartCols - 1);   // lanes 8.. repeat lanes 0..7 (the shuffles below read lanes 5 and 7)
    const bool is_max = c == 3 || c == 4;
    const double* col = part + e.first_row * kStatsPartCols + c;
    double x = 0.0;
#pragma unroll 4
    for (long r = 0; r < rows; ++r) {
        const double y = col[r * kStatsPartCols];
        x = is_max ? fmax(x, y) : x + y;
    }
    const double g_bad = __shfl(x, 5), p_bad = __shfl(x, 7);
    double* o = out + (long)blockIdx.x * RPE_PARAM_STATS_COLS;
    if (threadIdx.x < kStatsPartCols) o[c] = (c == 2 && st[3] != 0.f) ? 0.0 : x;   // a skipped fp16 step applied no update
    if (threadIdx.x == 0) {
        const double step = (double)st[5];
        o[8] = step;
        if ((g_bad != 0.0 || p_bad != 0.0) && o[9] == 0.0) o[9] = step;   // sticky until the host zeroes it
    }
}

}  // namespace rpe

using namespace rpe;

extern "C" long rpe_param_stats_rows(long n) { return param_stats_rows(n); }

extern "C" int rpe_param_stats(const float* p, const float* g, const float* m, const float* v, const long* table, const long* table_host, int T,
                               double* partials, double beta1, double beta2, double eps, const float* state, long every, void* stream) {
    if (T <= 0) return rpe_set_error(RPE_ERR_SHAPE, "param_stats: T >= 1");
    if (!p || !g || !m || !v || !table || !table_host || !partials || !state) return rpe_set_error(RPE_ERR_SHAPE, "param_stats: null pointer");
    if (every < 1) return rpe_set_error(RPE_ERR_SHAPE, "param_stats: every >= 1");
    if ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) return rpe_set_error(RPE_ERR_ALIGN, "param_stats: the four arenas must be 16-byte aligned");
    if ((((uintptr_t)table) | ((uintptr_t)partials)) & 7) return rpe_set_error(RPE_ERR_ALIGN, "param_stats: table and partials must be 8-byte aligned");
    long rows = 0;
    for (int t = 0; t < T; ++t) {
        const long off = table_host[3 * t], n = table_host[3 * t + 1], first = table_host[3 * t + 2];
        if (off < 0 || n < 0 || first != rows) return rpe_set_error(RPE_ERR_SHAPE, "param_stats: a table entry needs offset >= 0, numel >= 0 and first_row = the rows of the entries before it");
        if (off & 3) return rpe_set_error(RPE_ERR_ALIGN, "param_stats: every offset must be a multiple of 4 floats");
        rows += param_stats_rows(n);
    }
    if (rows >= (1L << 31)) return rpe_set_error(RPE_ERR_SHAPE, "param_stats: more than 2^31 - 1 rows");
    note_kernel("param_stats_kernel");
    hipLaunchKernelGGL(param_stats_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (const StatsEntry*)table, T, partials,
                       beta1, beta2, eps, state, every);
    RPE_CHECK_LAUNCH();
    return 0;
}

extern "C" int rpe_param_stats_finalize(const double* partials, const long* table, int T, double* out, const float* state, long every, void* stream) {
    if (T <= 0) return rpe_set_error(RPE_ERR_SHAPE, "param_stats_finalize: T >= 1");
    if (!partials || !table || !out || !state) return rpe_set_error(RPE_ERR_SHAPE, "param_stats_finalize: null pointer");
    if (every < 1) return rpe_set_error(RPE_ERR_SHAPE, "param_stats_finalize: every >= 1");
    if ((((uintptr_t)table) | ((uintptr_t)partials) | ((uintptr_t)out)) & 7) return rpe_set_error(RPE_ERR_ALIGN, "param_stats_finalize: table, partials and out must be 8-byte aligned");
    note_kernel("param_stats_finalize_kernel");
    hipLaunchKernelGGL(param_stats_finalize_kernel, dim3((unsigned)T), dim3(64), 0, (hipStream_t)stream, partials, (const StatsEntry*)table, out, state, every);
    RPE_CHECK_LAUNCH();
    return 0;
}
