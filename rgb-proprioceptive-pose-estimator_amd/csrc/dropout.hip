// Dropout on the rows the heads read (ops.dropout_begin / ops.dropout_rows, PoseModelBase.set_dropout): inverted dropout of a column
// range of an fp32 [n][ld] matrix, the mask drawn on the device and fresh at every train step.  DESIGN.md "Head dropout" has the
// specification; tests/_dropout_oracle.py restates it in numpy and the kernel is compared with it bit for bit.
//   dropout_begin_kernel : reads the step counter state[0], writes picks[0] = step, advances the counter -- the only reader and writer
//                          of `state` (the pattern of measure_params_kernel), so a captured train step draws a fresh mask at every replay
//   dropout_rows_kernel  : one thread owns one ALIGNED group of four columns (4g .. 4g + 3) and walks the rows grid-stride; one
//                          Philox4x32-10 call at counter (row, g, step, purpose of the site) yields the group's four decisions, word
//                          c & 3 for column c, so an element's fate depends on (row, column, step, site, seed) alone -- never on c0,
//                          c1, n or the launch geometry.  kept (word >= thresh): x * scale, one fp32 multiply; dropped: +0.0f by
//                          SELECTION, so a NaN or an infinity in a dropped position does not survive and -0 does not appear.
// The forward and the backward of a train step run the same kernel on the same picks[0]: they agree on the mask in whatever order they
// run.  A thread reads its elements before it writes them and no thread touches another's, so out == x is allowed.  Streaming, no LDS,
// no atomics: 16-byte accesses for the groups that lie inside [c0, c1) when both pointers and ld allow it, scalar ones for the partial
// groups at either end.
#include "common.h"

namespace rpe {

static_assert(sizeof(rpe_dropout_desc) == 16, "rpe_dropout_desc: _lib.DropoutDesc mirrors this layout");

constexpr unsigned kDropoutPurpose = 0x44524F50u;   // "DROP" + site (0..3): apart from the purposes of augment.hip (0..2), sample.hip
                                                     // ("SAMP"), measure.hip ("MEAK", "MEAS") and depth_augment.hip ("DEPH", "DEPR", "DEPX")
constexpr int kDropoutSites = 4;
constexpr int kDropoutMaxBlocks = 2048;              // 256 CUs x 8 workgroups: the rest of the rows are walked grid-stride

__global__ void __launch_bounds__(64) dropout_begin_kernel(unsigned* __restrict__ state, int* __restrict__ picks) {
    if (threadIdx.x == 0) {
        const unsigned step = state[0];
        picks[0] = (int)step;
        state[0] = step + 1u;   // wraps at 2^32
    }
}

// blockDim = (bx groups, 256 / bx rows); x and out may be the same buffer (no __restrict__ on either)
__global__ void __launch_bounds__(256) dropout_rows_kernel(const float* x, float* out, long n, long ld, int c0, int c1, int g0, int ng, unsigned purpose,
                                                           const int* __restrict__ picks, rpe_dropout_desc d, int vec) {
    const int gi = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (gi >= ng) return;
    const int g = g0 + gi, c = g * 4;
    const unsigned step = (unsigned)picks[0], k0 = (unsigned)d.seed, k1 = (unsigned)(d.seed >> 32);
    const bool whole = vec && c >= c0 && c + 4 <= c1;
    const long stride = (long)gridDim.y * blockDim.y;
    for (long r = (long)blockIdx.y * blockDim.y + threadIdx.y; r < n; r += stride) {
        unsigned w[4];
        philox4x32_10((unsigned)r, (unsigned)g, step, purpose, k0, k1, w);
        const long at = r * ld + c;
        if (whole) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + at);
            f32x4 o;
            o.x = w[0] >= d.thresh ? v.x * d.scale : 0.0f;
            o.y = w[1] >= d.thresh ? v.y * d.scale : 0.0f;
            o.z = w[2] >= d.thresh ? v.z * d.scale : 0.0f;
            o.w = w[3] >= d.thresh ? v.w * d.scale : 0.0f;
            *reinterpret_cast<f32x4*>(out + at) = o;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c + j >= c0 && c + j < c1) {
                    const float v = x[at + j];
                    out[at + j] = w[j] >= d.thresh ? v * d.scale : 0.0f;
                }
        }
    }
}

}  // namespace rpe

using namespace rpe;

extern "C" int rpe_dropout_begin(unsigned* state, int* picks, void* stream) {
    if (!state || !picks) return rpe_set_error(RPE_ERR_SHAPE, "dropout_begin: null pointer");
    note_kernel("dropout_begin_kernel");
    hipLaunchKernelGGL(dropout_begin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, picks);
    RPE_CHECK_LAUNCH();
    return 0;
}

extern "C" int rpe_dropout_rows_f32(const float* x, float* out, long n, int ld, int c0, int c1, int site, const int* picks, const rpe_dropout_desc* d,
                                    void* stream) {
    if (!x || !out || !picks || !d) return rpe_set_error(RPE_ERR_SHAPE, "dropout_rows_f32: null pointer");
    if (n < 1 || n >= (1L << 32)) return rpe_set_error(RPE_ERR_SHAPE, "dropout_rows_f32: n must be at least 1 and below 2^32 (the row is a 32-bit counter word)");
    if (c0 < 0 || c1 > ld || c0 >= c1) return rpe_set_error(RPE_ERR_SHAPE, "dropout_rows_f32: the columns must satisfy 0 <= c0 < c1 <= ld");
    if (site < 0 || site >= kDropoutSites) return rpe_set_error(RPE_ERR_SHAPE, "dropout_rows_f32: site must lie in [0, 4)");
    // the bytes either matrix spans, from its first row's column 0 to the last element written
    const uintptr_t bytes = ((uintptr_t)(n - 1) * (uintptr_t)ld + (uintptr_t)c1) * 4u;
    if (x != out && (uintptr_t)x < (uintptr_t)out + bytes && (uintptr_t)out < (uintptr_t)x + bytes)
        return rpe_set_error(RPE_ERR_SHAPE, "dropout_rows_f32: x and out overlap (the same buffer is allowed)");
    const int g0 = c0 >> 2, ng = ((c1 - 1) >> 2) - g0 + 1;
    const int vec = ((uintptr_t)x % 16 == 0 && (uintptr_t)out % 16 == 0 && ld % 4 == 0) ? 1 : 0;
    int bx = 256;   // groups per workgroup: a power of two, as narrow as the range allows (the other 256 / bx threads take further rows)
    while (bx > 1 && (bx >> 1) >= ng) bx >>= 1;
    const int by = 256 / bx;
    const int gx = ceil_div(ng, bx);
    const long rows_y = (n + by - 1) / by;
    const long cap = kDropoutMaxBlocks / gx > 0 ? kDropoutMaxBlocks / gx : 1;
    const unsigned gy = (unsigned)(rows_y < cap ? rows_y : cap);
    note_kernel("dropout_rows_kernel");
    hipLaunchKernelGGL(dropout_rows_kernel, dim3((unsigned)gx, gy), dim3((unsigned)bx, (unsigned)by), 0, (hipStream_t)stream, x, out, n, (long)ld, c0, c1, g0, ng,
                       kDropoutPurpose + (unsigned)site, picks, *d, vec);
    RPE_CHECK_LAUNCH();
    return 0;
}
