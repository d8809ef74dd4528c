// Measurement noise drawn on the device (ops.measurement_noise, util.data_utils.MeasurementNoise): the proprioceptive input
// x0bar = x0 + N(0, variance I) with the quaternion renormalised (the reference's util/data_utils.py:162-167), fresh at every launch,
// fp32 [S*N][7] -> fp32 of the same shape.  DESIGN.md "Measurement noise" has the specification; tests/_measure_oracle.py restates it
// in numpy and the kernels are compared with it within one fp32 ulp.
//   measure_params_kernel : reads the step counter state[0], writes picks[0] = step and each lane's scale index, advances the counter
//                           -- the only reader and writer of `state`, so a captured launch draws fresh numbers at every replay
//   measure_apply_kernel  : one thread per lane n walks s = 0 .. S-1 with the seven AR(1) values in registers; a thread reads the
//                           seven inputs of a row before it writes them and no thread reads another's rows, so out == x0 is allowed
// Random numbers: Philox4x32-10 keyed by the seed, counter (a, b, step, purpose); the normal is Box-Muller on two words.  All of the
// arithmetic is fp64 with ONE rounding to fp32 at the store; contraction to fused multiply-adds is off, so the sums are the ones the
// specification writes.  The data is a few thousand floats: fp64 throughput does not matter, the two launches do.
#include "common.h"

#include <cmath>

namespace rpe {

static_assert(sizeof(rpe_measure_desc) == 96, "rpe_measure_desc: _lib.MeasureDesc mirrors this layout");

constexpr unsigned kMeasurePickPurpose = 0x4D45414Bu;   // "MEAK": the scale index of a lane
constexpr unsigned kMeasureDrawPurpose = 0x4D454153u;   // "MEAS": the normals of a row
constexpr double kTwoPi = 6.283185307179586476925286766559;
constexpr double kTwoToMinus32 = 1.0 / 4294967296.0;

// one block; N lanes
__global__ void __launch_bounds__(256) measure_params_kernel(unsigned* __restrict__ state, int* __restrict__ picks, rpe_measure_desc d) {
    const unsigned step = state[0];
    __syncthreads();   // every thread has read the counter before it moves
    const unsigned k0 = (unsigned)d.seed, k1 = (unsigned)(d.seed >> 32);
    for (int n = threadIdx.x; n < d.N; n += 256) {
        int k = 0;
        if (d.num_scales > 1) {
            unsigned r[4];
            philox4x32_10((unsigned)n, 0u, step, kMeasurePickPurpose, k0, k1, r);
            k = (int)__umulhi(r[0], (unsigned)d.num_scales);
        }
        picks[1 + n] = k;
    }
    if (threadIdx.x == 0) {
        picks[0] = (int)step;
        state[0] = step + 1u;
    }
}

// x0 and out may be the same buffer (no __restrict__ on either)
__global__ void __launch_bounds__(256) measure_apply_kernel(const float* x0, float* out, const int* __restrict__ picks, rpe_measure_desc d) {
#pragma clang fp contract(off)
    const int n = (int)(blockIdx.x * 256u + threadIdx.x);
    if (n >= d.N) return;
    const unsigned step = (unsigned)picks[0], k0 = (unsigned)d.seed, k1 = (unsigned)(d.seed >> 32);
    const int pick = picks[1 + n];
    double sigma = d.sigma[0];   // a chain of selects: an index known only at run time would send the table to scratch
#pragma unroll
    for (int k = 1; k < 8; ++k) sigma = pick == k ? d.sigma[k] : sigma;
    const double rho = d.rho, fresh = sqrt(1.0 - rho * rho);
    double e[7];
    for (int s = 0; s < d.S; ++s) {
        const long r = (long)s * d.N + n;   // < 2^31 (checked on the host)
        const float* p = x0 + r * 7;
        float* q = out + r * 7;
        float x[7];
        double v[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) x[c] = p[c];
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            unsigned w[4];
            philox4x32_10((unsigned)r, (unsigned)c, step, kMeasureDrawPurpose, k0, k1, w);
            const double u1 = ((double)w[0] + 0.5) * kTwoToMinus32, u2 = (double)w[1] * kTwoToMinus32;
            const double z = sqrt(-2.0 * log(u1)) * cos(kTwoPi * u2);
            e[c] = s == 0 ? z : rho * e[c] + fresh * z;
            v[c] = (double)x[c] + sigma * e[c];
        }
        const double norm = sqrt(v[3] * v[3] + v[4] * v[4] + v[5] * v[5] + v[6] * v[6]);
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = (float)v[c];
#pragma unroll
        for (int c = 3; c < 7; ++c) q[c] = (float)(v[c] / norm);
    }
}

}  // namespace rpe

using namespace rpe;

extern "C" int rpe_measurement_noise(const float* x0, float* out, const rpe_measure_desc* d, unsigned* state, int* picks, void* stream) {
    if (!x0 || !out || !d || !state || !picks) return rpe_set_error(RPE_ERR_SHAPE, "measurement_noise: null pointer");
    if (d->S < 1 || d->N < 1 || (long)d->S * d->N >= (1L << 31)) return rpe_set_error(RPE_ERR_SHAPE, "measurement_noise: S and N must be at least 1 and S * N below 2^31");
    if (d->num_scales < 1 || d->num_scales > 8) return rpe_set_error(RPE_ERR_SHAPE, "measurement_noise: num_scales must lie in [1, 8]");
    for (int k = 0; k < d->num_scales; ++k)
        if (!(d->sigma[k] >= 0.0) || std::isinf(d->sigma[k])) return rpe_set_error(RPE_ERR_SHAPE, "measurement_noise: a sigma must be finite and not negative");
    if (!(d->rho >= 0.0 && d->rho < 1.0)) return rpe_set_error(RPE_ERR_SHAPE, "measurement_noise: rho must lie in [0, 1)");
    const uintptr_t bytes = (uintptr_t)d->S * (uintptr_t)d->N * 28u;
    if (x0 != out && (uintptr_t)x0 < (uintptr_t)out + bytes && (uintptr_t)out < (uintptr_t)x0 + bytes)
        return rpe_set_error(RPE_ERR_SHAPE, "measurement_noise: x0 and out overlap (the same buffer is allowed)");
    hipStream_t s = (hipStream_t)stream;
    note_kernel("measure_params_kernel");
    hipLaunchKernelGGL(measure_params_kernel, dim3(1), dim3(256), 0, s, state, picks, *d);
    RPE_CHECK_LAUNCH();
    prof_split(s, "measure_apply_kernel");
    hipLaunchKernelGGL(measure_apply_kernel, dim3((unsigned)(((long)d->N + 255) / 256)), dim3(256), 0, s, x0, out, (const int*)picks, *d);
    RPE_CHECK_LAUNCH();
    return 0;
}
