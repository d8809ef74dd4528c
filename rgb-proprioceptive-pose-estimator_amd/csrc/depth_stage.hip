// Raw depth frames -> the cropped network-size plane (ops.stage_depth): the reference's depth_transform
// (ToPILImage -> Resize(256) -> CenterCrop(224) -> ToTensor on a float32 (H, W, 1) array, util/data_utils.py:55-60) on the device.
//   depth_resize_crop_kernel : Pillow's 32-bit-float bilinear resample (Resample.c, ImagingResampleHorizontal_32bpc / Vertical_32bpc) restricted
//                              to the crop window, one thread per output pixel
// Pillow runs the horizontal pass over whole rows into an fp32 image and the vertical pass over that.  Here a thread recomputes the
// horizontal value of each of its ksy vertical taps in registers (ksx double multiply-adds, rounded to fp32 exactly where Pillow
// stores its intermediate), so there is no intermediate image, no scratch argument and no limit on the scale factor; the re-reads
// stay in L1/L2 (neighbouring pixels share their taps) and the whole pass is a few dozen fp64 operations per pixel.
// Bit-exactness: every product and every sum must be its own correctly rounded operation.  hipcc contracts a * b + c into an FMA by
// default, which rounds once where Pillow's C rounds twice -- and it does so for
// __dadd_rn(c, __dmul_rn(a, b)) as well: the HIP headers define those as plain `*` and `+`, which fuse after inlining (measured:
// v_fmac_f64 in the ISA, and the 130x100 test case one ulp off).  So contraction is switched off for this file's own code, the
// arithmetic is written with plain operators, and the ISA holds v_mul_f64 + v_add_f64.
#include "common.h"

#pragma clang fp contract(off)

namespace rpe {

// one horizontal-pass value: (float) sum_t (double)row[first + t] * k[t], the accumulator starting at 0.0 and the taps added in
// ascending order
__device__ inline float depth_h_tap(const float* __restrict__ row, int first, int count, const double* __restrict__ k) {
    double ss = 0.0;
    for (int t = 0; t < count; ++t) ss = ss + (double)row[first + t] * k[t];   // two roundings (contraction is off)
    return (float)ss;
}

__global__ void __launch_bounds__(256) depth_resize_crop_kernel(const float* __restrict__ frames, float* __restrict__ out, long n, int Hs, int Ws, int top,
                                                               int left, int H, int W, const int* __restrict__ xb, const double* __restrict__ xk, int ksx,
                                                               const int* __restrict__ yb, const double* __restrict__ yk, int ksy) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const long b = i / ((long)W * H);
    const int ox = left + x, oy = top + y;   // position in the resampled Hr x Wr image
    const float* f = frames + b * (long)Hs * Ws;
    // tap ranges, clamped to the source and to the table width: a damaged table cannot send a read outside the frame
    int x0 = ox, nx = 1;
    const double* kx = nullptr;
    if (xb) {
        x0 = min(max(xb[2 * ox], 0), Ws);
        nx = min(min(max(xb[2 * ox + 1], 0), ksx), Ws - x0);
        kx = xk + (long)ox * ksx;
    }
    float v;
    if (yb) {
        const int y0 = min(max(yb[2 * oy], 0), Hs);
        const int ny = min(min(max(yb[2 * oy + 1], 0), ksy), Hs - y0);
        const double* ky = yk + (long)oy * ksy;
        double ss = 0.0;
        for (int t = 0; t < ny; ++t) {
            const float* row = f + (long)(y0 + t) * Ws;
            const float h = xb ? depth_h_tap(row, x0, nx, kx) : row[ox];
            ss = ss + (double)h * ky[t];
        }
        v = (float)ss;
    } else {
        const float* row = f + (long)oy * Ws;
        v = xb ? depth_h_tap(row, x0, nx, kx) : row[ox];
    }
    out[i] = v;
}

}  // namespace rpe

using namespace rpe;

extern "C" int rpe_stage_depth_f32_resized(const float* frames, float* out, int B, int Hs, int Ws, int Hr, int Wr, int top, int left, int H, int W,
                                           const int* xb, const double* xk, int ksx, const int* yb, const double* yk, int ksy, void* stream) {
    if (!frames || !out) return rpe_set_error(RPE_ERR_SHAPE, "stage_depth_f32_resized: null pointer");
    if (B <= 0 || H <= 0 || W <= 0 || Hs <= 0 || Ws <= 0 || top < 0 || left < 0 || Hr < top + H || Wr < left + W)
        return rpe_set_error(RPE_ERR_SHAPE, "stage_depth_f32_resized: bad shape (the crop window must lie inside the resized frame)");
    const bool horiz = Wr != Ws, vert = Hr != Hs;
    if (horiz != (xb != nullptr) || vert != (yb != nullptr) || (horiz && (!xk || ksx <= 0)) || (vert && (!yk || ksy <= 0)))
        return rpe_set_error(RPE_ERR_SHAPE, "stage_depth_f32_resized: a pass that changes the size needs its tap tables, one that does not takes nulls");
    const long n = (long)B * H * W;
    if ((n + 255) / 256 > 0x7fffffffL) return rpe_set_error(RPE_ERR_SHAPE, "stage_depth_f32_resized: too many output pixels for one launch");
    note_kernel("depth_resize_crop_kernel");
    hipLaunchKernelGGL(depth_resize_crop_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, frames, out, n, Hs, Ws, top, left, H, W,
                       xb, xk, ksx, yb, yk, ksy);
    RPE_CHECK_LAUNCH();
    return 0;
}
