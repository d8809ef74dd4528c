// Order-independent float min / max over finite values, shared by the capture kernels (capture.hip) and the saliency kernels
// (saliency.hip).
#pragma once
#include "common.h"

namespace rpe {

__device__ inline bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// Order-independent float min / max through integer atomics on the value's bits: non-negative floats order like signed ints, negative
// ones like unsigned ints reversed.  The SIGN BIT picks the form (not v >= 0): -0 then orders below +0, so the result does not depend
// on the order blocks arrive in (min ends at -0, max at +0 when both occur).  *p starts at +inf (min) / -inf (max).
__device__ inline void atomic_min_f(float* p, float v) {
    if (__float_as_uint(v) >> 31) atomicMax((unsigned*)p, __float_as_uint(v));
    else atomicMin((int*)p, __float_as_int(v));
}
__device__ inline void atomic_max_f(float* p, float v) {
    if (__float_as_uint(v) >> 31) atomicMin((unsigned*)p, __float_as_uint(v));
    else atomicMax((int*)p, __float_as_int(v));
}

}  // namespace rpe
