// ofl_exp32.h -- the stated float32 exponential of K17 (convex upsampling) and K19 (global matching); include/ofl.h, K17.
#pragma once
#include "ofl_common.h"

namespace ofl {

// exp(t) for t in [-87, 0]: Cody-Waite reduction t = n ln2 + r with a two-part ln2 (n * kLn2Hi is exact: 9 x 7 bits), the
// degree-7 Taylor polynomial in Horner form with separate multiplies and adds, and n added to the exponent field
// (p * 2^n >= exp(-87) > 2^-126, so the field stays positive).  exp32(0) = 1 exactly.
__device__ __forceinline__ float exp32(float t)
{
    constexpr float kLog2e = 1.44269504f, kLn2Hi = 0.693359375f, kLn2Lo = -2.12194440e-4f;
    const float n = __builtin_rintf(__fmul_rn(t, kLog2e));
    float r = __fsub_rn(t, __fmul_rn(n, kLn2Hi));
    r = __fsub_rn(r, __fmul_rn(n, kLn2Lo));
    float p = 1.0f / 5040.0f;
    p = __fadd_rn(__fmul_rn(p, r), 1.0f / 720.0f);
    p = __fadd_rn(__fmul_rn(p, r), 1.0f / 120.0f);
    p = __fadd_rn(__fmul_rn(p, r), 1.0f / 24.0f);
    p = __fadd_rn(__fmul_rn(p, r), 1.0f / 6.0f);
    p = __fadd_rn(__fmul_rn(p, r), 0.5f);
    p = __fadd_rn(__fmul_rn(p, r), 1.0f);
    p = __fadd_rn(__fmul_rn(p, r), 1.0f);
    return __uint_as_float(__float_as_uint(p) + ((uint32_t)__float2int_rz(n) << 23));
}

}  // namespace ofl
