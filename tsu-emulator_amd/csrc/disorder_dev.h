// disorder_dev.h -- device helpers shared by the heat-bath kernels with per-bond couplings: K7 (ising2d_disorder.hip, 2-D) and
// K8 (ising3d.hip, 3-D).  Both take the same decision: an fp32 screen first, the float64 threshold of the contract only where
// the screen cannot decide.
#pragma once
#include <cmath>

#include "tsu_common.h"

// byte i (0 .. 15) of a 16-byte load, sign-extended: spin i of an octet's 16 columns
__device__ __forceinline__ int sbyte(const uint4& v, int i) {
    const uint32_t w = i < 4 ? v.x : (i < 8 ? v.y : (i < 12 ? v.z : v.w));
    return (int)(int8_t)((w >> (8 * (i & 3))) & 0xFFu);
}

// element i (0 .. 15) of 16 consecutive floats held as four float4
__device__ __forceinline__ float fat(const float4* a, int i) {
    const float4 v = a[i >> 2];
    const int k = i & 3;
    return k == 0 ? v.x : (k == 1 ? v.y : (k == 2 ? v.z : v.w));
}

__device__ __forceinline__ void load16f(const float* p, float4* a) {
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = reinterpret_cast<const float4*>(p)[k];
}

// Threshold of the contract in float64 (sigmoid clamped at +-20 as tsu_ising2d_thresholds / gibbs.py:73-77)
__device__ __forceinline__ uint64_t exact_thr(double f, double T) {
    const double x = (2.0 * f) / T;
    const double p = x > 20.0 ? 1.0 : (x < -20.0 ? 0.0 : 1.0 / (1.0 + exp(-x)));
    return (uint64_t)floor(p * 4294967296.0 + 0.5);
}

// fp32 screen.  Returns +1 (u < thr for every low half), -1 (u >= thr for every low half) or 0 (decide exactly).
// t = p32 2^16 is compared with the hi16 uniform: u in [hi 2^16, hi 2^16 + 65535] is below thr for sure when
// t - dt >= hi + 1 and not below it when t + dt <= hi, dt a bound of |t - thr / 2^16|.  With u = 2^-24, S = the sum of the
// |terms|, A = 2 S / T and n fp32 additions in the field (the products J s are exact, s = +-1):  the additions err by
// <= n u S; times fl(2 / T) adds 2 u |x|: |dx| <= (n + 3) u A.  __expf (v_exp_f32 on x log2 e) errs by <= (|x| + 2) u
// relative, so e = exp(-x) by <= ((n + 5) A + 4) u relative (|x| <= A); p = rcp(1 + e) moves by p (1 - p) <= 1/4 of that plus
// 3 u p of its own rounding: |dp| <= ((n + 5) A / 4 + 4) u + 3 u.  The +-20 clamp of the exact p adds 2.1e-9 = 2^-28.9, and
// the rounding of thr half a unit of 2^-32.  In units of 2^-16: dt <= (((n + 5) A / 4 + 7) + 2^-4.9) / 256 + 2^-17.
//   K7, five terms, n = 4: dt <= (2.25 A + 7.04) / 256 + 2^-17 < (A + 4) / 64 = the margin below, a factor >= 1.7 to spare;
//   K8, seven terms, n = 6: dt <= (2.75 A + 7.04) / 256 + 2^-17 < (4 A + 16) / 256 = the same margin, a factor >= 1.45 to
//   spare (4 / 2.75 as A grows, 16 / 7.05 at A = 0).  The comparisons themselves round h + 1 + m and h - m to fp32 (half an
//   ulp at 2^16: 1 / 256) and A, m carry a relative (n + 2) u: both far inside what is to spare ((1.25 A + 8.9) / 256).
// Non-finite A or t (huge disorder, tiny T) fail both comparisons and go to the exact branch.
__device__ __forceinline__ int screen(float f32, float a32, float c32, uint32_t hi) {
    const float x = f32 * c32;
    const float A = a32 * fabsf(c32);
    const float t = __builtin_amdgcn_rcpf(1.0f + __expf(-x)) * 65536.0f;
    const float m = (A + 4.0f) * (1.0f / 64.0f);
    const float h = (float)hi;
    if (t >= h + 1.0f + m) return 1;
    if (t <= h - m) return -1;
    return 0;
}
