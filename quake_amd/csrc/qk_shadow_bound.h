// qk_shadow_bound.h -- the error bound of the fp16 shadow form (qk_shadow.hip; derivation: DESIGN.md 5.20).  One function for the
// host (qk_shadow_error_bound, the C ABI) and the device (k_shadow_prep evaluates it per query).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define QK_SHADOW_HD __host__ __device__
#else  // (a plain C++ compiler: tests/native/shadow_bound_check.cpp)
#define QK_SHADOW_HD
#endif

// |approximate key - canonical fp32 key| <= the value returned, for a query q and any row x with
//   qn >= ||q||,  rho_q >= ||q - fp16(q)||,  rho >= ||x - fp16(x)||,  xmax >= ||fp16(x)||
// where a distance to an fp16 image counts a subnormal element as the farther of itself and zero (the bound holds whether or not
// the matrix unit flushes subnormal inputs).  Negative: no bound (an argument is negative, not finite, or the bound overflows).
// Every step rounds to nearest and is widened by 1 + 2^-10, which covers the roundings of this function itself.
QK_SHADOW_HD inline float qk_shadow_bound(int metric_l2, int d, float qn, float rho_q, float rho, float xmax) {
    if (!(qn >= 0.f) || !(rho_q >= 0.f) || !(rho >= 0.f) || !(xmax >= 0.f) || d <= 0) return -1.f;
    const float up = 1.0009765625f;
    const float xr = (xmax + rho) * up;  // >= ||x||
    const float qr = (qn + rho_q) * up;  // >= ||fp16(q)||
    // q.x - q^.x^ = q.(x - x^) + (q - q^).x^ in real arithmetic (Cauchy-Schwarz)
    float dot = ((qn * rho) * up + (rho_q * xmax) * up) * up;
    // the matrix unit's fp32 accumulation of n exact fp16 products in an unknown order (n 2^-23 sum |q^ x^|, one ulp per step
    // whatever its rounding mode) and the canonical chain's d fused steps (d 2^-24 sum |q x|): together under 2 n 2^-23 ||q^|| ||x||
    const float n = (float)(((d + 31) / 32) * 32 + 2);
    dot = (dot + (2.0f * n * 1.1920929e-07f) * ((qr * xr) * up)) * up;
    float E = dot;
    if (metric_l2) {
        // key = max(0, fma(-2, dot, fl(xn + yn))): the same xn + yn on both sides, one rounding each of a value under (||q|| + ||x||)^2
        const float s = (qn + xr) * up;
        E = (2.0f * dot + 2.3841858e-07f * ((s * s) * up)) * up;
    }
    E = E * up + 1e-37f;  // (products that underflow fp32: d 2^-149)
    return E < 1e38f ? E : -1.f;
}
