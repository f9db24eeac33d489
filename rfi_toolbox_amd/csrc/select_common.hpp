// Device helpers shared by the exact order-statistic kernels (flag_stats.hip, dataset_norm.hip, sumthreshold.hip,
// casa_flaggers.hip): the order-preserving integer image of a float for radix selection, |z| as NumPy computes it, and
// the fixed-order wave reductions.
#pragma once
#include <hip/hip_runtime.h>

namespace rfi {

typedef unsigned long long u64;

__device__ __forceinline__ unsigned okey(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ u64 okey(double f) {
    const u64 u = (u64)__double_as_longlong(f);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ float unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ double unkey(u64 k) {
    return __longlong_as_double((long long)((k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k));
}

__device__ __forceinline__ float fma_rn(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_rn(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float sqrt_rn(float a) { return __builtin_sqrtf(a); }
__device__ __forceinline__ double sqrt_rn(double a) { return __builtin_sqrt(a); }

// |re + i im| as NumPy's complex-abs loop computes it, in the input's precision:
// L = max(|re|,|im|), S = min(|re|,|im|), L * sqrt(fma(S/L, S/L, 1)); 0 for 0+0j, inf for an infinite part, else NaN
// for a NaN part.  (The preprocessing path's to_abs_f64_kernel uses hypot and is deliberately left alone.)
template <typename T>
__device__ __forceinline__ T cabs_np(T re, T im) {
    const T a = fabs(re), b = fabs(im);
    if (isinf(a) || isinf(b)) return (T)INFINITY;
    if (isnan(a) || isnan(b)) return a + b;
    const T L = a > b ? a : b, S = a > b ? b : a;
    if (L == (T)0) return (T)0;
    const T r = S / L;
    return L * sqrt_rn(fma_rn(r, r, (T)1));
}

// wave reductions in a fixed order (xor butterfly; every lane gets the result): the statistics are reproducible bit for bit
__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ u64 wave_usum(u64 v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_isum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace rfi
