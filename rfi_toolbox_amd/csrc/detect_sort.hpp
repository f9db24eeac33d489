// The 64-bit sort keys of the detector's box bookkeeping (detect_sample.hip, detect_infer.hip): an order-preserving image of a
// float32 score in the high word, a position in the low word, sorted ascending in LDS by a bitonic network.
#pragma once
#include <hip/hip_runtime.h>

namespace rfi {
namespace {

typedef unsigned long long u64;

// ascending bitonic sort of s[0 .. n) in LDS, n a power of two; every thread of the block takes part
__device__ void bitonic_sort(u64* s, int n) {
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < (n >> 1); t += blockDim.x) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int p = i | j;
                const bool up = (i & k) == 0;
                const u64 a = s[i], b = s[p];
                if ((a > b) == up) { s[i] = b; s[p] = a; }
            }
        }
    __syncthreads();
}

// order-preserving image of a float32 for DESCENDING order: smaller key = larger score; -0.0 and 0.0 tie
__device__ __forceinline__ unsigned desc_key(float s) {
    const unsigned bits = __float_as_uint((-s) + 0.0f);
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

inline int pow2_at_least(int n) {
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

}  // namespace
}  // namespace rfi
