// Philox4x32-10 (Salmon et al., Random123): the one counter-based generator of the library.  The synthetic generator, the
// simulator, the detector's samplers and the augmentation draw from it, and oracle/synth_ref.philox4x32_10 evaluates the
// same stream on the host; include/rfi_hip.h documents the counter and key conventions of each user.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace rfi {

struct U4 { unsigned x, y, z, w; };

// counter c, key (k0, k1) -> four 32-bit words.  __host__ too: rfi_augment_params draws on the host.
// UNROLL = false leaves the unrolling of the ten rounds to the compiler: for augment.hip, which draws three blocks on ONE lane
// per workgroup, where thirty rounds of straight-line code buy nothing and cost scalar registers
template <bool UNROLL = true>
__host__ __device__ __forceinline__ U4 philox4x32_10(U4 c, unsigned k0, unsigned k1) {
    auto round = [&]() {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c.z;
        const U4 n{(unsigned)(p1 >> 32) ^ c.y ^ k0, (unsigned)p1, (unsigned)(p0 >> 32) ^ c.w ^ k1, (unsigned)p0};
        c = n;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    };
    if constexpr (UNROLL) {
#pragma unroll
        for (int i = 0; i < 10; ++i) round();
    } else {
        for (int i = 0; i < 10; ++i) round();
    }
    return c;
}

}  // namespace rfi
