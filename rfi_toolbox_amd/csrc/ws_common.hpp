// What is specific to the wave-specialised float32 (3 x bf16) kernels (conv_ws.hip, gemm_ws.hip, ...): the diagnostic
// stamps, the bare barrier and the vmcnt wait.  The arithmetic itself is bf16_mma.hpp.
#pragma once
#include "bf16_mma.hpp"
#include "planes.hpp"

// RFI_DIAG_STAMPS builds (tools/build_diag.sh, never shipped): per-wave cycle sums of the phases of a kernel's main loop
#ifdef RFI_DIAG_STAMPS
#define WS_T(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#define WS_ACC(i, a_, b_) st_[i] += (b_) - (a_)
#else
#define WS_T(v)
#define WS_ACC(i, a_, b_)
#endif

namespace rfi {
namespace ws {

// a bare s_barrier: no s_waitcnt in front of it (__syncthreads() would also wait for the consumers' output stores and the
// producers' prefetched loads); the "memory" clobber keeps the compiler from moving LDS accesses across it
__device__ __forceinline__ void wg_barrier() { asm volatile("s_barrier" ::: "memory"); }

// s_waitcnt vmcnt(n) as the BUILTIN: the compiler's own wait bookkeeping sees it (an asm wait it would not), so the LDS
// writes that follow are not preceded by a conservative vmcnt(0) for the LDS-DMA issued before it
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    __builtin_amdgcn_s_waitcnt((N & 0xf) | (0x7 << 4) | (0xf << 8) | ((N >> 4) << 14));     // expcnt, lgkmcnt: no wait
}

}  // namespace ws
}  // namespace rfi
