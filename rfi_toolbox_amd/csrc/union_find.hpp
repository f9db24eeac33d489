// Union-find on an int32 parent array whose roots are the smallest index of their set (components.hip, instance_stitch.hip):
// a union hangs the larger root under the smaller one with atomicMin, so parent[p] <= p always, parents only ever decrease
// and the result does not depend on the order in which the unions arrive.  Whether a union succeeded is decided from the value
// atomicMin RETURNED, never from a load: on gfx950 every XCD has an L2 of its own, and a load may see an older parent while
// another XCD is merging.  That is harmless to find_root -- an older parent is still an ancestor, the walk merely starts
// higher up.  A plain load (each one issued) serves LDS, which is coherent inside the workgroup, and global memory that no
// running launch writes; a launch that merges in global memory reads with agent-scope loads.
#pragma once
#include <hip/hip_runtime.h>

namespace rfi {

struct PlainLoad {
    __device__ __forceinline__ int operator()(const int* p) const { return *reinterpret_cast<const volatile int*>(p); }
};
struct AgentLoad {
    __device__ __forceinline__ int operator()(const int* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
template <class Load> __device__ __forceinline__ int find_root(const int* L, int a, Load ld) {
    // terminates: a non-root's parent is smaller than itself, so `a` strictly decreases
    for (int p = ld(L + a); p != a; p = ld(L + a)) a = p;
    return a;
}
template <class Load> __device__ __forceinline__ void unite(int* L, int a, int b, Load ld) {
    // terminates: a pass that does not end the loop replaces the larger of (a, b) by the value atomicMin returned, which is
    // smaller than it (somebody else hung that root lower in the meantime); a + b strictly decreases
    for (;;) {
        a = find_root(L, a, ld);
        b = find_root(L, b, ld);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(L + b, a);        // b was a root iff the word still held b
        if (old == b) return;
        b = old;
    }
}

}  // namespace rfi
