// Confusion counts of "p > thresholds[k]" against a truth mask at EVERY threshold from one pass over the scores
// (evaluation/sweep.py, rfi_threshold_sweep, rfi_model_eval_sweep).  The arithmetic, pinned:
//   - an element's bin is b = the number of thresholds strictly below p (thresholds strictly increasing, so
//     p > thresholds[k]  <=>  k < b); a NaN p compares false everywhere and lands in bin 0;
//   - each element adds 1 to hist[2 * b + positive], positive = (truth != 0);
//   - tp[k] = sum_{b > k} hist[b][1], fp[k] = sum_{b > k} hist[b][0], fn[k] = P - tp[k], P = sum_b hist[b][1]
//     (threshold_sweep_counts below, on the host: K + 1 bins per group are not worth a launch).
// Everything is an integer count, so the result does not depend on the order of the adds, the grid or the layout.
//
// Memory bound: 4 B of score + 1 B (uint8) or 4 B (float32) of truth per element, read once.  A block walks its group
// in 16-byte score vectors (grid-stride); the up-to-3 elements before the first 16-byte-aligned score and after the last
// whole vector are read as scalars by block 0, so neither pointer needs any alignment beyond its element's: the truth
// vector is one 4- or 16-byte load when it happens to be aligned at the first score vector, else four scalar loads.
//
// Histogram: RFI probabilities are bimodal -- nearly every element is below the first threshold or above the last --
// so bins 0 and K never touch the LDS: each lane counts them in four registers, a wave adds them up with shuffles.
// The middle bins are u32 LDS atomics on one of R replicas of the histogram (a lane group of 256 / R lanes shares a
// replica; R = 16 while the replicas fit 32 KB, down to one per wave at K = 1024), found by a fixed-trip binary search
// over the thresholds in LDS.  At the end the block sums its replicas and adds the non-zero slots to the group's u64
// histogram in global memory.  A block's share of a group stays below 2^32 elements (launch_threshold_sweep).
#include <algorithm>
#include <cmath>

#include "kernels.hpp"

namespace rfi {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxReplicas = 16;
constexpr size_t kReplicaBudget = 32 * 1024;

__device__ __forceinline__ bool positive(uint8_t t) { return t != 0; }
__device__ __forceinline__ bool positive(float t) { return t != 0.0f; }

template <typename TT> struct Truth4;
template <> struct Truth4<uint8_t> { using type = uchar4; };
template <> struct Truth4<float> { using type = float4; };

// thr_dev: K thresholds; hist: per group 2 * (K + 1) u64 slots, zeroed; grid (blocks per group, groups)
template <bool LOGITS, typename TT>
__global__ void __launch_bounds__(kBlock) sweep_hist_kernel(const float* __restrict__ scores, const TT* __restrict__ truth,
                                                            int64_t group_elems, const float* __restrict__ thr_dev, int K,
                                                            int top_step, int replicas,
                                                            unsigned long long* __restrict__ hist) {
    extern __shared__ __align__(16) unsigned char smem[];
    float* thr = reinterpret_cast<float*>(smem);                                   // K floats, padded to 16 B
    unsigned* lh = reinterpret_cast<unsigned*>(smem + (((size_t)K * 4 + 15) & ~size_t(15)));
    const int S = 2 * (K + 1), tid = threadIdx.x;
    for (int i = tid; i < K; i += kBlock) thr[i] = thr_dev[i];
    for (int i = tid; i < replicas * S; i += kBlock) lh[i] = 0u;
    __syncthreads();

    const float t_first = thr[0], t_last = thr[K - 1];
    unsigned* mine = lh + (tid * replicas / kBlock) * S;
    unsigned lo0 = 0, lo1 = 0, hi0 = 0, hi1 = 0;                                   // bins 0 and K, truth 0 / 1
    auto add = [&](float x, bool pos) {
        const float p = LOGITS ? 1.0f / (1.0f + expf(-x)) : x;
        if (!(p > t_first)) {                                                      // (NaN too)
            lo0 += !pos;
            lo1 += pos;
        } else if (p > t_last) {
            hi0 += !pos;
            hi1 += pos;
        } else {                                                                   // 1 <= b <= K - 1
            int b = 0;
            for (int step = top_step; step > 0; step >>= 1)
                if (b + step <= K && thr[b + step - 1] < p) b += step;
            atomicAdd(&mine[2 * b + (pos ? 1 : 0)], 1u);
        }
    };

    const int64_t base = (int64_t)blockIdx.y * group_elems;
    const float* s = scores + base;
    const TT* t = truth + base;
    int64_t head = (int64_t)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(s) & 15u)) & 15u) / 4u);
    if (head > group_elems) head = group_elems;
    const int64_t nvec = (group_elems - head) / 4;
    const int tail = (int)(group_elems - head - 4 * nvec);
    const float4* s4 = reinterpret_cast<const float4*>(s + head);
    const TT* tb = t + head;
    using T4 = typename Truth4<TT>::type;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    if ((reinterpret_cast<uintptr_t>(tb) & (sizeof(T4) - 1)) == 0) {
        const T4* t4 = reinterpret_cast<const T4*>(tb);
#pragma unroll 2
        for (int64_t v = (int64_t)blockIdx.x * kBlock + tid; v < nvec; v += stride) {
            const float4 x = s4[v];
            const T4 y = t4[v];
            add(x.x, positive(y.x));
            add(x.y, positive(y.y));
            add(x.z, positive(y.z));
            add(x.w, positive(y.w));
        }
    } else {
#pragma unroll 2
        for (int64_t v = (int64_t)blockIdx.x * kBlock + tid; v < nvec; v += stride) {
            const float4 x = s4[v];
            const TT y0 = tb[4 * v], y1 = tb[4 * v + 1], y2 = tb[4 * v + 2], y3 = tb[4 * v + 3];
            add(x.x, positive(y0));
            add(x.y, positive(y1));
            add(x.z, positive(y2));
            add(x.w, positive(y3));
        }
    }
    if (blockIdx.x == 0) {                                                         // scalar head and tail (<= 3 each)
        if (tid < head) add(s[tid], positive(t[tid]));
        const int64_t t0 = head + 4 * nvec;
        if (tid < tail) add(s[t0 + tid], positive(t[t0 + tid]));
    }

#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo0 += __shfl_down(lo0, o, 64);
        lo1 += __shfl_down(lo1, o, 64);
        hi0 += __shfl_down(hi0, o, 64);
        hi1 += __shfl_down(hi1, o, 64);
    }
    if ((tid & 63) == 0) {                                                         // slots the loop above never touches
        atomicAdd(&lh[0], lo0);
        atomicAdd(&lh[1], lo1);
        atomicAdd(&lh[2 * K], hi0);
        atomicAdd(&lh[2 * K + 1], hi1);
    }
    __syncthreads();
    unsigned long long* gh = hist + (int64_t)blockIdx.y * S;
    for (int i = tid; i < S; i += kBlock) {
        unsigned sum = 0;
        for (int r = 0; r < replicas; ++r) sum += lh[r * S + i];
        if (sum) atomicAdd(&gh[i], (unsigned long long)sum);
    }
}

}  // namespace

void check_sweep_thresholds(const float* thr_host, int K) {
    RFI_REQUIRE(K >= 1 && K <= 1024, "threshold_sweep: 1 <= n_thresholds <= 1024");
    for (int k = 0; k < K; ++k)
        RFI_REQUIRE(std::isfinite(thr_host[k]) && (k == 0 || thr_host[k - 1] < thr_host[k]),
                    "threshold_sweep: thresholds must be finite and strictly increasing");
}

void launch_threshold_sweep(rfi_ctx* ctx, const float* scores, int kind, const void* truth, int truth_dtype,
                            int64_t n_groups, int64_t group_elems, const float* thr_dev, int K,
                            unsigned long long* hist) {
    RFI_REQUIRE(K >= 1 && K <= 1024, "threshold_sweep: 1 <= n_thresholds <= 1024");
    RFI_REQUIRE(n_groups >= 1 && n_groups <= 65535 && group_elems >= 1, "threshold_sweep: 1 .. 65535 non-empty groups");
    RFI_REQUIRE(kind == RFI_VALUES_LOGITS || kind == RFI_VALUES_PROBS, "threshold_sweep: kind must be logits or probabilities");
    RFI_REQUIRE(truth_dtype == RFI_U8 || truth_dtype == RFI_FLOAT32, "threshold_sweep: truth must be u8 or f32");
    const size_t tsz = truth_dtype == RFI_U8 ? 1 : 4;
    RFI_REQUIRE(reinterpret_cast<uintptr_t>(scores) % 4 == 0 && reinterpret_cast<uintptr_t>(truth) % tsz == 0,
                "threshold_sweep: pointers must be aligned to their element size");
    const size_t S = 2 * ((size_t)K + 1);
    ProfScope ps(ctx, FAM_METRICS, 0, (double)n_groups * (double)group_elems * (double)(4 + tsz));
    RFI_CHECK_HIP(hipMemsetAsync(hist, 0, (size_t)n_groups * S * sizeof(unsigned long long), ctx->stream));
    int replicas = kMaxReplicas;
    while (replicas > kBlock / 64 && (size_t)replicas * S * 4 > kReplicaBudget) replicas >>= 1;
    const size_t lds = (((size_t)K * 4 + 15) & ~size_t(15)) + (size_t)replicas * S * 4;
    int top_step = 1;
    while (top_step * 2 <= K) top_step *= 2;
    // ~2048 blocks in all, ~16 elements a thread; never 2^31 elements or more to a block (u32 LDS counters)
    int64_t bx = std::min(cdiv(group_elems, (int64_t)kBlock * 16), std::max<int64_t>(1, 2048 / n_groups));
    bx = std::max(bx, cdiv(group_elems, int64_t(1) << 31));
    RFI_REQUIRE(bx <= 0x7fffffff, "threshold_sweep: group too large for one launch");
    const dim3 grid((unsigned)bx, (unsigned)n_groups), block(kBlock);
    const bool logits = kind == RFI_VALUES_LOGITS;
    const uint8_t* t8 = static_cast<const uint8_t*>(truth);
    const float* tf = static_cast<const float*>(truth);
    if (truth_dtype == RFI_U8) {
        if (logits)
            hipLaunchKernelGGL((sweep_hist_kernel<true, uint8_t>), grid, block, lds, ctx->stream, scores, t8, group_elems,
                               thr_dev, K, top_step, replicas, hist);
        else
            hipLaunchKernelGGL((sweep_hist_kernel<false, uint8_t>), grid, block, lds, ctx->stream, scores, t8, group_elems,
                               thr_dev, K, top_step, replicas, hist);
    } else {
        if (logits)
            hipLaunchKernelGGL((sweep_hist_kernel<true, float>), grid, block, lds, ctx->stream, scores, tf, group_elems,
                               thr_dev, K, top_step, replicas, hist);
        else
            hipLaunchKernelGGL((sweep_hist_kernel<false, float>), grid, block, lds, ctx->stream, scores, tf, group_elems,
                               thr_dev, K, top_step, replicas, hist);
    }
    check_launch("threshold_sweep");
}

void threshold_sweep_counts(const unsigned long long* hist, int64_t n_groups, int K, int64_t* counts) {
    const size_t S = 2 * ((size_t)K + 1);
    for (int64_t g = 0; g < n_groups; ++g) {
        const unsigned long long* h = hist + (size_t)g * S;
        int64_t* c = counts + (size_t)g * K * 3;
        int64_t P = 0;
        for (int b = 0; b <= K; ++b) P += (int64_t)h[2 * b + 1];
        int64_t tp = 0, fp = 0;
        for (int k = K - 1; k >= 0; --k) {                 // bins b > k
            tp += (int64_t)h[2 * (k + 1) + 1];
            fp += (int64_t)h[2 * (k + 1)];
            c[3 * k] = tp;
            c[3 * k + 1] = fp;
            c[3 * k + 2] = P - tp;
        }
    }
}

}  // namespace rfi
