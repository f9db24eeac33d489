// Input normalisation of 8-channel RFI data (rfi_toolbox/datasets/rfi_mask_dataset.py:99-156 and
// scripts/normalize_rfi_data.py::normalize_array): the statistics of whole populations of real scalars, and the
// streaming transform dst = (src - centre) / scale with the layout conversion fused.
//
// Statistics.  A population is `seg` consecutive scalars of the concatenation of the call's chunks (dataset mode:
// one population, every chunk; per-sample mode: one chunk cut into equal segments).  Per population: min, max,
// the number of non-finite values, fp64 mean and population variance, and six order statistics (the two brackets
// of the median, the 25 % and the 75 % quantile; the ranks come from the host).
//
//   pass 0     sums, min / max, non-finite count, histogram of the first radix digit
//   control    one workgroup per population: fixed-order reduction of the partial sums; picks each rank's digit
//   pass 1     squared deviations about the mean + the second digit, for all six ranks of all populations at once
//   pass 2..   one digit each (3 passes in all for float32, 6 for float64); not run when no quantile is wanted
//
// Order statistics are exact: radix selection on the order-preserving integer image of T, kDigit bits at a time
// (as flag_stats.hip).  Sums are per SUM TILE: 8192 consecutive scalars of the population, owned by one wave, lane l
// adding its elements l, l + 64, ... in order, then a fixed xor butterfly; the tile sums are then added by one
// workgroup in a fixed order.  A tile is a range of population indices, not of memory: a tile that straddles two chunks is read
// from both, so every result is independent of the chunking and of the launch geometry, bit for bit.  Histogram
// counts are integers (LDS atomics, then one global integer atomic per non-zero bin); nothing is a floating-point
// atomic.
//
// Apply.  A lane owns one pixel: it reads the pixel's 8 scalars (8 planes, 4 complex planes, or 8 contiguous),
// forms (double(x) - centre) / scale in fp64, rounds once to float32 and writes 8 planes or 32 contiguous bytes.
//
// Validity-aware counterparts (prior flags and non-finite values; the last section of this file): the invalid map, one
// byte per visibility, the same statistics over the valid scalars only, and the apply that writes `fill` where invalid.
#include "kernels.hpp"
#include "select_common.hpp"

namespace rfi {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kDigit = 11, kBins = 1 << kDigit;
constexpr int kSlots = 6;                        // slot 2 q + j: q 0 median / 1 25 % / 2 75 %; j 0 lower, 1 upper bracket
constexpr int kUnroll = 8;
constexpr int kWaveTile = 64 * kUnroll;          // scalars a wave loads at a time
constexpr int kSuper = 16;                       // wave tiles per partial sum
constexpr int kSumTile = kWaveTile * kSuper;     // scalars per partial sum
constexpr int kMaxBlocks = 2048;                 // 8 workgroups per CU on 256 CUs

template <typename T> struct KeyOf;
template <> struct KeyOf<float> { typedef unsigned K; static constexpr int bits = 32; };
template <> struct KeyOf<double> { typedef u64 K; static constexpr int bits = 64; };

template <typename T> __host__ __device__ constexpr int npass() { return (KeyOf<T>::bits + kDigit - 1) / kDigit; }
template <typename T> __device__ __forceinline__ int digit_shift(int p) {
    const int s = KeyOf<T>::bits - kDigit * (p + 1);
    return s > 0 ? s : 0;
}

struct NsState {                                 // one per population (zeroed by the host before pass 0)
    u64 nminkey, maxkey, nonfinite;              // nminkey: max of ~key, so that zero is the identity of both
    double mean, var;
    u64 prefix[kSlots], rank[kSlots];
    int alias[kSlots];                           // slot whose histogram this slot reads (equal prefixes share one)
};
struct NsArgs {
    const norm_chunk* chunks;                    // n_chunks + 1 entries; the last one holds the total
    int n_chunks;
    int pops;
    int last_pass;                               // the pass after which the record is written (1 without quantiles)
    int64_t seg;                                 // scalars per population
    int64_t wtiles;                              // sum tiles per population
    u64 rank[kSlots];
    double* partial;                             // [pops][wtiles]
    u64* ghist;                                  // [pops][kSlots][kBins]
    NsState* st;
    rfi_norm_stats* out;
};

// the `len` scalars from index g0 of the concatenation, lane l taking l, l + 64, ...; lanes past `len` get 0
template <typename T>
__device__ __forceinline__ void load_tile(const NsArgs& a, int64_t g0, int len, int lane, T (&x)[kUnroll]) {
    int c = 0;
    if (a.n_chunks > 1) {                        // last chunk starting at or before g0 (wave-uniform)
        int lo = 0, hi = a.n_chunks - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.chunks[mid].start <= g0) lo = mid; else hi = mid - 1;
        }
        c = lo;
    }
    if (g0 + len <= a.chunks[c + 1].start) {     // the whole tile lies in chunk c
        const T* p = static_cast<const T*>(a.chunks[c].ptr) + (g0 - a.chunks[c].start);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int i = lane + 64 * u;
            x[u] = i < len ? p[i] : (T)0;
        }
    } else {                                     // the tile straddles chunks: each element finds its own
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int i = lane + 64 * u;
            x[u] = (T)0;
            if (i < len) {
                const int64_t g = g0 + i;
                while (c + 1 < a.n_chunks && g >= a.chunks[c + 1].start) ++c;
                x[u] = static_cast<const T*>(a.chunks[c].ptr)[g - a.chunks[c].start];
            }
        }
    }
}

// MODE 0: sums, extrema, non-finite count, first digit (one histogram).  MODE 1: squared deviations + a digit.
// MODE 2: a digit only.  grid (blocks, pops); every wave walks wave tiles of its population.
template <typename T, int MODE>
__global__ __launch_bounds__(kBlock) void ns_pass_kernel(NsArgs a, int pass) {
    typedef typename KeyOf<T>::K K;
    constexpr int NS = MODE == 0 ? 1 : kSlots;
    __shared__ unsigned lh[NS][kBins];
    const int pop = blockIdx.y;
    NsState* st = a.st + pop;
    bool built[NS];
    K prefix[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        built[s] = MODE == 0 || st->alias[s] == s;
        prefix[s] = MODE == 0 ? (K)0 : (K)st->prefix[s];
    }
    const int hi = KeyOf<T>::bits - kDigit * pass, sh = digit_shift<T>(pass);
    const K mask = pass == 0 ? (K)0 : (K)(~(K)0 << hi);
    const unsigned dmask = (1u << (hi - sh)) - 1u;
    const double mean = MODE == 1 ? st->mean : 0.0;
#pragma unroll
    for (int s = 0; s < NS; ++s)
        if (built[s])
            for (int b = threadIdx.x; b < kBins; b += kBlock) lh[s][b] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    T mn = (T)INFINITY, mx = (T)-INFINITY;
    u64 nf = 0;
    for (int64_t wt = (int64_t)blockIdx.x * kWaves + w; wt < a.wtiles; wt += (int64_t)gridDim.x * kWaves) {
        double s = 0.0;
        for (int j = 0; j < kSuper; ++j) {
            const int64_t off = wt * kSumTile + (int64_t)j * kWaveTile;
            const int64_t left = a.seg - off;
            if (left <= 0) break;
            const int len = left < kWaveTile ? (int)left : kWaveTile;
            T x[kUnroll];
            load_tile<T>(a, (int64_t)pop * a.seg + off, len, lane, x);
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const bool ok = lane + 64 * u < len;
                if (MODE == 0) {
                    s += (double)x[u];
                    if (ok) {
                        if (x[u] < mn) mn = x[u];
                        if (x[u] > mx) mx = x[u];
                        nf += isfinite(x[u]) ? 0 : 1;
                    }
                } else if (MODE == 1) {
                    const double d = ok ? (double)x[u] - mean : 0.0;
                    s += d * d;
                }
                if (ok) {
                    const K k = okey(x[u]);
#pragma unroll
                    for (int q = 0; q < NS; ++q)
                        if (built[q] && (k & mask) == prefix[q]) atomicAdd(&lh[q][(unsigned)(k >> sh) & dmask], 1u);
                }
            }
        }
        if (MODE != 2) {
            s = wave_sum(s);
            if (lane == 0) a.partial[(int64_t)pop * a.wtiles + wt] = s;
        }
    }
    if (MODE == 0) {
        const double lo = wave_min((double)mn), up = wave_max((double)mx);
        nf = wave_usum(nf);
        if (lane == 0) {
            if (lo <= up) {                      // (false for a wave that saw nothing, or nothing but NaN)
                atomicMax(&st->nminkey, ~okey(lo));
                atomicMax(&st->maxkey, okey(up));
            }
            if (nf) atomicAdd(&st->nonfinite, nf);
        }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (!built[s]) continue;
        u64* g = a.ghist + ((size_t)pop * kSlots + s) * kBins;
        for (int b = threadIdx.x; b < kBins; b += kBlock) {
            const unsigned c = lh[s][b];
            if (c) atomicAdd(&g[b], (u64)c);
        }
    }
}

// sum of the population's tile sums in a fixed order: thread t adds tiles t, t + kBlock, ...; then a fixed tree
__device__ double reduce_partials(const double* p, int64_t n) {
    __shared__ double sh[kBlock];
    double r = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kBlock) r += p[i];
    sh[threadIdx.x] = r;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    const double out = sh[0];
    __syncthreads();
    return out;
}

// digit of the bin holding 0-based rank `rank` of histogram h; *below = count in the bins before it
__device__ void find_digit(const u64* h, u64 rank, int* digit, u64* below) {
    constexpr int per = kBins / kBlock;
    __shared__ u64 part[kBlock];
    u64 loc[per], sum = 0;
#pragma unroll
    for (int k = 0; k < per; ++k) {
        loc[k] = h[threadIdx.x * per + k];
        sum += loc[k];
    }
    part[threadIdx.x] = sum;
    if (threadIdx.x == 0) { *digit = 0; *below = 0; }
    __syncthreads();
    for (int o = 1; o < kBlock; o <<= 1) {                   // inclusive scan
        const u64 add = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    const u64 incl = part[threadIdx.x], excl = incl - sum;
    if (rank >= excl && rank < incl) {
        u64 c = excl;
#pragma unroll
        for (int k = 0; k < per; ++k) {
            if (rank >= c && rank < c + loc[k]) {
                *digit = threadIdx.x * per + k;
                *below = c;
            }
            c += loc[k];
        }
    }
    __syncthreads();
}

// one workgroup per population, after pass `pass`: sums -> mean (pass 0) / variance (pass 1); every rank's digit;
// the histograms are cleared for the next pass; the last pass writes the record
template <typename T>
__global__ __launch_bounds__(kBlock) void ns_control_kernel(NsArgs a, int pass) {
    typedef typename KeyOf<T>::K K;
    __shared__ int s_digit, s_alias[kSlots];
    __shared__ u64 s_below, s_rank[kSlots];
    const int pop = blockIdx.x;
    NsState* st = a.st + pop;                                // written by thread 0 only; the others read LDS copies
    if (pass <= 1) {
        const double r = reduce_partials(a.partial + (int64_t)pop * a.wtiles, a.wtiles);
        if (threadIdx.x == 0) {
            if (pass == 0) st->mean = r / (double)a.seg;
            else st->var = r / (double)a.seg;
        }
    }
    if (threadIdx.x == 0)
        for (int s = 0; s < kSlots; ++s) {
            s_alias[s] = pass == 0 ? 0 : st->alias[s];
            s_rank[s] = pass == 0 ? a.rank[s] : st->rank[s];
        }
    __syncthreads();
    const int sh = digit_shift<T>(pass);
    u64* gh = a.ghist + (size_t)pop * kSlots * kBins;
    for (int s = 0; s < kSlots; ++s) {
        find_digit(gh + (size_t)s_alias[s] * kBins, s_rank[s], &s_digit, &s_below);
        if (threadIdx.x == 0) {
            st->prefix[s] = (pass == 0 ? 0 : st->prefix[s]) | ((u64)s_digit << sh);
            st->rank[s] = s_rank[s] - s_below;
        }
        __syncthreads();
    }
    for (int b = threadIdx.x; b < kSlots * kBins; b += kBlock) gh[b] = 0;
    if (threadIdx.x == 0) {
        for (int s = 0; s < kSlots; ++s) {
            int al = s;
            for (int r = s - 1; r >= 0; --r)
                if (st->prefix[r] == st->prefix[s]) al = r;
            st->alias[s] = al;
        }
        if (pass == a.last_pass) {
            rfi_norm_stats o;
            o.count = a.seg;
            o.nonfinite = (int64_t)st->nonfinite;
            o.min = unkey(~st->nminkey);
            o.max = unkey(st->maxkey);
            o.mean = st->mean;
            o.var = st->var;
            const bool have = a.last_pass == npass<T>() - 1;
            for (int s = 0; s < kSlots; ++s)
                o.q[s >> 1][s & 1] = have ? (double)unkey((K)st->prefix[s]) : __longlong_as_double(0x7ff8000000000000ll);
            a.out[pop] = o;
        }
    }
}

template <typename T>
void run_stats(rfi_ctx* ctx, const NsArgs& a) {
    const int64_t groups = cdiv(a.wtiles, kWaves);            // a workgroup's four waves take four sum tiles at a time
    const int64_t cap = std::max<int64_t>(1, kMaxBlocks / a.pops);
    const dim3 g((unsigned)std::min(groups, cap), (unsigned)a.pops), b(kBlock);
    hipLaunchKernelGGL((ns_pass_kernel<T, 0>), g, b, 0, ctx->stream, a, 0);
    check_launch("norm_stats_pass0");
    hipLaunchKernelGGL(ns_control_kernel<T>, dim3(a.pops), b, 0, ctx->stream, a, 0);
    hipLaunchKernelGGL((ns_pass_kernel<T, 1>), g, b, 0, ctx->stream, a, 1);
    hipLaunchKernelGGL(ns_control_kernel<T>, dim3(a.pops), b, 0, ctx->stream, a, 1);
    for (int p = 2; p <= a.last_pass; ++p) {
        hipLaunchKernelGGL((ns_pass_kernel<T, 2>), g, b, 0, ctx->stream, a, p);
        hipLaunchKernelGGL(ns_control_kernel<T>, dim3(a.pops), b, 0, ctx->stream, a, p);
    }
    check_launch("norm_stats");
}

constexpr size_t up256(size_t b) { return (b + 255) / 256 * 256; }
size_t hist_bytes(int pops) { return up256((size_t)pops * kSlots * kBins * sizeof(u64)); }
size_t state_bytes(int pops) { return up256((size_t)pops * sizeof(NsState)); }
size_t partial_bytes(int pops, int64_t seg) { return up256((size_t)pops * (size_t)cdiv(seg, kSumTile) * sizeof(double)); }

// ---------------------------------------------------------------- apply
enum { SRC_PLANAR = 0, SRC_COMPLEX = 1, SRC_NHWC = 2 };

template <typename S> struct alignas(2 * sizeof(S)) Pair { S x, y; };
template <typename S> struct alignas(16) Quad;                // 16 bytes of S
template <> struct alignas(16) Quad<float> { float v[4]; };
template <> struct alignas(16) Quad<double> { double v[2]; };

// src and dst may be the same buffer (same dtype and layout only): a lane reads its pixel's 8 values before it
// writes the same 8 places, so neither pointer is __restrict__
template <typename S, int SRC, bool DNHWC>
__global__ __launch_bounds__(kBlock) void ns_apply_kernel(const S* src, float* dst, int64_t total, int64_t px, double centre,
                                                          double scale, const double* params) {
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= total) return;
    const int64_t n = gid / px, p = gid - n * px;
    if (params) {
        centre = params[2 * n];
        scale = params[2 * n + 1];
    }
    S v[8];
    if constexpr (SRC == SRC_PLANAR) {
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = src[(n * 8 + c) * px + p];
    } else if constexpr (SRC == SRC_COMPLEX) {
        const Pair<S>* q = reinterpret_cast<const Pair<S>*>(src);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const Pair<S> z = q[(n * 4 + c) * px + p];
            v[2 * c] = z.x;
            v[2 * c + 1] = z.y;
        }
    } else {
        constexpr int per = 16 / sizeof(S);
        const Quad<S>* q = reinterpret_cast<const Quad<S>*>(src + gid * 8);
#pragma unroll
        for (int c = 0; c < 8 / per; ++c) {
            const Quad<S> z = q[c];
#pragma unroll
            for (int k = 0; k < per; ++k) v[c * per + k] = z.v[k];
        }
    }
    float o[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = norm_value(v[c], centre, scale);
    if constexpr (DNHWC) {
        Quad<float>* q = reinterpret_cast<Quad<float>*>(dst + gid * 8);
        q[0] = Quad<float>{{o[0], o[1], o[2], o[3]}};
        q[1] = Quad<float>{{o[4], o[5], o[6], o[7]}};
    } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) dst[(n * 8 + c) * px + p] = o[c];
    }
}

template <typename S, int SRC>
void run_apply(rfi_ctx* ctx, const void* src, float* dst, int64_t total, int64_t px, double centre, double scale,
               const double* params, bool dnhwc) {
    const dim3 g((unsigned)cdiv(total, kBlock)), b(kBlock);
    if (dnhwc)
        hipLaunchKernelGGL((ns_apply_kernel<S, SRC, true>), g, b, 0, ctx->stream, static_cast<const S*>(src), dst, total, px,
                           centre, scale, params);
    else
        hipLaunchKernelGGL((ns_apply_kernel<S, SRC, false>), g, b, 0, ctx->stream, static_cast<const S*>(src), dst, total, px,
                           centre, scale, params);
    check_launch("norm_apply");
}

// ---------------------------------------------------------------- validity-aware statistics, map and apply
// (include/rfi_hip.h, "validity-aware 8-channel input").  The kernels above are left as they are; these share their
// device functions (load_tile, okey, reduce_partials, find_digit, norm_value).  A scalar counts when the byte of its
// visibility in the chunk's invalid map is zero; an invalid scalar adds 0.0 to its lane's sum, like a lane past the
// tile's end, so that a population without an invalid scalar gives ns_pass_kernel's sums bit for bit.
struct NvState {                                 // NsState plus the population's valid count
    u64 nminkey, maxkey, nonfinite, count;
    double mean, var;
    u64 prefix[kSlots], rank[kSlots];
    int alias[kSlots];
};
struct NvArgs {
    NsArgs s;                                    // (its st and rank are not used: the ranks are formed on the device)
    const valid_chunk* vc;                       // n_chunks entries, beside s.chunks
    NvState* st;
};

// is scalar i of a chunk valid: the byte of its visibility in the chunk's (n, 4, px) map
__device__ __forceinline__ bool scalar_valid(const valid_chunk& v, int64_t i) {
    int64_t b;
    if (v.form == RFI_VALID_SRC_COMPLEX) {
        b = i >> 1;
    } else {
        const int64_t per = 8 * v.px, n = i / per, r = i - n * per;
        int64_t ch, p;
        if (v.form == RFI_VALID_SRC_PLANAR) { ch = r / v.px; p = r - ch * v.px; }
        else { ch = r & 7; p = r >> 3; }
        b = (n * 4 + (ch >> 1)) * v.px + p;
    }
    return v.map[b] == 0;
}

// load_tile's walk over the chunks, for the validity of the same `len` scalars; lanes past `len` get false
__device__ __forceinline__ void load_valid(const NvArgs& a, int64_t g0, int len, int lane, bool (&ok)[kUnroll]) {
    const norm_chunk* ch = a.s.chunks;
    int c = 0;
    if (a.s.n_chunks > 1) {
        int lo = 0, hi = a.s.n_chunks - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (ch[mid].start <= g0) lo = mid; else hi = mid - 1;
        }
        c = lo;
    }
    if (g0 + len <= ch[c + 1].start) {           // the whole tile lies in chunk c: its record is wave-uniform
        const valid_chunk v = a.vc[c];
        const int64_t i0 = g0 - ch[c].start;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int i = lane + 64 * u;
            ok[u] = i < len && scalar_valid(v, i0 + i);
        }
        return;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        const int i = lane + 64 * u;
        ok[u] = false;
        if (i < len) {
            const int64_t g = g0 + i;
            while (c + 1 < a.s.n_chunks && g >= ch[c + 1].start) ++c;
            ok[u] = scalar_valid(a.vc[c], g - ch[c].start);
        }
    }
}

// ns_pass_kernel over the valid scalars only; MODE 0 also counts them
template <typename T, int MODE>
__global__ __launch_bounds__(kBlock) void nv_pass_kernel(NvArgs a, int pass) {
    typedef typename KeyOf<T>::K K;
    constexpr int NS = MODE == 0 ? 1 : kSlots;
    __shared__ unsigned lh[NS][kBins];
    const int pop = blockIdx.y;
    NvState* st = a.st + pop;
    bool built[NS];
    K prefix[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        built[s] = MODE == 0 || st->alias[s] == s;
        prefix[s] = MODE == 0 ? (K)0 : (K)st->prefix[s];
    }
    const int hi = KeyOf<T>::bits - kDigit * pass, sh = digit_shift<T>(pass);
    const K mask = pass == 0 ? (K)0 : (K)(~(K)0 << hi);
    const unsigned dmask = (1u << (hi - sh)) - 1u;
    const double mean = MODE == 1 ? st->mean : 0.0;
#pragma unroll
    for (int s = 0; s < NS; ++s)
        if (built[s])
            for (int b = threadIdx.x; b < kBins; b += kBlock) lh[s][b] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    T mn = (T)INFINITY, mx = (T)-INFINITY;
    u64 nf = 0, cnt = 0;
    for (int64_t wt = (int64_t)blockIdx.x * kWaves + w; wt < a.s.wtiles; wt += (int64_t)gridDim.x * kWaves) {
        double s = 0.0;
        for (int j = 0; j < kSuper; ++j) {
            const int64_t off = wt * kSumTile + (int64_t)j * kWaveTile;
            const int64_t left = a.s.seg - off;
            if (left <= 0) break;
            const int len = left < kWaveTile ? (int)left : kWaveTile;
            T x[kUnroll];
            bool ok[kUnroll];
            load_tile<T>(a.s, (int64_t)pop * a.s.seg + off, len, lane, x);
            load_valid(a, (int64_t)pop * a.s.seg + off, len, lane, ok);
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                if (MODE == 0) {
                    s += ok[u] ? (double)x[u] : 0.0;
                    if (ok[u]) {
                        if (x[u] < mn) mn = x[u];
                        if (x[u] > mx) mx = x[u];
                        nf += isfinite(x[u]) ? 0 : 1;
                        cnt += 1;
                    }
                } else if (MODE == 1) {
                    const double d = ok[u] ? (double)x[u] - mean : 0.0;
                    s += d * d;
                }
                if (ok[u]) {
                    const K k = okey(x[u]);
#pragma unroll
                    for (int q = 0; q < NS; ++q)
                        if (built[q] && (k & mask) == prefix[q]) atomicAdd(&lh[q][(unsigned)(k >> sh) & dmask], 1u);
                }
            }
        }
        if (MODE != 2) {
            s = wave_sum(s);
            if (lane == 0) a.s.partial[(int64_t)pop * a.s.wtiles + wt] = s;
        }
    }
    if (MODE == 0) {
        const double lo = wave_min((double)mn), up = wave_max((double)mx);
        nf = wave_usum(nf);
        cnt = wave_usum(cnt);
        if (lane == 0) {
            if (lo <= up) {
                atomicMax(&st->nminkey, ~okey(lo));
                atomicMax(&st->maxkey, okey(up));
            }
            if (nf) atomicAdd(&st->nonfinite, nf);
            if (cnt) atomicAdd(&st->count, cnt);
        }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (!built[s]) continue;
        u64* g = a.s.ghist + ((size_t)pop * kSlots + s) * kBins;
        for (int b = threadIdx.x; b < kBins; b += kBlock) {
            const unsigned c = lh[s][b];
            if (c) atomicAdd(&g[b], (u64)c);
        }
    }
}

// rfi_norm_bracket's arithmetic (api.cpp, norm_bracket) on the device: one fp64 product, floor, two integer ranks
__device__ __forceinline__ void bracket_ranks(u64 count, double q, u64* r) {
    const double v = q * (double)((int64_t)count - 1), f = floor(v);
    const int64_t lo = (int64_t)f, up = lo + 1 < (int64_t)count - 1 ? lo + 1 : (int64_t)count - 1;
    r[0] = (u64)lo;
    r[1] = (u64)up;
}

// ns_control_kernel with the mean, the variance and the six ranks taken from the population's own valid count
template <typename T>
__global__ __launch_bounds__(kBlock) void nv_control_kernel(NvArgs a, int pass) {
    typedef typename KeyOf<T>::K K;
    __shared__ int s_digit, s_alias[kSlots];
    __shared__ u64 s_below, s_rank[kSlots];
    const int pop = blockIdx.x;
    NvState* st = a.st + pop;
    if (pass <= 1) {
        const double r = reduce_partials(a.s.partial + (int64_t)pop * a.s.wtiles, a.s.wtiles);
        if (threadIdx.x == 0) {
            if (pass == 0) st->mean = r / (double)st->count;
            else st->var = r / (double)st->count;
        }
    }
    if (threadIdx.x == 0) {
        u64 fresh[kSlots] = {0, 0, 0, 0, 0, 0};
        if (pass == 0 && st->count) {
            bracket_ranks(st->count, 0.5, fresh + 0);
            bracket_ranks(st->count, 0.25, fresh + 2);
            bracket_ranks(st->count, 0.75, fresh + 4);
        }
        for (int s = 0; s < kSlots; ++s) {
            s_alias[s] = pass == 0 ? 0 : st->alias[s];
            s_rank[s] = pass == 0 ? fresh[s] : st->rank[s];
        }
    }
    __syncthreads();
    const int sh = digit_shift<T>(pass);
    u64* gh = a.s.ghist + (size_t)pop * kSlots * kBins;
    for (int s = 0; s < kSlots; ++s) {
        find_digit(gh + (size_t)s_alias[s] * kBins, s_rank[s], &s_digit, &s_below);
        if (threadIdx.x == 0) {
            st->prefix[s] = (pass == 0 ? 0 : st->prefix[s]) | ((u64)s_digit << sh);
            st->rank[s] = s_rank[s] - s_below;
        }
        __syncthreads();
    }
    for (int b = threadIdx.x; b < kSlots * kBins; b += kBlock) gh[b] = 0;
    if (threadIdx.x == 0) {
        for (int s = 0; s < kSlots; ++s) {
            int al = s;
            for (int r = s - 1; r >= 0; --r)
                if (st->prefix[r] == st->prefix[s]) al = r;
            st->alias[s] = al;
        }
        if (pass == a.s.last_pass) {
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            const bool any = st->count != 0;
            rfi_norm_stats o;
            o.count = (int64_t)st->count;
            o.nonfinite = (int64_t)st->nonfinite;
            o.min = any ? unkey(~st->nminkey) : nan;
            o.max = any ? unkey(st->maxkey) : nan;
            o.mean = any ? st->mean : nan;
            o.var = any ? st->var : nan;
            const bool have = any && a.s.last_pass == npass<T>() - 1;
            for (int s = 0; s < kSlots; ++s) o.q[s >> 1][s & 1] = have ? (double)unkey((K)st->prefix[s]) : nan;
            a.s.out[pop] = o;
        }
    }
}

template <typename T>
void run_valid_stats(rfi_ctx* ctx, const NvArgs& a) {
    const int64_t groups = cdiv(a.s.wtiles, kWaves);
    const int64_t cap = std::max<int64_t>(1, kMaxBlocks / a.s.pops);
    const dim3 g((unsigned)std::min(groups, cap), (unsigned)a.s.pops), b(kBlock);
    hipLaunchKernelGGL((nv_pass_kernel<T, 0>), g, b, 0, ctx->stream, a, 0);
    check_launch("valid_stats_pass0");
    hipLaunchKernelGGL(nv_control_kernel<T>, dim3(a.s.pops), b, 0, ctx->stream, a, 0);
    hipLaunchKernelGGL((nv_pass_kernel<T, 1>), g, b, 0, ctx->stream, a, 1);
    hipLaunchKernelGGL(nv_control_kernel<T>, dim3(a.s.pops), b, 0, ctx->stream, a, 1);
    for (int p = 2; p <= a.s.last_pass; ++p) {
        hipLaunchKernelGGL((nv_pass_kernel<T, 2>), g, b, 0, ctx->stream, a, p);
        hipLaunchKernelGGL(nv_control_kernel<T>, dim3(a.s.pops), b, 0, ctx->stream, a, p);
    }
    check_launch("valid_stats");
}

size_t vstate_bytes(int pops) { return up256((size_t)pops * sizeof(NvState)); }

// the 8 scalars of pixel p of sample n (ns_apply_kernel's three source forms)
template <typename S, int SRC>
__device__ __forceinline__ void load_pixel(const S* src, int64_t n, int64_t p, int64_t px, S (&v)[8]) {
    if constexpr (SRC == SRC_PLANAR) {
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = src[(n * 8 + c) * px + p];
    } else if constexpr (SRC == SRC_COMPLEX) {
        const Pair<S>* q = reinterpret_cast<const Pair<S>*>(src);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const Pair<S> z = q[(n * 4 + c) * px + p];
            v[2 * c] = z.x;
            v[2 * c + 1] = z.y;
        }
    } else {
        constexpr int per = 16 / sizeof(S);
        const Quad<S>* q = reinterpret_cast<const Quad<S>*>(src + (n * px + p) * 8);
#pragma unroll
        for (int c = 0; c < 8 / per; ++c) {
            const Quad<S> z = q[c];
#pragma unroll
            for (int k = 0; k < per; ++k) v[c * per + k] = z.v[k];
        }
    }
}

// grid (pixel blocks, samples): a lane owns one pixel at a time, reads its 8 scalars and up to 4 flag bytes once and
// writes one byte per polarisation; the sample's invalid count is one integer atomic per workgroup (the grid is capped
// and strides over the pixels: one atomic per wave of 64 pixels, all of a sample on one address, cost more than the pass)
template <typename S, int SRC>
__global__ __launch_bounds__(kBlock) void nv_map_kernel(const S* src, const uint8_t* flags, int64_t fsample, int64_t fpol,
                                                        int64_t px, uint8_t* map, unsigned long long* counts) {
    __shared__ u64 s_bad[kWaves];
    const int64_t n = blockIdx.y;
    u64 bad = 0;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < px; p += (int64_t)gridDim.x * kBlock) {
        S v[8];
        load_pixel<S, SRC>(src, n, p, px, v);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const bool flagged = flags && flags[n * fsample + c * fpol + p] != 0;
            const bool inv = flagged || !isfinite(v[2 * c]) || !isfinite(v[2 * c + 1]);
            map[(n * 4 + c) * px + p] = inv ? 1 : 0;
            bad += inv ? 1 : 0;
        }
    }
    bad = wave_usum(bad);
    if ((threadIdx.x & 63) == 0) s_bad[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 all = 0;
        for (int w = 0; w < kWaves; ++w) all += s_bad[w];
        if (all) atomicAdd(counts + n, (unsigned long long)all);
    }
}

template <typename S, int SRC>
void run_valid_map(rfi_ctx* ctx, const void* src, const uint8_t* flags, bool per_baseline, int n, int64_t px, uint8_t* map,
                   int64_t* counts) {
    const size_t scalars = (size_t)8 * px;
    for (int n0 = 0; n0 < n; n0 += kMaxGridY) {
        const int ny = std::min(n - n0, kMaxGridY);
        const dim3 g((unsigned)std::min<int64_t>(cdiv(px, kBlock), std::max(1, 2 * kMaxBlocks / ny)), (unsigned)ny), b(kBlock);
        hipLaunchKernelGGL((nv_map_kernel<S, SRC>), g, b, 0, ctx->stream, static_cast<const S*>(src) + (size_t)n0 * scalars,
                           flags ? flags + (size_t)n0 * (per_baseline ? 1 : 4) * px : nullptr, per_baseline ? px : 4 * px,
                           per_baseline ? (int64_t)0 : px, px, map + (size_t)n0 * 4 * px,
                           reinterpret_cast<unsigned long long*>(counts) + n0);
    }
    check_launch("valid_map");
}

// ns_apply_kernel with the invalid map: both channels of an invalid visibility get `fill`.  In place under the same
// rule: a lane reads its pixel's 8 values and 4 map bytes before it writes
template <typename S, int SRC, bool DNHWC>
__global__ __launch_bounds__(kBlock) void nv_apply_kernel(const S* src, const uint8_t* map, float fill, float* dst, int64_t total,
                                                          int64_t px, double centre, double scale, const double* params) {
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= total) return;
    const int64_t n = gid / px, p = gid - n * px;
    if (params) {
        centre = params[2 * n];
        scale = params[2 * n + 1];
    }
    S v[8];
    load_pixel<S, SRC>(src, n, p, px, v);
    float o[8];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const bool inv = map[(n * 4 + c) * px + p] != 0;
        o[2 * c] = inv ? fill : norm_value(v[2 * c], centre, scale);
        o[2 * c + 1] = inv ? fill : norm_value(v[2 * c + 1], centre, scale);
    }
    if constexpr (DNHWC) {
        Quad<float>* q = reinterpret_cast<Quad<float>*>(dst + gid * 8);
        q[0] = Quad<float>{{o[0], o[1], o[2], o[3]}};
        q[1] = Quad<float>{{o[4], o[5], o[6], o[7]}};
    } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) dst[(n * 8 + c) * px + p] = o[c];
    }
}

template <typename S, int SRC>
void run_valid_apply(rfi_ctx* ctx, const void* src, const uint8_t* map, float fill, float* dst, int64_t total, int64_t px,
                     double centre, double scale, const double* params, bool dnhwc) {
    const dim3 g((unsigned)cdiv(total, kBlock)), b(kBlock);
    if (dnhwc)
        hipLaunchKernelGGL((nv_apply_kernel<S, SRC, true>), g, b, 0, ctx->stream, static_cast<const S*>(src), map, fill, dst, total,
                           px, centre, scale, params);
    else
        hipLaunchKernelGGL((nv_apply_kernel<S, SRC, false>), g, b, 0, ctx->stream, static_cast<const S*>(src), map, fill, dst, total,
                           px, centre, scale, params);
    check_launch("valid_apply");
}

// the six source forms -> the template instance that reads them
#define RFI_VALID_BY_SOURCE(run, ...)                                                                        \
    do {                                                                                                     \
        if (dtype == RFI_C128) run<double, SRC_COMPLEX>(__VA_ARGS__);                                        \
        else if (dtype == RFI_C64) run<float, SRC_COMPLEX>(__VA_ARGS__);                                     \
        else if (dtype == RFI_F64 && src_nhwc) run<double, SRC_NHWC>(__VA_ARGS__);                           \
        else if (dtype == RFI_F64) run<double, SRC_PLANAR>(__VA_ARGS__);                                     \
        else if (src_nhwc) run<float, SRC_NHWC>(__VA_ARGS__);                                                \
        else run<float, SRC_PLANAR>(__VA_ARGS__);                                                            \
    } while (0)

}  // namespace

size_t valid_stats_ws_bytes(int pops, int64_t seg) { return hist_bytes(pops) + vstate_bytes(pops) + partial_bytes(pops, seg); }

void launch_valid_stats(rfi_ctx* ctx, const norm_chunk* chunks_dev, const valid_chunk* valid_dev, int n_chunks, bool f32, int64_t seg,
                        int pops, bool quantiles, void* ws, rfi_norm_stats* out_dev) {
    const int np = norm_stats_passes(f32, quantiles);
    ProfScope ps(ctx, FAM_PREPROCESS, 0, (double)np * (double)pops * (double)seg * (f32 ? 4.5 : 8.5), "valid_stats");
    NvArgs a;
    a.s.chunks = chunks_dev;
    a.s.n_chunks = n_chunks;
    a.s.pops = pops;
    a.s.last_pass = np - 1;
    a.s.seg = seg;
    a.s.wtiles = cdiv(seg, kSumTile);
    for (int s = 0; s < kSlots; ++s) a.s.rank[s] = 0;
    char* w = static_cast<char*>(ws);
    a.s.ghist = reinterpret_cast<u64*>(w);
    a.s.st = nullptr;
    a.st = reinterpret_cast<NvState*>(w + hist_bytes(pops));
    a.s.partial = reinterpret_cast<double*>(w + hist_bytes(pops) + vstate_bytes(pops));
    a.s.out = out_dev;
    a.vc = valid_dev;
    RFI_CHECK_HIP(hipMemsetAsync(ws, 0, hist_bytes(pops) + vstate_bytes(pops), ctx->stream));
    if (f32) run_valid_stats<float>(ctx, a);
    else run_valid_stats<double>(ctx, a);
}

void launch_valid_map(rfi_ctx* ctx, const void* src, int dtype, bool src_nhwc, const uint8_t* flags, bool per_baseline, int n,
                      int64_t px, uint8_t* map, int64_t* counts_dev) {
    const bool f32 = dtype == RFI_C64 || dtype == RFI_F32;
    ProfScope ps(ctx, FAM_PREPROCESS, 0, (double)n * (double)px * (8 * (f32 ? 4 : 8) + 4 + (flags ? (per_baseline ? 1 : 4) : 0)),
                 "valid_map");
    RFI_CHECK_HIP(hipMemsetAsync(counts_dev, 0, (size_t)n * sizeof(int64_t), ctx->stream));
    RFI_VALID_BY_SOURCE(run_valid_map, ctx, src, flags, per_baseline, n, px, map, counts_dev);
}

void launch_valid_apply(rfi_ctx* ctx, const void* src, int dtype, bool src_nhwc, const uint8_t* map, float fill, int n, int64_t px,
                        double centre, double scale, const double* params_dev, float* dst, bool dst_nhwc) {
    const int64_t total = (int64_t)n * px;
    const bool f32 = dtype == RFI_C64 || dtype == RFI_F32;
    ProfScope ps(ctx, FAM_PREPROCESS, 0, (double)total * (8 * ((f32 ? 4 : 8) + 4) + 4), "valid_apply");
    RFI_VALID_BY_SOURCE(run_valid_apply, ctx, src, map, fill, dst, total, px, centre, scale, params_dev, dst_nhwc);
}

size_t norm_stats_ws_bytes(int pops, int64_t seg) { return hist_bytes(pops) + state_bytes(pops) + partial_bytes(pops, seg); }

int norm_stats_passes(bool f32, bool quantiles) { return !quantiles ? 2 : (f32 ? npass<float>() : npass<double>()); }

void launch_norm_stats(rfi_ctx* ctx, const norm_chunk* chunks_dev, int n_chunks, bool f32, int64_t seg, int pops,
                       bool quantiles, const int64_t* ranks6, void* ws, rfi_norm_stats* out_dev) {
    const int np = norm_stats_passes(f32, quantiles);
    ProfScope ps(ctx, FAM_PREPROCESS, 0, (double)np * (double)pops * (double)seg * (f32 ? 4 : 8));
    NsArgs a;
    a.chunks = chunks_dev;
    a.n_chunks = n_chunks;
    a.pops = pops;
    a.last_pass = np - 1;
    a.seg = seg;
    a.wtiles = cdiv(seg, kSumTile);
    for (int s = 0; s < kSlots; ++s) a.rank[s] = (u64)ranks6[s];
    char* w = static_cast<char*>(ws);
    a.ghist = reinterpret_cast<u64*>(w);
    a.st = reinterpret_cast<NsState*>(w + hist_bytes(pops));
    a.partial = reinterpret_cast<double*>(w + hist_bytes(pops) + state_bytes(pops));
    a.out = out_dev;
    RFI_CHECK_HIP(hipMemsetAsync(ws, 0, hist_bytes(pops) + state_bytes(pops), ctx->stream));
    if (f32) run_stats<float>(ctx, a);
    else run_stats<double>(ctx, a);
}

void launch_norm_apply(rfi_ctx* ctx, const void* src, int dtype, bool src_nhwc, int n, int64_t px, double centre, double scale,
                       const double* params_dev, float* dst, bool dst_nhwc) {
    const int64_t total = (int64_t)n * px;
    const bool f32 = dtype == RFI_C64 || dtype == RFI_F32;
    ProfScope ps(ctx, FAM_PREPROCESS, 0, (double)total * 8 * ((f32 ? 4 : 8) + 4));
    if (dtype == RFI_C128) run_apply<double, SRC_COMPLEX>(ctx, src, dst, total, px, centre, scale, params_dev, dst_nhwc);
    else if (dtype == RFI_C64) run_apply<float, SRC_COMPLEX>(ctx, src, dst, total, px, centre, scale, params_dev, dst_nhwc);
    else if (dtype == RFI_F64 && src_nhwc) run_apply<double, SRC_NHWC>(ctx, src, dst, total, px, centre, scale, params_dev, dst_nhwc);
    else if (dtype == RFI_F64) run_apply<double, SRC_PLANAR>(ctx, src, dst, total, px, centre, scale, params_dev, dst_nhwc);
    else if (src_nhwc) run_apply<float, SRC_NHWC>(ctx, src, dst, total, px, centre, scale, params_dev, dst_nhwc);
    else run_apply<float, SRC_PLANAR>(ctx, src, dst, total, px, centre, scale, params_dev, dst_nhwc);
}

}  // namespace rfi
