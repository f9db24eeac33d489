// Flagging-quality statistics of a whole array (rfi_toolbox/evaluation/statistics.py:10-229): count, mean, std,
// median, MAD and max of ALL elements and of the UNFLAGGED elements, from one call.
//
// Values are |z| for complex input (NumPy's complex-abs rule, cabs_np below) and stay in the input's precision:
// T = float for complex64 / float32 (NumPy's float32 median, |x - median| and mean-of-two), T = double otherwise.
//
//   pass 1     read the input once: per view count / NaN count / fp64 sum / max, the flagged count, the first radix
//              digit's histogram of both views; |z| is stored (input precision) for the later passes
//   control    one workgroup: fixed-order reduction of the per-workgroup slabs -> mean; picks the digit of each
//              wanted order statistic from the global histogram and narrows its rank (all on the device)
//   hist       one radix digit over the elements that still match each target's prefix, for both views and both
//              middle ranks at once; the first MAD digit shares its read with the (x - mean)^2 pass
//
// Order statistics are exact: radix selection on the order-preserving integer image of T (32 or 64 bits) in digits
// of kDigit bits, so 3 passes for float32-origin data and 6 for float64.  Sums are fp64 per thread in grid-stride
// order, then a fixed shuffle tree, then per-workgroup slabs reduced in a fixed order: bitwise reproducible.  The
// unflagged view runs the same instructions as the all view, guarded by the flag, so with no flag set the two are
// bit-identical.  Histogram counts are integers (LDS atomics, then one global integer atomic per non-zero bin).
#include "kernels.hpp"
#include "select_common.hpp"

namespace rfi {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kDigit = 11, kBins = 1 << kDigit;
constexpr int kSlots = 4;            // slot 2*view + j: view 0 all / 1 unflagged; j 0 rank (n-1)/2, j 1 rank n/2
constexpr int kMaxPass = 6;          // ceil(64 / kDigit)
constexpr int kMaxGrid = 1024;       // 4 workgroups per CU on 256 CUs
constexpr int kUnroll = 4;

template <typename T> struct KeyOf;
template <> struct KeyOf<float> { typedef unsigned K; static constexpr int bits = 32; };
template <> struct KeyOf<double> { typedef u64 K; static constexpr int bits = 64; };

template <typename T, int IN>
__device__ __forceinline__ T load_in(const void* __restrict__ src, int64_t i) {
    if constexpr (IN == RFI_C128) {
        const double* p = static_cast<const double*>(src);
        return cabs_np(p[2 * i], p[2 * i + 1]);
    } else if constexpr (IN == RFI_C64) {
        const float* p = static_cast<const float*>(src);
        return cabs_np(p[2 * i], p[2 * i + 1]);
    } else {
        return static_cast<const T*>(src)[i];
    }
}

// device-side state of one call (zeroed by the host before pass 1)
struct FsState {
    u64 cnt[2], nan[2], madnan[2], flagged;
    double sum[2], max[2], mean[2], ssd[2], sel[2][2];      // sel[0]: median, sel[1]: MAD of each view
    u64 prefix[kSlots], rank[kSlots];
    int active[kSlots], alias[kSlots];                       // alias: slot whose histogram this slot reads
};
struct Slab {                     // per-workgroup partials (pass 1: sums/maxima; deviation pass: squared deviations)
    double sum[2], max[2];
    u64 nan[2], flagged, pad;
};
struct FsArgs {
    const void* src;              // input (dtype of the call)
    const uint8_t* flags;         // nullptr: nothing flagged
    int64_t n;
    void* mag;                    // |z| in T (complex input), nullptr for real input
    int views;                    // bit 0 all, bit 1 unflagged
    int medians;
    int grid;
    Slab* slab;
    u64* ghist;                   // [2 selections][kMaxPass][kSlots][kBins]
    FsState* st;
    rfi_flag_stats* out;          // [2] views
};

template <typename T> __host__ __device__ constexpr int npass() { return (KeyOf<T>::bits + kDigit - 1) / kDigit; }
template <typename T> __device__ __forceinline__ int digit_shift(int p) {
    const int s = KeyOf<T>::bits - kDigit * (p + 1);
    return s > 0 ? s : 0;
}
__device__ __forceinline__ u64* hist_of(const FsArgs& a, int sel, int pass, int slot) {
    return a.ghist + ((size_t)(sel * kMaxPass + pass) * kSlots + slot) * kBins;
}

// reduce this thread's partials over the workgroup and store them as slab[blockIdx.x]
__device__ void store_slab(Slab* slab, double s0, double s1, double m0, double m1, u64 n0, u64 n1, u64 fl) {
    __shared__ Slab ws[kWaves];
    s0 = wave_sum(s0); s1 = wave_sum(s1); m0 = wave_max(m0); m1 = wave_max(m1);
    n0 = wave_usum(n0); n1 = wave_usum(n1); fl = wave_usum(fl);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) ws[w] = Slab{{s0, s1}, {m0, m1}, {n0, n1}, fl, 0};
    __syncthreads();
    if (threadIdx.x == 0) {
        Slab r = ws[0];
        for (int k = 1; k < kWaves; ++k) {
            for (int v = 0; v < 2; ++v) {
                r.sum[v] += ws[k].sum[v];
                r.max[v] = fmax(r.max[v], ws[k].max[v]);
                r.nan[v] += ws[k].nan[v];
            }
            r.flagged += ws[k].flagged;
        }
        slab[blockIdx.x] = r;
    }
}

// add the workgroup's LDS histograms of the built slots into the pass's global histograms
__device__ void merge_hist(const FsArgs& a, unsigned (*lh)[kBins], const int* built, int sel, int pass) {
    __syncthreads();
    for (int s = 0; s < kSlots; ++s) {
        if (!built[s]) continue;
        u64* g = hist_of(a, sel, pass, s);
        for (int b = threadIdx.x; b < kBins; b += kBlock) {
            const unsigned c = lh[s][b];
            if (c) atomicAdd(&g[b], (u64)c);
        }
    }
}

// ---- pass 1: moments of both views + the first median digit; |z| stored for the later passes
template <typename T, int IN>
__global__ __launch_bounds__(kBlock) void fs_pass1_kernel(FsArgs a) {
    __shared__ unsigned lh[kSlots][kBins];
    const bool v0 = a.views & 1, v1 = (a.views & 2) != 0, med = a.medians != 0;
    const int built[kSlots] = {v0 && med, 0, v1 && med, 0};
    if (med)
        for (int b = threadIdx.x; b < kSlots * kBins; b += kBlock) (&lh[0][0])[b] = 0;
    __syncthreads();
    const int sh = digit_shift<T>(0);
    double s0 = 0, s1 = 0;
    T m0 = (T)-INFINITY, m1 = (T)-INFINITY;
    u64 n0 = 0, n1 = 0, fl = 0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t base = (int64_t)blockIdx.x * kBlock + threadIdx.x; base < a.n; base += stride * kUnroll) {
        T x[kUnroll];
        bool f[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t i = base + u * stride;
            x[u] = i < a.n ? load_in<T, IN>(a.src, i) : (T)0;
            f[u] = i < a.n && a.flags && a.flags[i];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t i = base + u * stride;
            if (i >= a.n) break;
            if (a.mag) static_cast<T*>(a.mag)[i] = x[u];
            fl += f[u] ? 1 : 0;
            const bool nx = isnan(x[u]);
            const unsigned d = (unsigned)(okey(x[u]) >> sh);
            if (v0) {
                s0 += (double)x[u];
                n0 += nx ? 1 : 0;
                if (x[u] > m0) m0 = x[u];
                if (med) atomicAdd(&lh[0][d], 1u);
            }
            if (v1 && !f[u]) {
                s1 += (double)x[u];
                n1 += nx ? 1 : 0;
                if (x[u] > m1) m1 = x[u];
                if (med) atomicAdd(&lh[2][d], 1u);
            }
        }
    }
    store_slab(a.slab, s0, s1, (double)m0, (double)m1, n0, n1, fl);
    if (med) merge_hist(a, lh, built, 0, 0);
}

// ---- one radix digit of selection `sel` (0 median, 1 MAD about the median) for every active target; with `dev`
//      also the squared deviations about the fp64 mean and the NaN count of the MAD view (the MAD's first digit)
template <typename T>
__global__ __launch_bounds__(kBlock) void fs_hist_kernel(FsArgs a, const T* __restrict__ v, int sel, int pass, int dev) {
    typedef typename KeyOf<T>::K K;
    __shared__ unsigned lh[kSlots][kBins];
    const FsState* st = a.st;
    int built[kSlots];
    K prefix[kSlots];
    bool any = false;
    for (int s = 0; s < kSlots; ++s) {
        built[s] = st->active[s] && st->alias[s] == s;
        prefix[s] = (K)st->prefix[s];
        any = any || built[s];
    }
    const int hi = KeyOf<T>::bits - kDigit * pass, sh = digit_shift<T>(pass);
    const K mask = pass == 0 ? (K)0 : (K)(~(K)0 << hi);
    const unsigned dmask = (1u << (hi - sh)) - 1u;
    const bool v0 = a.views & 1, v1 = (a.views & 2) != 0;
    const double mean0 = st->mean[0], mean1 = st->mean[1];
    const T c0 = (T)st->sel[0][0], c1 = (T)st->sel[0][1];           // medians (T values) for the MAD view
    if (any)
        for (int b = threadIdx.x; b < kSlots * kBins; b += kBlock) (&lh[0][0])[b] = 0;
    __syncthreads();
    double q0 = 0, q1 = 0;
    u64 z0 = 0, z1 = 0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t base = (int64_t)blockIdx.x * kBlock + threadIdx.x; base < a.n; base += stride * kUnroll) {
        T x[kUnroll];
        bool f[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t i = base + u * stride;
            x[u] = i < a.n ? v[i] : (T)0;
            f[u] = i < a.n && a.flags && a.flags[i];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (base + u * stride >= a.n) break;
            for (int w = 0; w < 2; ++w) {
                if (!(w ? v1 && !f[u] : v0)) continue;
                if (dev) {
                    const double d = (double)x[u] - (w ? mean1 : mean0);
                    (w ? q1 : q0) += d * d;
                }
                if (!any) continue;
                const T y = sel ? fabs(x[u] - (w ? c1 : c0)) : x[u];
                if (dev) (w ? z1 : z0) += isnan(y) ? 1 : 0;
                const K k = okey(y);
                for (int j = 0; j < 2; ++j) {
                    const int s = 2 * w + j;
                    if (built[s] && (k & mask) == prefix[s]) atomicAdd(&lh[s][(unsigned)(k >> sh) & dmask], 1u);
                }
            }
        }
    }
    if (dev) store_slab(a.slab, q0, q1, 0.0, 0.0, z0, z1, 0);
    if (any) merge_hist(a, lh, built, sel, pass);
}

// ---- one workgroup: slab reduction, digit choice, results
enum { ST_MOMENTS = 0, ST_SCAN = 1, ST_DEVIATIONS = 2, ST_FINAL = 3 };

// fixed-order reduction of the grid's slabs (thread t takes slabs t, t + kBlock, ...; then a fixed tree)
__device__ Slab reduce_slabs(const Slab* slab, int grid) {
    __shared__ Slab sh[kBlock];
    Slab r{{0, 0}, {-INFINITY, -INFINITY}, {0, 0}, 0, 0};
    for (int g = threadIdx.x; g < grid; g += kBlock) {
        const Slab s = slab[g];
        for (int v = 0; v < 2; ++v) {
            r.sum[v] += s.sum[v];
            r.max[v] = fmax(r.max[v], s.max[v]);
            r.nan[v] += s.nan[v];
        }
        r.flagged += s.flagged;
    }
    sh[threadIdx.x] = r;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            Slab& x = sh[threadIdx.x];
            const Slab& y = sh[threadIdx.x + o];
            for (int v = 0; v < 2; ++v) {
                x.sum[v] += y.sum[v];
                x.max[v] = fmax(x.max[v], y.max[v]);
                x.nan[v] += y.nan[v];
            }
            x.flagged += y.flagged;
        }
        __syncthreads();
    }
    const Slab out = sh[0];
    __syncthreads();
    return out;
}

// digit of the bin holding 0-based rank `rank` of histogram h; *below = count in the bins before it
__device__ void find_digit(const u64* h, u64 rank, int* digit, u64* below) {
    constexpr int per = kBins / kBlock;
    __shared__ u64 part[kBlock];
    u64 loc[per], sum = 0;
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
        for (int k = 0; k < per; ++k) {
            if (rank < c + loc[k]) {
                *digit = threadIdx.x * per + k;
                *below = c;
                break;
            }
            c += loc[k];
        }
    }
    __syncthreads();
}

template <typename T>
__device__ void scan_pass(const FsArgs& a, int sel, int pass) {
    typedef typename KeyOf<T>::K K;
    __shared__ int s_digit, s_act[kSlots], s_alias[kSlots];
    __shared__ u64 s_below, s_rank[kSlots];
    FsState* st = a.st;                                     // written by thread 0 only; the others read LDS copies
    const int sh = digit_shift<T>(pass);
    if (threadIdx.x == 0)
        for (int s = 0; s < kSlots; ++s) {
            s_act[s] = st->active[s];
            s_alias[s] = st->alias[s];
            s_rank[s] = st->rank[s];
        }
    __syncthreads();
    for (int s = 0; s < kSlots; ++s) {
        if (!s_act[s]) continue;                             // uniform across the workgroup
        find_digit(hist_of(a, sel, pass, s_alias[s]), s_rank[s], &s_digit, &s_below);
        if (threadIdx.x == 0) {
            st->prefix[s] |= (u64)s_digit << sh;
            st->rank[s] -= s_below;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        for (int w = 0; w < 2; ++w)                           // the two middle ranks share a histogram while their prefixes agree
            st->alias[2 * w + 1] = st->prefix[2 * w + 1] == st->prefix[2 * w] ? 2 * w : 2 * w + 1;
        if (pass == npass<T>() - 1) {
            for (int w = 0; w < 2; ++w) {
                if (!st->active[2 * w]) continue;
                const T lo = unkey((K)st->prefix[2 * w]), hi = unkey((K)st->prefix[2 * w + 1]);
                st->sel[sel][w] = (st->cnt[w] & 1) ? (double)lo : (double)((T)(lo + hi) / (T)2);   // np.mean of the two
            }
        }
    }
    __syncthreads();
}

// (re)arm the four targets for a selection: ranks (n-1)/2 and n/2 of each wanted, non-empty view
__device__ void arm(FsState* st, int views, int medians) {
    for (int s = 0; s < kSlots; ++s) {
        const int w = s >> 1;
        const u64 n = st->cnt[w];
        st->active[s] = medians && ((views >> w) & 1) && n > 0;
        st->rank[s] = st->active[s] ? ((s & 1) ? n / 2 : (n - 1) / 2) : 0;
        st->prefix[s] = 0;
        st->alias[s] = (s & 1) ? s - 1 : s;                   // pass 0: one histogram per view
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void fs_control_kernel(FsArgs a, int stage, int sel, int pass) {
    FsState* st = a.st;
    const bool f32 = sizeof(T) == 4;
    if (stage == ST_MOMENTS || stage == ST_DEVIATIONS) {
        const Slab r = reduce_slabs(a.slab, a.grid);
        if (threadIdx.x == 0) {
            if (stage == ST_MOMENTS) {
                st->flagged = r.flagged;
                st->cnt[0] = (a.views & 1) ? (u64)a.n : 0;
                st->cnt[1] = (a.views & 2) ? (u64)a.n - r.flagged : 0;
                for (int w = 0; w < 2; ++w) {
                    st->sum[w] = r.sum[w];
                    st->max[w] = r.max[w];
                    st->nan[w] = r.nan[w];
                    st->mean[w] = st->cnt[w] ? r.sum[w] / (double)st->cnt[w] : 0.0;
                }
                arm(st, a.views, a.medians);
            } else {
                for (int w = 0; w < 2; ++w) {
                    st->ssd[w] = r.sum[w];
                    st->madnan[w] = r.nan[w];
                }
            }
        }
        __syncthreads();
        if (a.medians) scan_pass<T>(a, stage == ST_MOMENTS ? 0 : 1, 0);
    } else if (stage == ST_SCAN) {
        scan_pass<T>(a, sel, pass);
        if (sel == 0 && pass == npass<T>() - 1 && threadIdx.x == 0) arm(st, a.views, a.medians);   // targets of the MAD
    } else if (threadIdx.x == 0) {                                                                  // ST_FINAL
        const double qnan = __longlong_as_double(0x7ff8000000000000ll);
        for (int w = 0; w < 2; ++w) {
            rfi_flag_stats o;
            o.count = (int64_t)st->cnt[w];
            o.flagged = (int64_t)st->flagged;
            o.mean = o.std = o.median = o.mad = o.max = qnan;
            if (st->cnt[w]) {
                const double n = (double)st->cnt[w];
                o.mean = f32 ? (double)(float)st->mean[w] : st->mean[w];
                const double sd = sqrt(st->ssd[w] / n);
                o.std = f32 ? (double)(float)sd : sd;
                if (!st->nan[w]) {
                    o.max = st->max[w];
                    if (a.medians) {
                        o.median = st->sel[0][w];
                        if (!st->madnan[w]) o.mad = st->sel[1][w];
                    }
                }
            }
            a.out[w] = o;
        }
    }
}

template <typename T, int IN>
void run(rfi_ctx* ctx, FsArgs a) {
    const T* v = a.mag ? static_cast<const T*>(a.mag) : static_cast<const T*>(a.src);
    const dim3 g(a.grid), b(kBlock);
    const int np = npass<T>();
    hipLaunchKernelGGL((fs_pass1_kernel<T, IN>), g, b, 0, ctx->stream, a);
    check_launch("flag_stats_pass1");
    hipLaunchKernelGGL(fs_control_kernel<T>, dim3(1), b, 0, ctx->stream, a, (int)ST_MOMENTS, 0, 0);
    for (int p = 1; a.medians && p < np; ++p) {
        hipLaunchKernelGGL(fs_hist_kernel<T>, g, b, 0, ctx->stream, a, v, 0, p, 0);
        hipLaunchKernelGGL(fs_control_kernel<T>, dim3(1), b, 0, ctx->stream, a, (int)ST_SCAN, 0, p);
    }
    hipLaunchKernelGGL(fs_hist_kernel<T>, g, b, 0, ctx->stream, a, v, 1, 0, 1);
    hipLaunchKernelGGL(fs_control_kernel<T>, dim3(1), b, 0, ctx->stream, a, (int)ST_DEVIATIONS, 1, 0);
    for (int p = 1; a.medians && p < np; ++p) {
        hipLaunchKernelGGL(fs_hist_kernel<T>, g, b, 0, ctx->stream, a, v, 1, p, 0);
        hipLaunchKernelGGL(fs_control_kernel<T>, dim3(1), b, 0, ctx->stream, a, (int)ST_SCAN, 1, p);
    }
    hipLaunchKernelGGL(fs_control_kernel<T>, dim3(1), b, 0, ctx->stream, a, (int)ST_FINAL, 0, 0);
    check_launch("flag_stats");
}

constexpr size_t kHistBytes = (size_t)2 * kMaxPass * kSlots * kBins * sizeof(u64);
constexpr size_t kSlabBytes = (size_t)kMaxGrid * sizeof(Slab);
constexpr size_t kStateBytes = (sizeof(FsState) + 255) / 256 * 256;

}  // namespace

size_t flag_stats_ws_bytes() { return kHistBytes + kSlabBytes + kStateBytes + 2 * sizeof(rfi_flag_stats); }

void launch_flag_stats(rfi_ctx* ctx, const void* src, int dtype, int64_t n, const uint8_t* flags, int views,
                       bool medians, void* ws, void* mag, rfi_flag_stats* out_dev) {
    const size_t esz = dtype == RFI_C128 ? 16 : (dtype == RFI_F32 ? 4 : 8);
    const bool f32 = dtype == RFI_C64 || dtype == RFI_F32;
    // full-array reads: pass 1 (input), then the deviation pass and (npass - 1) digits of each selection (T values)
    const int later = 1 + (medians ? 2 * ((f32 ? npass<float>() : npass<double>()) - 1) : 0);
    const double fb = flags ? 1.0 : 0.0;
    ProfScope ps(ctx, FAM_METRICS, 0, (double)n * (esz + fb) + (double)later * n * ((f32 ? 4 : 8) + fb));
    FsArgs a;
    a.src = src;
    a.flags = flags;
    a.n = n;
    a.mag = (dtype == RFI_C128 || dtype == RFI_C64) ? mag : nullptr;
    a.views = views;
    a.medians = medians ? 1 : 0;
    const int64_t gr = cdiv(n, (int64_t)kBlock * 8);
    a.grid = (int)(gr < 1 ? 1 : (gr > kMaxGrid ? kMaxGrid : gr));
    char* w = static_cast<char*>(ws);
    a.ghist = reinterpret_cast<u64*>(w);
    a.slab = reinterpret_cast<Slab*>(w + kHistBytes);
    a.st = reinterpret_cast<FsState*>(w + kHistBytes + kSlabBytes);
    a.out = out_dev;
    RFI_CHECK_HIP(hipMemsetAsync(ws, 0, kHistBytes + kSlabBytes + kStateBytes, ctx->stream));
    switch (dtype) {
        case RFI_C128: run<double, RFI_C128>(ctx, a); break;
        case RFI_C64: run<float, RFI_C64>(ctx, a); break;
        case RFI_F64: run<double, RFI_F64>(ctx, a); break;
        default: run<float, RFI_F32>(ctx, a); break;
    }
}

}  // namespace rfi
