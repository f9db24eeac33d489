// SumThreshold baseline flagger on the device (Offringa et al. 2010, MNRAS 405, 155; the scale-invariant-rank operator of
// Offringa, van de Gronde & Roerdink 2012, A&A 539, A95) over a stack of (C, T) planes, time contiguous.  The arithmetic is
// pinned in include/rfi_hip.h ("statistical baseline flagger"); tests/sumthreshold_ref.py restates it in NumPy and every
// result here equals it bit for bit.  The reference toolbox has no counterpart.
//
//   prepare    |z| (cabs_np, input precision) -> float32 X; F = prior | ~isfinite(X); non-finite X <- 0
//   stats      per plane, exact median and MAD of R = X - B over the unflagged samples: radix selection on the ordered
//              integer image of float32 in digits of 11, 11 and 10 bits (st_hist_kernel: LDS histogram per workgroup, one
//              integer atomic per non-zero bin; st_pick_kernel: one workgroup per plane picks the digit of both middle
//              ranks).  The last pick writes median, MAD, the `done` mark and the threshold ladder into the plane's state
//              record: nothing is read back between the upload and the download.
//   pass       one window length along one axis.  F_out starts as a copy of F_in and the kernel only ever stores 1, so
//              workgroups may overlap in what they write.  Time: a workgroup holds kTLen consecutive samples of one row
//              (kTLen - (M - 1) window starts); frequency: kFRows channels of kFCols adjacent time samples (lanes across
//              time, so loads coalesce).  The balanced tree d_j(i) = d_{j-1}(i) + d_{j-1}(i + 2^(j-1)) is built in LDS,
//              one level per barrier pair.
//   smooth     two separable masked sums in double, taps ascending, the intermediate (N1, D1) planes through HBM.
//   sir        one lane per line walks it twice: forward for the prefix sums and their running minimum (kept in a
//              workspace), backward for the suffix maximum.  Lanes lie across lines.
// No float atomics; every kernel is a function of its arguments alone.
#include <climits>
#include <utility>

#include "kernels.hpp"
#include "launch_common.hpp"
#include "select_common.hpp"

namespace rfi {

// the threshold ladder: the one function of rfi_sumthreshold_ladder (host) and st_pick_kernel (device)
__host__ __device__ inline void st_ladder(const rfi_sumthreshold_config& c, double sigma, int it, double* chi) {
    double s = c.base_sensitivity;
    for (int i = 0; i < c.iterations - 1 - it; ++i) s = s * 2.0;
    const double num = (s * c.chi_1) * sigma;
    double p = 1.0;
    for (int k = 0; k < c.levels; ++k) {
        if (k) p = p * c.rho;
        chi[k] = num / p;
    }
}

namespace {

constexpr int kBlock = 256;
constexpr int kDigit = 11, kBins = 1 << kDigit, kPasses = 3;
constexpr int kTLen = 640;                  // time pass: samples of one row per workgroup
constexpr int kFRows = 160, kFCols = 32;    // frequency pass: channels x time samples per workgroup
constexpr int kMaxWindow = 128;

struct StPlane {                            // per-plane state, device resident
    double center;                          // (double) median of the current iteration
    double chi[8];                          // thresholds of the current iteration
    unsigned prefix[2], rank[2];            // radix selection of ranks (n - 1) / 2 and n / 2
    unsigned n;                             // unflagged samples
    int done;                               // no unflagged sample, or MAD == 0: the plane goes straight to SIR
    float med, mad;
};
constexpr int kStateDoubles = sizeof(StPlane) / sizeof(double), kStateInts = sizeof(StPlane) / sizeof(int);
static_assert(sizeof(StPlane) % sizeof(double) == 0, "StPlane is addressed in doubles");

template <int IN>
__global__ __launch_bounds__(kBlock) void st_prepare_kernel(const void* __restrict__ src, const uint8_t* __restrict__ prior, int64_t n,
                                                            float* __restrict__ X, uint8_t* __restrict__ F) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float x;
    if constexpr (IN == RFI_C128) {
        const double* p = static_cast<const double*>(src);
        x = (float)cabs_np(p[2 * i], p[2 * i + 1]);
    } else if constexpr (IN == RFI_C64) {
        const float* p = static_cast<const float*>(src);
        x = cabs_np(p[2 * i], p[2 * i + 1]);
    } else if constexpr (IN == RFI_F64) {
        x = (float)static_cast<const double*>(src)[i];
    } else {
        x = static_cast<const float*>(src)[i];
    }
    const bool fin = isfinite(x);
    F[i] = ((prior && prior[i]) || !fin) ? 1 : 0;
    X[i] = fin ? x : 0.0f;
}

// ---- statistics: one radix digit of selection `sel` (0: R, 1: |R - median|) over the unflagged samples of every plane
__global__ __launch_bounds__(kBlock) void st_hist_kernel(const float* __restrict__ X, const float* __restrict__ B,
                                                         const uint8_t* __restrict__ F, int64_t px, int bpp,
                                                         const StPlane* __restrict__ st, unsigned* __restrict__ hist, int sel, int pass) {
    __shared__ unsigned lh[2][kBins];
    const int plane = blockIdx.x / bpp, blk = blockIdx.x - plane * bpp;
    const StPlane& s = st[plane];
    if (s.done) return;
    const unsigned p0 = s.prefix[0], p1 = s.prefix[1];
    const bool two = p0 != p1;              // the two middle ranks share a histogram while their prefixes agree
    const float med = s.med;
    for (int b = threadIdx.x; b < 2 * kBins; b += kBlock) (&lh[0][0])[b] = 0;
    __syncthreads();
    const int hi = 32 - kDigit * pass, sh = hi > kDigit ? hi - kDigit : 0;
    const unsigned mask = pass == 0 ? 0u : ~0u << hi, dmask = (1u << (hi - sh)) - 1u;
    const int64_t base = (int64_t)plane * px;
    for (int64_t i = (int64_t)blk * kBlock + threadIdx.x; i < px; i += (int64_t)bpp * kBlock) {
        if (F[base + i]) continue;
        const float r = X[base + i] - B[base + i];
        const float y = sel ? fabsf(r - med) : r;
        const unsigned k = okey(y);
        if ((k & mask) == p0) atomicAdd(&lh[0][(k >> sh) & dmask], 1u);
        if (two && (k & mask) == p1) atomicAdd(&lh[1][(k >> sh) & dmask], 1u);
    }
    __syncthreads();
    unsigned* g = hist + (size_t)plane * 2 * kBins;
    for (int b = threadIdx.x; b < (two ? 2 : 1) * kBins; b += kBlock) {
        const unsigned c = (&lh[0][0])[b];
        if (c) atomicAdd(&g[b], c);
    }
}

// one workgroup per plane: the digit of both ranks, then (last digit) the value; zeroes the histograms it has read
__global__ __launch_bounds__(kBlock) void st_pick_kernel(StPlane* __restrict__ st, unsigned* __restrict__ hist, int sel, int pass,
                                                         rfi_sumthreshold_config cfg, int it) {
    constexpr int per = kBins / kBlock;
    __shared__ unsigned part[kBlock];
    __shared__ unsigned s_digit[2], s_below[2];
    StPlane* s = st + blockIdx.x;
    if (s->done) return;
    unsigned* g = hist + (size_t)blockIdx.x * 2 * kBins;
    const bool two = s->prefix[0] != s->prefix[1];
    unsigned n = s->n;
    unsigned rank[2] = {s->rank[0], s->rank[1]};
    const int tid = threadIdx.x;
    bool empty = false;
    for (int q = 0; q < 2; ++q) {
        const unsigned* h = g + (two ? q : 0) * kBins;
        unsigned loc[per], sum = 0;
        for (int k = 0; k < per; ++k) {
            loc[k] = h[tid * per + k];
            sum += loc[k];
        }
        __syncthreads();                                   // (the previous round's readers of part[] are through)
        part[tid] = sum;
        __syncthreads();
        for (int o = 1; o < kBlock; o <<= 1) {             // inclusive scan
            const unsigned add = tid >= o ? part[tid - o] : 0;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        if (pass == 0) {                                   // the first digit's histogram holds every unflagged sample
            n = part[kBlock - 1];
            if (n == 0) { empty = true; break; }           // uniform: every lane reads the same total
            rank[q] = q ? n / 2 : (n - 1) / 2;
        }
        const unsigned incl = part[tid], excl = incl - sum;
        if (rank[q] >= excl && rank[q] < incl) {
            unsigned c = excl;
            for (int k = 0; k < per; ++k) {
                if (rank[q] < c + loc[k]) {
                    s_digit[q] = tid * per + k;
                    s_below[q] = c;
                    break;
                }
                c += loc[k];
            }
        }
    }
    __syncthreads();
    for (int b = tid; b < 2 * kBins; b += kBlock) g[b] = 0;
    if (tid != 0) return;
    if (empty) {
        s->n = 0;
        s->done = 1;
        return;
    }
    const int hi = 32 - kDigit * pass, sh = hi > kDigit ? hi - kDigit : 0;
    unsigned prefix[2];
    for (int q = 0; q < 2; ++q) {
        prefix[q] = s->prefix[q] | (s_digit[q] << sh);
        s->prefix[q] = prefix[q];
        s->rank[q] = rank[q] - s_below[q];
    }
    s->n = n;
    if (pass != kPasses - 1) return;
    const float lo = unkey(prefix[0]), up = unkey(prefix[1]);
    const float val = (n & 1u) ? lo : (lo + up) / 2.0f;    // NumPy's float32 mean of the two middle values
    s->prefix[0] = s->prefix[1] = 0;
    if (sel == 0) {
        s->med = val;
        s->center = (double)val;
    } else {
        s->mad = val;
        if (val == 0.0f) s->done = 1;
        else st_ladder(cfg, 1.4826 * (double)val, it, s->chi);
    }
}

// ---- one SumThreshold pass along time.  Window starts t0 .. t0 + kTLen - M of row `line`; F_out already holds F_in.
__global__ __launch_bounds__(kBlock) void st_pass_time_kernel(const float* __restrict__ X, const float* __restrict__ B,
                                                              const uint8_t* __restrict__ Fin, uint8_t* __restrict__ Fout, int C, int T,
                                                              int M, int tiles, const double* __restrict__ center,
                                                              const double* __restrict__ chi, int pstride,
                                                              const int* __restrict__ done, int dstride) {
    __shared__ double d[kTLen];
    __shared__ unsigned short nn[kTLen];
    __shared__ uint8_t mark[kTLen];
    const int64_t line = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - line * tiles);
    const int plane = (int)(line / C);
    if (done && done[(size_t)plane * dstride]) return;
    const int step = kTLen - (M - 1), t0 = tile * step, tid = threadIdx.x;
    const double ctr = center[(size_t)plane * pstride], th = chi[(size_t)plane * pstride];
    const int64_t base = line * T;
    for (int i = tid; i < kTLen; i += kBlock) {
        const int t = t0 + i;
        double v = 0.0;
        unsigned short u = 0;
        if (t < T && !Fin[base + t]) {
            const float r = B ? X[base + t] - B[base + t] : X[base + t];
            v = (double)r - ctr;
            u = 1;
        }
        d[i] = v;
        nn[i] = u;
        mark[i] = 0;
    }
    __syncthreads();
    constexpr int kPer = (kTLen + kBlock - 1) / kBlock;
    for (int h = 1; h < M; h <<= 1) {
        double a[kPer];
        unsigned short b[kPer];
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int i = tid + kBlock * j;
            if (i + h < kTLen) {
                a[j] = d[i] + d[i + h];
                b[j] = (unsigned short)(nn[i] + nn[i + h]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int i = tid + kBlock * j;
            if (i + h < kTLen) {
                d[i] = a[j];
                nn[i] = b[j];
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < step; i += kBlock) {
        if (t0 + i + M > T) break;                         // only windows wholly inside the line
        const int n = nn[i];
        if (n >= 1 && fabs(d[i]) > (double)n * th)
            for (int m = 0; m < M; ++m) mark[i + m] = 1;
    }
    __syncthreads();
    for (int i = tid; i < kTLen; i += kBlock)
        if (mark[i]) Fout[base + t0 + i] = 1;              // (a marked sample lies inside a counted window: t0 + i < T)
}

// ---- one SumThreshold pass along frequency: channels c0 .. c0 + kFRows - 1 of kFCols adjacent time samples
__global__ __launch_bounds__(kBlock) void st_pass_freq_kernel(const float* __restrict__ X, const float* __restrict__ B,
                                                              const uint8_t* __restrict__ Fin, uint8_t* __restrict__ Fout, int C, int T,
                                                              int M, int ctiles, int rtiles, const double* __restrict__ center,
                                                              const double* __restrict__ chi, int pstride,
                                                              const int* __restrict__ done, int dstride) {
    __shared__ double d[kFRows][kFCols];
    __shared__ unsigned short nn[kFRows][kFCols];
    __shared__ uint8_t mark[kFRows][kFCols];
    const int ct = blockIdx.x % ctiles;
    const int64_t rest = blockIdx.x / ctiles;
    const int rt = (int)(rest % rtiles), plane = (int)(rest / rtiles);
    if (done && done[(size_t)plane * dstride]) return;
    constexpr int kGroups = kBlock / kFCols, kPer = kFRows / kGroups;
    const int col = threadIdx.x % kFCols, rg = threadIdx.x / kFCols;
    const int step = kFRows - (M - 1), c0 = rt * step, t = ct * kFCols + col;
    const double ctr = center[(size_t)plane * pstride], th = chi[(size_t)plane * pstride];
    const int64_t base = (int64_t)plane * C * T;
#pragma unroll 4
    for (int j = 0; j < kPer; ++j) {
        const int r = rg + kGroups * j, c = c0 + r;
        double v = 0.0;
        unsigned short u = 0;
        if (t < T && c < C) {
            const int64_t o = base + (int64_t)c * T + t;
            if (!Fin[o]) {
                const float x = B ? X[o] - B[o] : X[o];
                v = (double)x - ctr;
                u = 1;
            }
        }
        d[r][col] = v;
        nn[r][col] = u;
        mark[r][col] = 0;
    }
    __syncthreads();
    for (int h = 1; h < M; h <<= 1) {
        double a[kPer];
        unsigned short b[kPer];
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int r = rg + kGroups * j;
            if (r + h < kFRows) {
                a[j] = d[r][col] + d[r + h][col];
                b[j] = (unsigned short)(nn[r][col] + nn[r + h][col]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int r = rg + kGroups * j;
            if (r + h < kFRows) {
                d[r][col] = a[j];
                nn[r][col] = b[j];
            }
        }
        __syncthreads();
    }
    if (t < T)
        for (int r = rg; r < step; r += kGroups) {
            if (c0 + r + M > C) break;
            const int n = nn[r][col];
            if (n >= 1 && fabs(d[r][col]) > (double)n * th)
                for (int m = 0; m < M; ++m) mark[r + m][col] = 1;
        }
    __syncthreads();
    if (t < T)
        for (int r = rg; r < kFRows; r += kGroups)
            if (mark[r][col]) Fout[base + (int64_t)(c0 + r) * T + t] = 1;
}

// ---- masked smooth, time direction: N1 = sum w_t x, D1 = sum w_t u over the taps inside the row, ascending
__global__ __launch_bounds__(kBlock) void st_smooth_time_kernel(const float* __restrict__ X, const uint8_t* __restrict__ F, int64_t total,
                                                                int T, const double* __restrict__ w, int H, double* __restrict__ N1,
                                                                double* __restrict__ D1) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int t = (int)(i % T);
    const int lo = -H > -t ? -H : -t, hi = H < T - 1 - t ? H : T - 1 - t;
    double n = 0.0, dd = 0.0;
    for (int k = lo; k <= hi; ++k) {
        const double u = F[i + k] ? 0.0 : 1.0;
        const double x = u * (double)X[i + k];
        const double wk = w[k + H];
        n = n + wk * x;
        dd = dd + wk * u;
    }
    N1[i] = n;
    D1[i] = dd;
}
// frequency direction on (N1, D1), then B = D2 > 0 ? (float)(N2 / D2) : 0
__global__ __launch_bounds__(kBlock) void st_smooth_freq_kernel(const double* __restrict__ N1, const double* __restrict__ D1, int64_t total,
                                                                int C, int T, const double* __restrict__ w, int H, float* __restrict__ Bout) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int c = (int)((i / T) % C);
    const int lo = -H > -c ? -H : -c, hi = H < C - 1 - c ? H : C - 1 - c;
    double n = 0.0, dd = 0.0;
    for (int k = lo; k <= hi; ++k) {
        const double wk = w[k + H];
        n = n + wk * N1[i + (int64_t)k * T];
        dd = dd + wk * D1[i + (int64_t)k * T];
    }
    Bout[i] = dd > 0.0 ? (float)(n / dd) : 0.0f;
}

// ---- scale-invariant rank operator along one axis; element k of line l of a plane lies at l * lstride + k * kstride.
// With v = q for a flagged sample and q - 1024 otherwise, P the prefix sums of v: flagged iff max_{j>k} P_j >= min_{j<=k} P_j.
// Fin and Fout may be the same buffer (a lane reads its sample before it writes it, and no other lane touches its line).
__global__ __launch_bounds__(kBlock) void st_sir_kernel(const uint8_t* Fin, uint8_t* Fout, int* __restrict__ pmin, int64_t lines,
                                                        int lines_per_plane, int L, int64_t lstride, int64_t kstride,
                                                        int64_t plane_stride, int q) {
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= lines) return;
    const int64_t plane = g / lines_per_plane;
    const int64_t base = plane * plane_stride + (g - plane * lines_per_plane) * lstride;
    int P = 0, mn = 0;
    for (int k = 0; k < L; ++k) {
        const int64_t o = base + k * kstride;
        mn = P < mn ? P : mn;
        pmin[o] = mn;
        P += Fin[o] ? q : q - 1024;
    }
    int smax = INT_MIN;
    for (int k = L - 1; k >= 0; --k) {                     // here P == P_{k+1}
        const int64_t o = base + k * kstride;
        smax = P > smax ? P : smax;
        const int f = Fin[o] ? q : q - 1024;
        Fout[o] = smax >= pmin[o] ? 1 : 0;
        P -= f;
    }
}

unsigned* hist_of(void* state, int planes) { return reinterpret_cast<unsigned*>(static_cast<StPlane*>(state) + planes); }

}  // namespace

void sumthreshold_ladder_host(const rfi_sumthreshold_config& cfg, double sigma, int iteration, double* chi) {
    st_ladder(cfg, sigma, iteration, chi);
}

size_t st_state_bytes(int planes) { return (size_t)planes * (sizeof(StPlane) + 2 * kBins * sizeof(unsigned)); }
int st_max_window() { return kMaxWindow; }

void launch_st_prepare(rfi_ctx* ctx, const void* src, int dtype, const uint8_t* prior, int64_t n, float* X, uint8_t* F) {
    ProfScope ps(ctx, FAM_METRICS, 0, (double)n * (dtype_bytes(dtype) + (prior ? 1 : 0) + 5), "st_prepare");
    const dim3 g(grid_of(cdiv(n, kBlock), "sumthreshold prepare")), b(kBlock);
    switch (dtype) {
        case RFI_C128: hipLaunchKernelGGL(st_prepare_kernel<RFI_C128>, g, b, 0, ctx->stream, src, prior, n, X, F); break;
        case RFI_C64: hipLaunchKernelGGL(st_prepare_kernel<RFI_C64>, g, b, 0, ctx->stream, src, prior, n, X, F); break;
        case RFI_F64: hipLaunchKernelGGL(st_prepare_kernel<RFI_F64>, g, b, 0, ctx->stream, src, prior, n, X, F); break;
        default: hipLaunchKernelGGL(st_prepare_kernel<RFI_F32>, g, b, 0, ctx->stream, src, prior, n, X, F); break;
    }
    check_launch("st_prepare");
}

// median, MAD and the ladder of iteration `it` into the planes' state records (state: st_state_bytes(planes), zeroed once
// before the first iteration)
void launch_st_stats(rfi_ctx* ctx, const float* X, const float* B, const uint8_t* F, int planes, int64_t px, void* state,
                     const rfi_sumthreshold_config& cfg, int it) {
    ProfScope ps(ctx, FAM_METRICS, 0, (double)planes * px * 9 * 2 * kPasses, "st_stats");
    StPlane* st = static_cast<StPlane*>(state);
    unsigned* hist = hist_of(state, planes);
    const int64_t want = cdiv(px, (int64_t)kBlock * 16);
    const int bpp = (int)(want < 1 ? 1 : (want > 256 ? 256 : want));
    const dim3 g(grid_of((int64_t)planes * bpp, "sumthreshold statistics")), b(kBlock);
    for (int sel = 0; sel < 2; ++sel)
        for (int p = 0; p < kPasses; ++p) {
            hipLaunchKernelGGL(st_hist_kernel, g, b, 0, ctx->stream, X, B, F, px, bpp, st, hist, sel, p);
            hipLaunchKernelGGL(st_pick_kernel, dim3(planes), b, 0, ctx->stream, st, hist, sel, p, cfg, it);
        }
    check_launch("st_stats");
}

// F_out = F_in | hits of window M along `axis` (0 frequency, 1 time); the caller has checked 1 <= M <= line length.
// center / chi: one double per plane, pstride doubles apart; done (optional): one int per plane, dstride ints apart.
void launch_st_pass(rfi_ctx* ctx, const float* X, const float* B, const uint8_t* Fin, uint8_t* Fout, int planes, int C, int T, int M,
                    int axis, const double* center, const double* chi, int pstride, const int* done, int dstride) {
    const int64_t n = (int64_t)planes * C * T;
    ProfScope ps(ctx, FAM_METRICS, 0, (double)n * ((B ? 8 : 4) + 3), "st_pass");
    RFI_CHECK_HIP(hipMemcpyAsync(Fout, Fin, (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
    if (axis == 1) {
        const int tiles = (int)cdiv(T - M + 1, kTLen - (M - 1));
        hipLaunchKernelGGL(st_pass_time_kernel, dim3(grid_of((int64_t)planes * C * tiles, "sumthreshold pass")), dim3(kBlock), 0,
                           ctx->stream, X, B, Fin, Fout, C, T, M, tiles, center, chi, pstride, done, dstride);
    } else {
        const int ctiles = (int)cdiv(T, kFCols), rtiles = (int)cdiv(C - M + 1, kFRows - (M - 1));
        hipLaunchKernelGGL(st_pass_freq_kernel, dim3(grid_of((int64_t)planes * ctiles * rtiles, "sumthreshold pass")), dim3(kBlock), 0,
                           ctx->stream, X, B, Fin, Fout, C, T, M, ctiles, rtiles, center, chi, pstride, done, dstride);
    }
    check_launch("st_pass");
}

// B = masked weighted mean of X; wt / wf: device tables of 2 ht + 1 / 2 hf + 1 doubles; nd: 2 n doubles of workspace
void launch_st_smooth(rfi_ctx* ctx, const float* X, const uint8_t* F, int planes, int C, int T, const double* wt, int ht,
                      const double* wf, int hf, double* nd, float* B) {
    const int64_t n = (int64_t)planes * C * T;
    ProfScope ps(ctx, FAM_METRICS, 0, (double)n * (5 + 16 + 16 + 4), "st_smooth");
    const dim3 g(grid_of(cdiv(n, kBlock), "sumthreshold smooth")), b(kBlock);
    hipLaunchKernelGGL(st_smooth_time_kernel, g, b, 0, ctx->stream, X, F, n, T, wt, ht, nd, nd + n);
    hipLaunchKernelGGL(st_smooth_freq_kernel, g, b, 0, ctx->stream, nd, nd + n, n, C, T, wf, hf, B);
    check_launch("st_smooth");
}

// SIR along `axis` (0 frequency, 1 time) with integer q in 1 .. 1023; ws: n ints; Fin may equal Fout
void launch_st_sir(rfi_ctx* ctx, const uint8_t* Fin, uint8_t* Fout, int planes, int C, int T, int axis, int q, int* ws) {
    const int64_t n = (int64_t)planes * C * T;
    ProfScope ps(ctx, FAM_METRICS, 0, (double)n * (1 + 4 + 1 + 4 + 1), "st_sir");
    const int lpp = axis == 1 ? C : T, L = axis == 1 ? T : C;
    const int64_t lines = (int64_t)planes * lpp;
    hipLaunchKernelGGL(st_sir_kernel, dim3(grid_of(cdiv(lines, kBlock), "sumthreshold sir")), dim3(kBlock), 0, ctx->stream, Fin, Fout, ws,
                       lines, lpp, L, axis == 1 ? (int64_t)T : (int64_t)1, axis == 1 ? (int64_t)1 : (int64_t)T, (int64_t)C * T, q);
    check_launch("st_sir");
}

// the whole pipeline on `planes` device-resident planes.  Workspace: the state records, X and B floats, Fa and Fb bytes and
// the (N1, D1) doubles of n = planes C T samples; wt / wf: device weight tables.  The flags end in `dst` (n bytes of device
// memory), or in a buffer inside ws when dst is null; returns where.
size_t sumthreshold_ws_bytes(int planes, int C, int T) {
    const size_t n = (size_t)planes * C * T;
    return al(st_state_bytes(planes)) + 2 * al(n * 4) + 2 * al(n) + al(n * 16);
}
uint8_t* launch_sumthreshold_flag(rfi_ctx* ctx, const void* src, int dtype, const uint8_t* prior, int planes, int C, int T,
                                  const rfi_sumthreshold_config& cfg, const double* wt, const double* wf, void* ws, uint8_t* dst) {
    const int64_t px = (int64_t)C * T, n = planes * px;
    Carve cv{static_cast<char*>(ws)};
    void* state = cv.take<char>(st_state_bytes(planes));
    float *X = cv.take<float>(n), *B = cv.take<float>(n);
    uint8_t *Fa = cv.take<uint8_t>(n), *Fb = cv.take<uint8_t>(n);
    double* nd = cv.take<double>(2 * n);
    uint8_t* out = dst ? dst : Fa;
    RFI_CHECK_HIP(hipMemsetAsync(state, 0, st_state_bytes(planes), ctx->stream));
    RFI_CHECK_HIP(hipMemsetAsync(B, 0, (size_t)n * sizeof(float), ctx->stream));
    launch_st_prepare(ctx, src, dtype, prior, n, X, Fa);
    uint8_t *cur = Fa, *other = Fb;
    const StPlane* st = static_cast<const StPlane*>(state);
    const double* center = &st->center;
    const int* done = &st->done;
    for (int it = 0; it < cfg.iterations; ++it) {
        launch_st_stats(ctx, X, B, cur, planes, px, state, cfg, it);
        for (int k = 0; k < cfg.levels; ++k) {
            const int M = 1 << k;
            for (int axis = 1; axis >= 0; --axis) {
                if (M > (axis == 1 ? T : C)) continue;
                launch_st_pass(ctx, X, B, cur, other, planes, C, T, M, axis, center, st->chi + k, kStateDoubles, done, kStateInts);
                std::swap(cur, other);
            }
        }
        if (it < cfg.iterations - 1) launch_st_smooth(ctx, X, cur, planes, C, T, wt, cfg.half_t, wf, cfg.half_f, nd, B);
    }
    if (cfg.sir_q > 0) {
        launch_st_sir(ctx, cur, cur, planes, C, T, 1, cfg.sir_q, reinterpret_cast<int*>(nd));
        launch_st_sir(ctx, cur, out, planes, C, T, 0, cfg.sir_q, reinterpret_cast<int*>(nd));
    } else if (out != cur) {
        RFI_CHECK_HIP(hipMemcpyAsync(out, cur, (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return out;
}

}  // namespace rfi
