// CASA-style baseline flaggers on the device: TFCrop (robust piecewise-polynomial fits along time and frequency), RFlag
// (windowed rms along time, deviation from the mean spectrum, exact medians) and the flag extension, over a stack of (C, T)
// planes, time contiguous, every plane cut along time into chunks of `ntime` samples.  The arithmetic is pinned in
// include/rfi_hip.h ("CASA-style baseline flaggers"); tests/casa_flaggers_ref.py restates it in NumPy and every result here
// equals it bit for bit.  The reference toolbox takes these flaggers from CASA and has no counterpart.
//
//   fit        cf_fit_kernel: one lane per line over an array laid out (planes, K, N) whose lines run along K (element
//              stride N) in chunks of `chunk`; lanes lie across N, so every load of a wave is one contiguous run.  Per
//              iteration and piece the lane walks its samples three times: moments, residuals (kept in a double workspace),
//              rejection.  The working mask is the flag plane itself, updated in place (a lane owns its line).
//   time lines are fitted on the transpose: cf_transpose_kernel stages 32 x 32 tiles through LDS so that both the loads and
//              the stores coalesce, the fit runs on (planes, T, C) with K = T, and the flags are transposed back.
//   bandpass   cf_mean_kernel (on the transpose, lanes across channels), the same fit kernel on the (planes, C, chunks) means
//              with its fit kept, cf_divide_kernel.
//   rflag      rf_rms_kernel (one lane per sample, two walks over its window), rf_spec_kernel (one lane per time sample, two
//              walks over the channels), rf_thr_kernel (one wave per line: median and MAD by radix selection on the ordered
//              64-bit image of the doubles, eight digits of 8 bits, integer LDS atomics), rf_flag_kernel.
//   extend     five integer kernels, each reading a snapshot and writing the other buffer.
// No float atomics; every kernel is a function of its arguments alone.
#include <utility>

#include "kernels.hpp"
#include "launch_common.hpp"
#include "select_common.hpp"

namespace rfi {
namespace {

constexpr int kBlock = 256;
constexpr int kLane = 64;                   // fit and selection kernels: one wave per workgroup
constexpr int kTile = 32;                   // transpose tile
constexpr int kFitIterations = 5;

// ---- (planes, R, S) -> (planes, S, R)
template <typename T>
__global__ __launch_bounds__(kBlock) void cf_transpose_kernel(const T* __restrict__ src, T* __restrict__ dst, int R, int S, int tr, int ts) {
    __shared__ T tile[kTile][kTile + 1];
    const int bs = blockIdx.x % ts;
    const int64_t rest = blockIdx.x / ts;
    const int br = (int)(rest % tr);
    const int64_t plane = rest / tr;
    const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
    const int64_t base = plane * R * S;
    for (int j = ty; j < kTile; j += kBlock / kTile) {
        const int r = br * kTile + j, s = bs * kTile + tx;
        if (r < R && s < S) tile[j][tx] = src[base + (int64_t)r * S + s];
    }
    __syncthreads();
    for (int j = ty; j < kTile; j += kBlock / kTile) {
        const int s = bs * kTile + j, r = br * kTile + tx;
        if (r < R && s < S) dst[base + (int64_t)s * R + r] = tile[tx][j];
    }
}
template <typename T>
void transpose(rfi_ctx* ctx, const T* src, T* dst, int planes, int R, int S) {
    const int tr = (int)cdiv(R, kTile), ts = (int)cdiv(S, kTile);
    hipLaunchKernelGGL(cf_transpose_kernel<T>, dim3(grid_of((int64_t)planes * tr * ts, "flagger transpose")), dim3(kBlock), 0, ctx->stream,
                       src, dst, R, S, tr, ts);
}

// ---- channel means of a chunk from the transposed plane: Xt, Ft (planes, T, C) -> Mf, Mu (planes, C, nq)
__global__ __launch_bounds__(kBlock) void cf_mean_kernel(const float* __restrict__ Xt, const uint8_t* __restrict__ Ft, int64_t lines, int C,
                                                         int T, int ntime, int nq, float* __restrict__ Mf, uint8_t* __restrict__ Mu) {
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= lines) return;
    const int c = (int)(g % C);
    const int64_t rest = g / C;
    const int q = (int)(rest % nq);
    const int64_t plane = rest / nq;
    const int t0 = q * ntime, t1 = t0 + ntime < T ? t0 + ntime : T;
    double s = 0.0;
    int cnt = 0;
    for (int t = t0; t < t1; ++t) {
        const int64_t o = (plane * T + t) * C + c;
        const bool u = !Ft[o];
        s = s + (u ? (double)Xt[o] : 0.0);
        cnt += u;
    }
    const int64_t o = (plane * C + c) * nq + q;
    Mf[o] = cnt > 0 ? (float)(s / (double)cnt) : 0.0f;
    Mu[o] = cnt > 0 ? 0 : 1;
}

__global__ __launch_bounds__(kBlock) void cf_divide_kernel(const float* __restrict__ X, const double* __restrict__ Bfit, int64_t n, int C,
                                                           int T, int ntime, int nq, float* __restrict__ Y) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int t = (int)(i % T);
    const int64_t row = i / T;                              // plane * C + c
    const double b = Bfit[row * nq + t / ntime];
    const float x = X[i];
    Y[i] = (b > 0.0 && isfinite(b)) ? (float)((double)x / b) : x;
}

// ---- the robust fit.  Element k of line (plane, q, n) lies at ((plane K + q chunk + k) N + n); W holds the flags (non-zero
// == outside the working mask) and is updated in place; R: residual workspace; fit_out (optional): the fit of the last
// iteration that ran.
__global__ __launch_bounds__(kLane) void cf_fit_kernel(const float* __restrict__ Y, uint8_t* __restrict__ W, double* __restrict__ R,
                                                       double* __restrict__ fit_out, int64_t lines, int K, int N, int chunk, int nq,
                                                       int poly, int maxnp, double cutoff) {
    const int64_t g = (int64_t)blockIdx.x * kLane + threadIdx.x;
    if (g >= lines) return;
    const int n = (int)(g % N);
    const int64_t rest = g / N;
    const int q = (int)(rest % nq);
    const int64_t plane = rest / nq;
    const int k0 = q * chunk, L = chunk < K - k0 ? chunk : K - k0;
    const int64_t base = (plane * K + k0) * N + n, stride = N;
    for (int j = 0; j < kFitIterations; ++j) {
        const bool cubic = poly && j > 0;
        const int pieces = cubic ? (2 * j + 1 < maxnp ? 2 * j + 1 : maxnp) : 1, deg = cubic ? 3 : 1;
        int cnt = 0;
        double s1 = 0.0, s2 = 0.0;
        for (int p = 0; p < pieces; ++p) {
            const int a = (int)((int64_t)p * L / pieces), e = (int)((int64_t)(p + 1) * L / pieces), m = e - a;
            if (m == 0) continue;
            const double span = m > 1 ? (double)(m - 1) : 1.0;
            double S[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, B[4] = {0.0, 0.0, 0.0, 0.0};
            int k = 0;
            for (int i = 0; i < m; ++i) {
                const int64_t o = base + (int64_t)(a + i) * stride;
                const bool w = !W[o];
                const double yd = (double)Y[o];
                const double x = (double)(2 * i - (m - 1)) / span;
                const double x2 = x * x, x3 = x2 * x, x4 = x2 * x2, x5 = x4 * x, x6 = x3 * x3;
                k += w;
                S[0] = S[0] + (w ? 1.0 : 0.0);
                S[1] = S[1] + (w ? x : 0.0);
                S[2] = S[2] + (w ? x2 : 0.0);
                S[3] = S[3] + (w ? x3 : 0.0);
                S[4] = S[4] + (w ? x4 : 0.0);
                S[5] = S[5] + (w ? x5 : 0.0);
                S[6] = S[6] + (w ? x6 : 0.0);
                B[0] = B[0] + (w ? 1.0 * yd : 0.0);
                B[1] = B[1] + (w ? x * yd : 0.0);
                B[2] = B[2] + (w ? x2 * yd : 0.0);
                B[3] = B[3] + (w ? x3 * yd : 0.0);
            }
            const int d = deg < k - 1 ? deg : k - 1;
            double A[4][4], b[4], c[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int s = 0; s < 4; ++s) A[r][s] = (r <= d && s <= d) ? S[r + s] : (r == s ? 1.0 : 0.0);
                b[r] = r <= d ? B[r] : 0.0;
            }
#pragma unroll
            for (int pv = 0; pv < 4; ++pv)
#pragma unroll
                for (int r = pv + 1; r < 4; ++r) {
                    const double f = A[r][pv] / A[pv][pv];
#pragma unroll
                    for (int s = pv + 1; s < 4; ++s) A[r][s] = A[r][s] - f * A[pv][s];
                    b[r] = b[r] - f * b[pv];
                }
#pragma unroll
            for (int r = 3; r >= 0; --r) {
                double s = b[r];
#pragma unroll
                for (int t = r + 1; t < 4; ++t) s = s - A[r][t] * c[t];
                c[r] = s / A[r][r];
            }
            for (int i = 0; i < m; ++i) {
                const int64_t o = base + (int64_t)(a + i) * stride;
                const bool w = !W[o];
                const double x = (double)(2 * i - (m - 1)) / span;
                const double fit = ((c[3] * x + c[2]) * x + c[1]) * x + c[0];
                const double r = (double)Y[o] - fit;
                R[o] = r;
                if (fit_out) fit_out[o] = fit;
                cnt += w;
                s1 = s1 + (w ? r : 0.0);
                s2 = s2 + (w ? r * r : 0.0);
            }
        }
        const double nn = (double)cnt, mean = s1 / nn, var = s2 / nn - mean * mean;
        const double sigma = cnt > 0 ? sqrt_rn(var > 0.0 ? var : 0.0) : 0.0;
        if (!(sigma > 0.0)) break;
        const double lim = cutoff * sigma;
        for (int i = 0; i < L; ++i) {
            const int64_t o = base + (int64_t)i * stride;
            if (!W[o] && !(fabs(R[o]) <= lim)) W[o] = 1;
        }
    }
}

void fit(rfi_ctx* ctx, const float* Y, uint8_t* W, double* R, double* fit_out, int planes, int K, int N, int chunk, int poly, int maxnp,
         double cutoff) {
    const int nq = (int)cdiv(K, chunk);
    const int64_t lines = (int64_t)planes * nq * N;
    hipLaunchKernelGGL(cf_fit_kernel, dim3(grid_of(cdiv(lines, kLane), "flagger fit")), dim3(kLane), 0, ctx->stream, Y, W, R, fit_out, lines,
                       K, N, chunk, nq, poly, maxnp, cutoff);
}

// ---- RFlag
template <int IN>
__global__ __launch_bounds__(kBlock) void rf_prepare_kernel(const void* __restrict__ src, const uint8_t* __restrict__ prior, int64_t n,
                                                            double* __restrict__ Z, uint8_t* __restrict__ F) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double re, im;
    if constexpr (IN == RFI_C128) {
        const double* p = static_cast<const double*>(src);
        re = p[2 * i], im = p[2 * i + 1];
    } else {
        const float* p = static_cast<const float*>(src);
        re = (double)p[2 * i], im = (double)p[2 * i + 1];
    }
    const bool fin = isfinite(re) && isfinite(im);
    F[i] = ((prior && prior[i]) || !fin) ? 1 : 0;
    Z[2 * i] = fin ? re : 0.0;
    Z[2 * i + 1] = fin ? im : 0.0;
}

// rms of the unflagged samples of the window around every sample, inside its chunk; -1 where fewer than two
__global__ __launch_bounds__(kBlock) void rf_rms_kernel(const double* __restrict__ Z, const uint8_t* __restrict__ F, int64_t n, int T,
                                                        int ntime, int h, double* __restrict__ D) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int t = (int)(i % T);
    const int64_t row = i - t;
    const int c0 = (t / ntime) * ntime, c1 = (c0 + ntime < T ? c0 + ntime : T) - 1;
    const int lo = t - h > c0 ? t - h : c0, hi = t + h < c1 ? t + h : c1;
    int cnt = 0;
    double sr = 0.0, si = 0.0;
    for (int k = lo; k <= hi; ++k) {
        const bool u = !F[row + k];
        cnt += u;
        sr = sr + (u ? Z[2 * (row + k)] : 0.0);
        si = si + (u ? Z[2 * (row + k) + 1] : 0.0);
    }
    const double nn = (double)cnt, mr = sr / nn, mi = si / nn;
    double vr = 0.0, vi = 0.0;
    for (int k = lo; k <= hi; ++k) {
        const bool u = !F[row + k];
        const double dr = Z[2 * (row + k)] - mr, di = Z[2 * (row + k) + 1] - mi;
        vr = vr + (u ? dr * dr : 0.0);
        vi = vi + (u ? di * di : 0.0);
    }
    const double v = vr / nn + vi / nn;
    D[i] = cnt >= 2 ? sqrt_rn(v > 0.0 ? v : 0.0) : -1.0;
}

// per time sample: the mean spectrum sample A (re, im) and the deviation Dt across the unflagged channels (-1: fewer than two)
__global__ __launch_bounds__(kBlock) void rf_spec_kernel(const double* __restrict__ Z, const uint8_t* __restrict__ F, int64_t cols, int C,
                                                         int T, double* __restrict__ A, double* __restrict__ Dt) {
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= cols) return;
    const int t = (int)(g % T);
    const int64_t base = (g / T) * C * T + t;
    int cnt = 0;
    double sr = 0.0, si = 0.0;
    for (int c = 0; c < C; ++c) {
        const int64_t o = base + (int64_t)c * T;
        const bool u = !F[o];
        cnt += u;
        sr = sr + (u ? Z[2 * o] : 0.0);
        si = si + (u ? Z[2 * o + 1] : 0.0);
    }
    const double nn = (double)cnt, ar = sr / nn, ai = si / nn;
    double vr = 0.0, vi = 0.0;
    for (int c = 0; c < C; ++c) {
        const int64_t o = base + (int64_t)c * T;
        const bool u = !F[o];
        const double dr = Z[2 * o] - ar, di = Z[2 * o + 1] - ai;
        vr = vr + (u ? dr * dr : 0.0);
        vi = vi + (u ? di * di : 0.0);
    }
    const double v = vr / nn + vi / nn;
    A[2 * g] = ar;
    A[2 * g + 1] = ai;
    Dt[g] = cnt >= 2 ? sqrt_rn(v > 0.0 ? v : 0.0) : -1.0;
}

// the value of rank `rank` among the valid (>= 0) entries x of v[0 .. L), or among |x - med| when dev; one wave
__device__ double wave_select(const double* __restrict__ v, int L, unsigned rank, bool dev, double med, unsigned* hist, unsigned* pick) {
    const int tid = threadIdx.x;
    u64 prefix = 0;
    for (int pass = 0; pass < 8; ++pass) {
        const int sh = 56 - 8 * pass;
        const u64 mask = pass ? ~0ull << (sh + 8) : 0ull;
        for (int b = tid; b < 256; b += kLane) hist[b] = 0;
        __syncthreads();
        for (int i = tid; i < L; i += kLane) {
            double x = v[i];
            if (!(x >= 0.0)) continue;
            if (dev) x = fabs(x - med);
            const u64 k = okey(x);
            if ((k & mask) == prefix) atomicAdd(&hist[(unsigned)(k >> sh) & 255u], 1u);
        }
        __syncthreads();
        unsigned loc[4], sum = 0;
        for (int k = 0; k < 4; ++k) {
            loc[k] = hist[tid * 4 + k];
            sum += loc[k];
        }
        unsigned incl = sum;
        for (int o = 1; o < kLane; o <<= 1) {
            const unsigned up = __shfl_up(incl, o, kLane);
            if (tid >= o) incl += up;
        }
        const unsigned excl = incl - sum;
        if (rank >= excl && rank < incl) {
            unsigned c = excl;
            for (int k = 0; k < 4; ++k) {
                if (rank < c + loc[k]) {
                    pick[0] = tid * 4 + k;
                    pick[1] = c;
                    break;
                }
                c += loc[k];
            }
        }
        __syncthreads();
        prefix |= (u64)pick[0] << sh;
        rank -= pick[1];
        __syncthreads();
    }
    return unkey(prefix);
}

// one wave per line (row, chunk) of vals (rows, T): thr = scale * (median + median |x - median|) over the valid entries, +inf
// base for none; with `over` (one value per row) thr = scale * over[row]
__global__ __launch_bounds__(kLane) void rf_thr_kernel(const double* __restrict__ vals, int T, int ntime, int nq, double scale,
                                                       const double* __restrict__ over, double* __restrict__ thr) {
    __shared__ unsigned hist[256];
    __shared__ unsigned pick[2];
    __shared__ unsigned count;
    const int64_t row = blockIdx.x / nq;
    const int q = (int)(blockIdx.x % nq);
    if (over) {
        if (threadIdx.x == 0) thr[blockIdx.x] = scale * over[row];
        return;
    }
    const int t0 = q * ntime, L = ntime < T - t0 ? ntime : T - t0;
    const double* v = vals + row * T + t0;
    if (threadIdx.x == 0) count = 0;
    __syncthreads();
    unsigned mine = 0;
    for (int i = threadIdx.x; i < L; i += kLane) mine += v[i] >= 0.0 ? 1u : 0u;
    if (mine) atomicAdd(&count, mine);
    __syncthreads();
    const unsigned n = count;
    double base = INFINITY;
    if (n) {                                                // uniform across the wave
        const double lo = wave_select(v, L, (n - 1) / 2, false, 0.0, hist, pick);
        const double med = (n & 1u) ? lo : (lo + wave_select(v, L, n / 2, false, 0.0, hist, pick)) / 2.0;
        const double dl = wave_select(v, L, (n - 1) / 2, true, med, hist, pick);
        const double mad = (n & 1u) ? dl : (dl + wave_select(v, L, n / 2, true, med, hist, pick)) / 2.0;
        base = med + mad;
    }
    if (threadIdx.x == 0) thr[blockIdx.x] = scale * base;
}

__global__ __launch_bounds__(kBlock) void rf_flag_kernel(const double* __restrict__ Z, const uint8_t* __restrict__ F,
                                                         const double* __restrict__ D, const double* __restrict__ thr_t,
                                                         const double* __restrict__ A, const double* __restrict__ Dt,
                                                         const double* __restrict__ thr_f, int64_t n, int C, int T, int ntime, int nq,
                                                         uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int t = (int)(i % T), q = t / ntime;
    const int64_t row = i / T, plane = row / C, col = plane * T + t;
    const bool f = F[i] != 0;
    const double rms = D[i];
    const bool hit_t = rms >= 0.0 && rms > thr_t[row * nq + q];
    const double dr = Z[2 * i] - A[2 * col], di = Z[2 * i + 1] - A[2 * col + 1];
    const double dist = sqrt_rn(dr * dr + di * di);
    const bool hit_f = !f && Dt[col] >= 0.0 && dist > thr_f[plane * nq + q];
    out[i] = (f || hit_t || hit_f) ? 1 : 0;
}

// ---- extend: every kernel reads Fin (a snapshot) and writes all of Fout
__global__ __launch_bounds__(kBlock) void ex_around_kernel(const uint8_t* __restrict__ Fin, uint8_t* __restrict__ Fout, int64_t n, int C,
                                                           int T, int ntime, int grow) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    bool f = Fin[i] != 0;
    if (grow && !f) {
        const int t = (int)(i % T), c = (int)((i / T) % C);
        const int c0 = (t / ntime) * ntime, c1 = (c0 + ntime < T ? c0 + ntime : T) - 1;
        int nb = 0;
        for (int dc = -1; dc <= 1; ++dc)
            for (int dt = -1; dt <= 1; ++dt) {
                if ((dc == 0 && dt == 0) || c + dc < 0 || c + dc >= C || t + dt < c0 || t + dt > c1) continue;
                nb += Fin[i + (int64_t)dc * T + dt] != 0;
            }
        f = nb > 4;
    }
    Fout[i] = f ? 1 : 0;
}
// one wave per (row, chunk): the whole line when more than `grow` per cent of it is flagged
__global__ __launch_bounds__(kLane) void ex_growtime_kernel(const uint8_t* __restrict__ Fin, uint8_t* __restrict__ Fout, int T, int ntime,
                                                            int nq, double grow) {
    __shared__ int count;
    const int64_t row = blockIdx.x / nq;
    const int q = (int)(blockIdx.x % nq);
    const int t0 = q * ntime, L = ntime < T - t0 ? ntime : T - t0;
    const uint8_t* in = Fin + row * T + t0;
    uint8_t* out = Fout + row * T + t0;
    if (threadIdx.x == 0) count = 0;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < L; i += kLane) mine += in[i] != 0;
    if (mine) atomicAdd(&count, mine);
    __syncthreads();
    const bool all = (double)(100ll * count) > grow * (double)L;
    for (int i = threadIdx.x; i < L; i += kLane) out[i] = (all || in[i]) ? 1 : 0;
}
__global__ __launch_bounds__(kBlock) void ex_growfreq_kernel(const uint8_t* __restrict__ Fin, uint8_t* __restrict__ Fout, int64_t cols,
                                                             int C, int T, double grow) {
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= cols) return;
    const int64_t base = (g / T) * C * T + g % T;
    int count = 0;
    for (int c = 0; c < C; ++c) count += Fin[base + (int64_t)c * T] != 0;
    const bool all = (double)(100ll * count) > grow * (double)C;
    for (int c = 0; c < C; ++c) Fout[base + (int64_t)c * T] = (all || Fin[base + (int64_t)c * T]) ? 1 : 0;
}
__global__ __launch_bounds__(kBlock) void ex_near_kernel(const uint8_t* __restrict__ Fin, uint8_t* __restrict__ Fout, int64_t n, int C,
                                                         int T, int ntime, int axis) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    bool f = Fin[i] != 0;
    if (axis == 1) {
        const int t = (int)(i % T);
        const int c0 = (t / ntime) * ntime, c1 = (c0 + ntime < T ? c0 + ntime : T) - 1;
        if (t > c0) f = f || Fin[i - 1];
        if (t < c1) f = f || Fin[i + 1];
    } else {
        const int c = (int)((i / T) % C);
        if (c > 0) f = f || Fin[i - T];
        if (c < C - 1) f = f || Fin[i + T];
    }
    Fout[i] = f ? 1 : 0;
}

}  // namespace

// ---- TFCrop.  Workspace: X, Y, Tf floats and F, Ft bytes and R doubles of n = planes C T samples; Mf floats, Mu bytes, Bfit
// doubles of planes C nq.  Returns the buffer (inside ws) that holds the flags.
size_t tfcrop_ws_bytes(int planes, int C, int T, int ntime) {
    const size_t n = (size_t)planes * C * T, m = (size_t)planes * C * (size_t)cdiv(T, ntime);
    return 3 * al(n * 4) + 2 * al(n) + al(n * 8) + al(m * 4) + al(m) + al(m * 8);
}
uint8_t* launch_tfcrop_flag(rfi_ctx* ctx, const void* src, int dtype, const uint8_t* prior, int planes, int C, int T,
                            const rfi_tfcrop_config& cfg, void* ws) {
    const int ntime = cfg.ntime, nq = (int)cdiv(T, ntime);
    const int64_t n = (int64_t)planes * C * T, m = (int64_t)planes * C * nq;
    ProfScope ps(ctx, FAM_METRICS, 0, (double)n * 28 * 2 * kFitIterations, "tfcrop_flag");
    Carve cv{static_cast<char*>(ws)};
    float *X = cv.take<float>(n), *Y = cv.take<float>(n), *Tf = cv.take<float>(n);
    uint8_t *F = cv.take<uint8_t>(n), *Ft = cv.take<uint8_t>(n);
    double* R = cv.take<double>(n);
    float* Mf = cv.take<float>(m);
    uint8_t* Mu = cv.take<uint8_t>(m);
    double* Bfit = cv.take<double>(m);
    const dim3 ge(grid_of(cdiv(n, kBlock), "tfcrop")), b(kBlock);
    launch_st_prepare(ctx, src, dtype, prior, n, X, F);
    // bandpass: channel means per chunk, their robust fit along frequency (its flags are dropped), the division
    transpose(ctx, X, Tf, planes, C, T);
    transpose(ctx, F, Ft, planes, C, T);
    hipLaunchKernelGGL(cf_mean_kernel, dim3(grid_of(cdiv(m, kBlock), "tfcrop")), b, 0, ctx->stream, Tf, Ft, m, C, T, ntime, nq, Mf, Mu);
    fit(ctx, Mf, Mu, R, Bfit, planes, C, nq, C, cfg.freqfit, cfg.maxnpieces, cfg.freqcutoff);
    hipLaunchKernelGGL(cf_divide_kernel, ge, b, 0, ctx->stream, X, Bfit, n, C, T, ntime, nq, Y);
    static const int kStages[4][2] = {{1, 0}, {0, 1}, {1, -1}, {0, -1}};      // by flagdimension: 1 time, 0 frequency, -1 none
    for (int s = 0; s < 2; ++s) {
        const int stage = kStages[cfg.flagdimension][s];
        if (stage == 1) {
            transpose(ctx, Y, Tf, planes, C, T);
            transpose(ctx, F, Ft, planes, C, T);
            fit(ctx, Tf, Ft, R, nullptr, planes, T, C, ntime, cfg.timefit, cfg.maxnpieces, cfg.timecutoff);
            transpose(ctx, Ft, F, planes, T, C);
        } else if (stage == 0) {
            fit(ctx, Y, F, R, nullptr, planes, C, T, C, cfg.freqfit, cfg.maxnpieces, cfg.freqcutoff);
        }
    }
    check_launch("tfcrop_flag");
    return F;
}

// ---- RFlag.  timedev (planes C doubles) and freqdev (planes doubles) are device pointers or null.
size_t rflag_ws_bytes(int planes, int C, int T, int ntime) {
    const size_t n = (size_t)planes * C * T, nq = (size_t)cdiv(T, ntime), cols = (size_t)planes * T;
    return al(n * 16) + 2 * al(n) + al(n * 8) + al(cols * 16) + al(cols * 8) + al((size_t)planes * C * nq * 8) + al(planes * nq * 8);
}
uint8_t* launch_rflag_flag(rfi_ctx* ctx, const void* src, int dtype, const uint8_t* prior, int planes, int C, int T,
                           const rfi_rflag_config& cfg, const double* timedev, const double* freqdev, void* ws) {
    const int ntime = cfg.ntime, nq = (int)cdiv(T, ntime);
    const int64_t n = (int64_t)planes * C * T, cols = (int64_t)planes * T, rows = (int64_t)planes * C;
    ProfScope ps(ctx, FAM_METRICS, 0, (double)n * 100, "rflag_flag");
    Carve cv{static_cast<char*>(ws)};
    double* Z = cv.take<double>(2 * n);
    uint8_t *F = cv.take<uint8_t>(n), *out = cv.take<uint8_t>(n);
    double *D = cv.take<double>(n), *A = cv.take<double>(2 * cols), *Dt = cv.take<double>(cols);
    double *thr_t = cv.take<double>(rows * nq), *thr_f = cv.take<double>((int64_t)planes * nq);
    const dim3 ge(grid_of(cdiv(n, kBlock), "rflag")), b(kBlock);
    if (dtype == RFI_C128) hipLaunchKernelGGL(rf_prepare_kernel<RFI_C128>, ge, b, 0, ctx->stream, src, prior, n, Z, F);
    else hipLaunchKernelGGL(rf_prepare_kernel<RFI_C64>, ge, b, 0, ctx->stream, src, prior, n, Z, F);
    const int h = cfg.winsize / 2 < T ? cfg.winsize / 2 : T;
    hipLaunchKernelGGL(rf_rms_kernel, ge, b, 0, ctx->stream, Z, F, n, T, ntime, h, D);
    hipLaunchKernelGGL(rf_thr_kernel, dim3(grid_of(rows * nq, "rflag thresholds")), dim3(kLane), 0, ctx->stream, D, T, ntime, nq,
                       cfg.timedevscale, timedev, thr_t);
    hipLaunchKernelGGL(rf_spec_kernel, dim3(grid_of(cdiv(cols, kBlock), "rflag")), b, 0, ctx->stream, Z, F, cols, C, T, A, Dt);
    hipLaunchKernelGGL(rf_thr_kernel, dim3(grid_of((int64_t)planes * nq, "rflag thresholds")), dim3(kLane), 0, ctx->stream, Dt, T, ntime, nq,
                       cfg.freqdevscale, freqdev, thr_f);
    hipLaunchKernelGGL(rf_flag_kernel, ge, b, 0, ctx->stream, Z, F, D, thr_t, A, Dt, thr_f, n, C, T, ntime, nq, out);
    check_launch("rflag_flag");
    return out;
}

// ---- extend.  Workspace: two byte planes of n; Fin is only read.
size_t extend_ws_bytes(int planes, int C, int T) { return 2 * al((size_t)planes * C * T); }
uint8_t* launch_extend_flags(rfi_ctx* ctx, const uint8_t* Fin, int planes, int C, int T, const rfi_extend_config& cfg, void* ws) {
    const int ntime = cfg.ntime, nq = (int)cdiv(T, ntime);
    const int64_t n = (int64_t)planes * C * T;
    ProfScope ps(ctx, FAM_METRICS, 0, (double)n * 10, "extend_flags");
    Carve cv{static_cast<char*>(ws)};
    uint8_t *cur = cv.take<uint8_t>(n), *other = cv.take<uint8_t>(n);
    const dim3 ge(grid_of(cdiv(n, kBlock), "extend")), b(kBlock);
    hipLaunchKernelGGL(ex_around_kernel, ge, b, 0, ctx->stream, Fin, cur, n, C, T, ntime, cfg.growaround ? 1 : 0);
    if (cfg.growtime < 100.0) {
        hipLaunchKernelGGL(ex_growtime_kernel, dim3(grid_of((int64_t)planes * C * nq, "extend growtime")), dim3(kLane), 0, ctx->stream, cur,
                           other, T, ntime, nq, cfg.growtime);
        std::swap(cur, other);
    }
    if (cfg.growfreq < 100.0) {
        hipLaunchKernelGGL(ex_growfreq_kernel, dim3(grid_of(cdiv((int64_t)planes * T, kBlock), "extend")), b, 0, ctx->stream, cur, other,
                           (int64_t)planes * T, C, T, cfg.growfreq);
        std::swap(cur, other);
    }
    if (cfg.flagneartime) {
        hipLaunchKernelGGL(ex_near_kernel, ge, b, 0, ctx->stream, cur, other, n, C, T, ntime, 1);
        std::swap(cur, other);
    }
    if (cfg.flagnearfreq) {
        hipLaunchKernelGGL(ex_near_kernel, ge, b, 0, ctx->stream, cur, other, n, C, T, ntime, 0);
        std::swap(cur, other);
    }
    check_launch("extend_flags");
    return cur;
}

}  // namespace rfi
