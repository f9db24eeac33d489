// Inverse of the tiling of Preprocessor.create_dataset(inference_mode=True): per-patch model outputs -> one flag (and
// optionally one combined probability) per waterfall pixel.  Gather form: a thread owns one output pixel, derives the
// (view, tile row, tile column) triples that cover it from the grid arithmetic of rfi_tiling (include/rfi_hip.h) and
// reads those patch pixels in a fixed order -- views ascending, then tile rows, then tile columns.  No atomics, no
// scatter: the result is bitwise reproducible.  Memory bound: 4 B read per covering tile, 1 (+4) B written per pixel.
// Views 0/1 read along patch rows (coalesced); views 2/3 walk a patch column across a wavefront, so a block spans
// 4 waterfall rows whose reads share those cache lines.
#include <algorithm>

#include "kernels.hpp"

namespace rfi {
namespace {

// tile origins along an axis of length L: n = 1 when L <= ps, else k + 1 with k = ceil((L - ps) / s); origin i = i * s,
// except the last one under edge = shift, which is L - ps (no padded tile)
__host__ __device__ inline int axis_tiles(int L, int ps, int s) { return L <= ps ? 1 : (L - ps + s - 1) / s + 1; }

struct StitchGrid {
    int C, T, ps, s, shift, views;
    int nC, nT;                    // tiles along C and along T
    int64_t ppp;                   // patches per plane
};

__device__ __forceinline__ int origin(int i, int n, int L, const StitchGrid& g) {
    return (g.shift && i == n - 1 && L > g.ps) ? L - g.ps : i * g.s;
}

// kind 0: values are logits (sigmoid as threshold_kernel computes it), 1: probabilities as they are
template <int KIND, int COMBINE>
__global__ void __launch_bounds__(256) stitch_kernel(const float* __restrict__ vals, StitchGrid g, float thr,
                                                     uint8_t* __restrict__ flags, float* __restrict__ prob) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y * blockDim.y + threadIdx.y;
    const int plane = blockIdx.z;
    if (t >= g.T || c >= g.C) return;
    const int64_t ps2 = (int64_t)g.ps * g.ps;
    const float* pv = vals + (int64_t)plane * g.ppp * ps2;
    float acc = 0.0f;
    int cnt = 0;
    for (int v = 0; v < g.views; ++v) {
        const bool tr = v >= 2;
        const int Hv = tr ? g.T : g.C, Wv = tr ? g.C : g.T;
        const int nr = tr ? g.nT : g.nC, nc = tr ? g.nC : g.nT;
        // waterfall pixel (c, t) in view coordinates (y, x); views: 0 plane, 1 plane[::-1,:], 2 plane.T, 3 plane.T[::-1,:]
        const int yy = tr ? t : c, x = tr ? c : t;
        const int y = (v & 1) ? Hv - 1 - yy : yy;
        const int64_t vbase = (int64_t)v * nr * nc;
        const int i0 = y >= g.ps ? (y - g.ps) / g.s + 1 : 0;
        const int j0 = x >= g.ps ? (x - g.ps) / g.s + 1 : 0;
        for (int i = i0; i < nr; ++i) {
            const int r0 = origin(i, nr, Hv, g);
            if (r0 > y) break;
            if (y >= r0 + g.ps) continue;
            for (int j = j0; j < nc; ++j) {
                const int c0 = origin(j, nc, Wv, g);
                if (c0 > x) break;
                if (x >= c0 + g.ps) continue;
                const float raw = pv[(vbase + (int64_t)i * nc + j) * ps2 + (int64_t)(y - r0) * g.ps + (x - c0)];
                const float p = KIND == 0 ? 1.0f / (1.0f + expf(-raw)) : raw;
                if (COMBINE == 0) acc += p;
                else acc = (cnt == 0 || p > acc) ? p : acc;
                ++cnt;
            }
        }
    }
    const float r = COMBINE == 0 ? acc / (float)cnt : acc;
    const int64_t o = ((int64_t)plane * g.C + c) * g.T + t;
    flags[o] = r > thr ? 1 : 0;
    if (prob) prob[o] = r;
}

}  // namespace

int64_t tiling_patches_per_plane(int C, int T, const rfi_tiling& tl) {
    return (int64_t)tl.views * axis_tiles(C, tl.ps, tl.stride) * axis_tiles(T, tl.ps, tl.stride);
}

void check_tiling(const rfi_tiling& tl) {
    RFI_REQUIRE(tl.ps > 0, "tiling: patch size must be positive");
    RFI_REQUIRE(tl.stride >= 1 && tl.stride <= tl.ps, "tiling: stride must lie in [1, patch size]");
    RFI_REQUIRE(tl.edge == RFI_EDGE_PAD || tl.edge == RFI_EDGE_SHIFT, "tiling: edge must be RFI_EDGE_PAD or RFI_EDGE_SHIFT");
    RFI_REQUIRE(tl.views == 1 || tl.views == 2 || tl.views == 4, "tiling: views must be 1, 2 or 4");
}

void launch_stitch(rfi_ctx* ctx, const float* values, int kind, int n_planes, int C, int T, const rfi_tiling& tl,
                   int combine, float threshold, uint8_t* flags, float* prob) {
    RFI_REQUIRE(kind == RFI_VALUES_LOGITS || kind == RFI_VALUES_PROBS, "stitch: kind must be logits (0) or probabilities (1)");
    RFI_REQUIRE(combine == RFI_COMBINE_MEAN || combine == RFI_COMBINE_MAX, "stitch: combine must be mean (0) or max (1)");
    if (n_planes == 0) return;
    StitchGrid g{C, T, tl.ps, tl.stride, tl.edge == RFI_EDGE_SHIFT ? 1 : 0, tl.views, axis_tiles(C, tl.ps, tl.stride),
                 axis_tiles(T, tl.ps, tl.stride), 0};
    g.ppp = (int64_t)g.views * g.nC * g.nT;
    const double px = (double)n_planes * C * T;
    // bytes: every covering tile read once (about views x (ps / stride)^2 per pixel), flags and probabilities written
    const double cover = (double)g.views * ((double)tl.ps / tl.stride) * ((double)tl.ps / tl.stride);
    ProfScope ps_(ctx, FAM_METRICS, 0, px * (4 * cover + 1 + (prob ? 4 : 0)), "stitch");
    RFI_REQUIRE(cdiv(C, 4) <= 65535, "stitch: at most 262140 channels");
    const dim3 block(64, 4);
    for (int p0 = 0; p0 < n_planes; p0 += 65535) {           // grid.z: at most 65535 planes per launch
        const int np = std::min(65535, n_planes - p0);
        const dim3 grid((unsigned)cdiv(T, 64), (unsigned)cdiv(C, 4), (unsigned)np);
        const float* v = values + (int64_t)p0 * g.ppp * tl.ps * tl.ps;
        uint8_t* f = flags + (int64_t)p0 * C * T;
        float* pr = prob ? prob + (int64_t)p0 * C * T : nullptr;
#define RFI_STITCH(K, M) hipLaunchKernelGGL((stitch_kernel<K, M>), grid, block, 0, ctx->stream, v, g, threshold, f, pr)
        if (kind == 0) {
            if (combine == 0) RFI_STITCH(0, 0);
            else RFI_STITCH(0, 1);
        } else {
            if (combine == 0) RFI_STITCH(1, 0);
            else RFI_STITCH(1, 1);
        }
#undef RFI_STITCH
        check_launch("stitch");
    }
}

}  // namespace rfi
