// Inverse of the tiling of Preprocessor.create_dataset(inference_mode=True): per-patch model outputs -> one flag (and
// optionally one combined probability) per waterfall pixel.  Gather form: a thread owns one output pixel and reads the
// patch pixels of the tiles that cover it in the order of for_each_covering_tile (tiling.hpp, which holds the grid
// arithmetic of rfi_tiling) -- views ascending, then tile rows, then tile columns.  No atomics, no
// scatter: the result is bitwise reproducible.  Memory bound: 4 B read per covering tile, 1 (+4) B written per pixel.
// Views 0/1 read along patch rows (coalesced); views 2/3 walk a patch column across a wavefront, so a block spans
// 4 waterfall rows whose reads share those cache lines.
#include <algorithm>

#include "kernels.hpp"
#include "tiling.hpp"

namespace rfi {
namespace {

// kind 0: values are logits (sigmoid as threshold_kernel computes it), 1: probabilities as they are
// K classes, channel-last in a patch pixel: grid.z counts (plane, class) pairs, which is also the output plane
template <int KIND, int COMBINE>
__global__ void __launch_bounds__(256) stitch_kernel(const float* __restrict__ vals, TileGrid g, int K, float thr,
                                                     uint8_t* __restrict__ flags, float* __restrict__ prob) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y * blockDim.y + threadIdx.y;
    const int plane = blockIdx.z;
    if (t >= g.T || c >= g.C) return;
    const int64_t ps2 = (int64_t)g.ps * g.ps * K;
    const float* pv = vals + (int64_t)(plane / K) * g.ppp * ps2 + plane % K;
    float acc = 0.0f;
    int cnt = 0;
    for_each_covering_tile<int64_t>(g, c, t, [&](int64_t tile, int64_t off) {
        const float raw = pv[tile * ps2 + off * K];
        const float p = KIND == 0 ? 1.0f / (1.0f + expf(-raw)) : raw;
        if (COMBINE == 0) acc += p;
        else acc = (cnt == 0 || p > acc) ? p : acc;
        ++cnt;
    });
    const float r = COMBINE == 0 ? acc / (float)cnt : acc;
    const int64_t o = ((int64_t)plane * g.C + c) * g.T + t;
    flags[o] = r > thr ? 1 : 0;
    if (prob) prob[o] = r;
}

}  // namespace

int64_t tiling_patches_per_plane(int C, int T, const rfi_tiling& tl) {
    return make_tile_grid(C, T, tl).ppp;
}

void check_tiling(const rfi_tiling& tl) {
    RFI_REQUIRE(tl.ps > 0, "tiling: patch size must be positive");
    RFI_REQUIRE(tl.stride >= 1 && tl.stride <= tl.ps, "tiling: stride must lie in [1, patch size]");
    RFI_REQUIRE(tl.edge == RFI_EDGE_PAD || tl.edge == RFI_EDGE_SHIFT, "tiling: edge must be RFI_EDGE_PAD or RFI_EDGE_SHIFT");
    RFI_REQUIRE(tl.views == 1 || tl.views == 2 || tl.views == 4, "tiling: views must be 1, 2 or 4");
}

void launch_stitch(rfi_ctx* ctx, const float* values, int kind, int n_planes, int C, int T, const rfi_tiling& tl,
                   int combine, float threshold, uint8_t* flags, float* prob, int n_classes) {
    RFI_REQUIRE(n_classes >= 1 && n_classes <= 65535, "stitch: 1 to 65535 classes");
    RFI_REQUIRE(kind == RFI_VALUES_LOGITS || kind == RFI_VALUES_PROBS, "stitch: kind must be logits (0) or probabilities (1)");
    RFI_REQUIRE(combine == RFI_COMBINE_MEAN || combine == RFI_COMBINE_MAX, "stitch: combine must be mean (0) or max (1)");
    if (n_planes == 0) return;
    const TileGrid g = make_tile_grid(C, T, tl);
    const double px = (double)n_planes * n_classes * C * T;
    // bytes: every covering tile read once (about views x (ps / stride)^2 per pixel), flags and probabilities written
    const double cover = (double)g.views * ((double)tl.ps / tl.stride) * ((double)tl.ps / tl.stride);
    ProfScope ps_(ctx, FAM_METRICS, 0, px * (4 * cover + 1 + (prob ? 4 : 0)), "stitch");
    RFI_REQUIRE(cdiv(C, 4) <= 65535, "stitch: at most 262140 channels");
    const dim3 block(64, 4);
    const int step = 65535 / n_classes;                      // grid.z: at most 65535 (plane, class) pairs per launch
    for (int p0 = 0; p0 < n_planes; p0 += step) {
        const int np = std::min(step, n_planes - p0);
        const dim3 grid((unsigned)cdiv(T, 64), (unsigned)cdiv(C, 4), (unsigned)(np * n_classes));
        const float* v = values + (int64_t)p0 * g.ppp * tl.ps * tl.ps * n_classes;
        uint8_t* f = flags + (int64_t)p0 * n_classes * C * T;
        float* pr = prob ? prob + (int64_t)p0 * n_classes * C * T : nullptr;
#define RFI_STITCH(K, M) hipLaunchKernelGGL((stitch_kernel<K, M>), grid, block, 0, ctx->stream, v, g, n_classes, threshold, f, pr)
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
