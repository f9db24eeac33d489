// Scoring detections per instance (include/rfi_hip.h, "instance matching"): bit-packed mask planes, the pairwise mask and
// box IoU of every (detection, ground truth) of an image, and COCO-style greedy matching at T thresholds in one launch.
// Integer work, and float32 / float64 work in a pinned operation order: every result is exact and independent of launch
// geometry.  No atomics: every output word has one writer.
//
//   pack    one workgroup per plane; a wave turns 64 consecutive bytes of a row into one word with __ballot, so the word,
//           its popcount and whether it is non-zero are wave-uniform.  Area and extent of the plane are combined across
//           the workgroup's waves through LDS.
//   iou     one workgroup per (image, detection).  The words of the detection's extent window are staged in LDS when they
//           fit (kStageWords; read in place otherwise); waves take the ground truths in turn, lanes stride over the words
//           of the window the two extents share.  Pairs with disjoint extents cost two extent loads.
//   match   one wave per (image, threshold): lane l owns ground truths l, l + 64, l + 128, l + 192.  Detections are ranked
//           by counting, then taken in that order; the best free ground truth of one detection is one wave-wide maximum of
//           (IoU bits << 32 | ~slot), which is greatest IoU first, lowest slot on ties.
#include "kernels.hpp"
#include "launch_common.hpp"
#include "select_common.hpp"

namespace rfi {
namespace {

constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr int kMaxSlots = 256;             // D and G: detect's post_nms cap and MAX_INSTANCES
constexpr int kMaxThresholds = 32;
constexpr int kStageWords = 4096;          // 32 KB of LDS: a full 512 x 512 plane
constexpr int kPackBlock = 512, kPackWaves = kPackBlock / 64, kPackUnroll = 4;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- pack.  grid (m), block kPackBlock.  bits [m][H][Wc], area [m], extent [m][4] = (row0, col0, row1, col1) of the non-zero
// words, (0, 0, 0, 0) for an empty plane
__global__ void __launch_bounds__(kPackBlock) pack_masks_kernel(const uint8_t* __restrict__ masks, int H, int W, int Wc,
                                                                u64* __restrict__ bits, int* __restrict__ area, int* __restrict__ extent) {
    __shared__ int s_red[kPackWaves][5];
    const int64_t plane = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t* src = masks + plane * H * W;
    u64* dst = bits + plane * H * Wc;
    const int words = H * Wc;                                     // (<= H W <= 2^24)
    int a = 0, r0 = H, c0 = Wc, r1 = 0, c1 = 0;                    // wave-uniform
    // a wave takes kPackUnroll consecutive words at a time: that many byte loads are in flight before the first vote
    for (int k0 = wave * kPackUnroll; k0 < words; k0 += kPackWaves * kPackUnroll) {
        bool on[kPackUnroll];
#pragma unroll
        for (int u = 0; u < kPackUnroll; ++u) {
            const int k = k0 + u, r = k / Wc, c = k - r * Wc, x = c * 64 + lane;
            on[u] = k < words && x < W && src[(int64_t)r * W + x] != 0;
        }
        u64 mine = 0;                                             // lane u keeps word k0 + u: one store for all of them
#pragma unroll
        for (int u = 0; u < kPackUnroll; ++u) {
            const int k = k0 + u, r = k / Wc, c = k - r * Wc;
            const u64 word = __ballot(on[u]);
            if (lane == u) mine = word;
            if (word) {                                           // (a word past the end has no bit set)
                a += __popcll(word);
                r0 = min(r0, r); r1 = max(r1, r + 1);
                c0 = min(c0, c); c1 = max(c1, c + 1);
            }
        }
        if (lane < kPackUnroll && k0 + lane < words) dst[k0 + lane] = mine;
    }
    if (lane == 0) {
        s_red[wave][0] = a; s_red[wave][1] = r0; s_red[wave][2] = c0; s_red[wave][3] = r1; s_red[wave][4] = c1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < kPackWaves; ++v) {
            a += s_red[v][0];
            r0 = min(r0, s_red[v][1]); c0 = min(c0, s_red[v][2]);
            r1 = max(r1, s_red[v][3]); c1 = max(c1, s_red[v][4]);
        }
        if (a == 0) r0 = c0 = r1 = c1 = 0;
        area[plane] = a;
        int* e = extent + plane * 4;
        e[0] = r0; e[1] = c0; e[2] = r1; e[3] = c1;
    }
}

// ---- mask IoU.  grid (D, n), block kBlock.  A side is (bits, area, extent) over m planes, the planes of image i being
// base[i] .. base[i] + count[i] - 1; a plane index outside 0 .. m - 1 counts as an empty mask (never read)
struct Side {
    const u64* bits;
    const int* area;
    const int* extent;
    const int* count;
    const int* base;
    int64_t m;
};

__global__ void __launch_bounds__(kBlock) mask_iou_kernel(Side det, Side gt, int D, int G, int H, int Wc, int* __restrict__ inter,
                                                          float* __restrict__ iou) {
    __shared__ u64 s_win[kStageWords];
    __shared__ int s_inter[kMaxSlots], s_area[kMaxSlots];
    const int i = blockIdx.y, d = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int* out_inter = inter + ((int64_t)i * D + d) * G;
    float* out_iou = iou + ((int64_t)i * D + d) * G;
    const int dcount = clampi(det.count[i], 0, D), gcount = clampi(gt.count[i], 0, G);
    const int64_t dp = (int64_t)det.base[i] + d;
    if (d >= dcount || dp < 0 || dp >= det.m) {                  // (uniform over the workgroup)
        for (int g = threadIdx.x; g < G; g += kBlock) { out_inter[g] = 0; out_iou[g] = 0.0f; }
        return;
    }
    const int darea = det.area[dp];
    const int dr0 = det.extent[dp * 4], dc0 = det.extent[dp * 4 + 1], dr1 = det.extent[dp * 4 + 2], dc1 = det.extent[dp * 4 + 3];
    // an extent a caller made up is cut to the plane: nothing outside it is ever addressed
    const int r0 = clampi(dr0, 0, H), c0 = clampi(dc0, 0, Wc), r1 = clampi(dr1, r0, H), c1 = clampi(dc1, c0, Wc);
    const int dw = c1 - c0, dwords = (r1 - r0) * dw;
    const u64* dbits = det.bits + dp * H * Wc;
    const bool staged = dwords <= kStageWords;
    if (staged) {
        for (int k = threadIdx.x; k < dwords; k += kBlock) {
            const int r = k / dw, c = k - r * dw;
            s_win[k] = dbits[(int64_t)(r0 + r) * Wc + c0 + c];
        }
    }
    __syncthreads();
    for (int g = wave; g < G; g += kWaves) {
        int acc = 0, garea = 0;
        const int64_t gp = (int64_t)gt.base[i] + g;
        if (g < gcount && gp >= 0 && gp < gt.m) {
            garea = gt.area[gp];
            const int rr0 = max(r0, gt.extent[gp * 4]), cc0 = max(c0, gt.extent[gp * 4 + 1]);
            const int rr1 = min(r1, gt.extent[gp * 4 + 2]), cc1 = min(c1, gt.extent[gp * 4 + 3]);
            if (rr0 < rr1 && cc0 < cc1) {
                const int cw = cc1 - cc0, nw = (rr1 - rr0) * cw;
                const u64* gbits = gt.bits + gp * H * Wc;
                for (int k = lane; k < nw; k += 64) {
                    const int r = rr0 + k / cw, c = cc0 + k % cw;
                    const u64 a = staged ? s_win[(r - r0) * dw + (c - c0)] : dbits[(int64_t)r * Wc + c];
                    acc += __popcll(a & gbits[(int64_t)r * Wc + c]);
                }
                acc = wave_isum(acc);
            }
        } else {
            garea = -1;                                           // behind the count: the entry is 0
        }
        if (lane == 0) { s_inter[g] = acc; s_area[g] = garea; }
    }
    __syncthreads();
    for (int g = threadIdx.x; g < G; g += kBlock) {
        const int in = s_inter[g], ga = s_area[g];
        const int64_t uni = ga < 0 ? 0 : (int64_t)darea + ga - in;
        out_inter[g] = ga < 0 ? 0 : in;
        out_iou[g] = uni == 0 ? 0.0f : (float)((double)in / (double)uni);
    }
}

// ---- box IoU, iou_of's operation order (rpn_kernels.hip) in float32.  One thread per (image, detection, ground truth)
__global__ void __launch_bounds__(kBlock) box_iou_kernel(const float* __restrict__ dboxes, const int* __restrict__ dcount,
                                                         const float* __restrict__ gboxes, const int* __restrict__ gcount, int D, int G,
                                                         int64_t total, float* __restrict__ iou) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= total) return;
    const int g = (int)(e % G), d = (int)((e / G) % D);
    const int64_t i = e / ((int64_t)G * D);
    float v = 0.0f;
    if (d < dcount[i] && g < gcount[i]) {
        const float* a = dboxes + (i * D + d) * 4;
        const float* b = gboxes + (i * G + g) * 4;
        const float ax1 = a[0], ay1 = a[1], ax2 = a[2], ay2 = a[3], bx1 = b[0], by1 = b[1], bx2 = b[2], by2 = b[3];
        const float iw = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.0f), ih = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.0f);
        const float in = iw * ih;
        const float uni = ((ax2 - ax1) * (ay2 - ay1) + (bx2 - bx1) * (by2 - by1)) - in;
        v = uni <= 0.0f ? 0.0f : in / uni;
    }
    iou[e] = v;
}

// ---- greedy matching.  grid (T, n), block 64 (one wave)
struct Thresholds {
    float t[kMaxThresholds];
};

__global__ void __launch_bounds__(64) match_instances_kernel(const float* __restrict__ iou, const float* __restrict__ scores,
                                                             const int* __restrict__ dlabels, const int* __restrict__ dcount,
                                                             const int* __restrict__ glabels, const int* __restrict__ gcount, int D, int G,
                                                             int T, Thresholds thr, int class_aware, int* __restrict__ det_match,
                                                             int* __restrict__ gt_match) {
    __shared__ unsigned s_key[kMaxSlots];
    __shared__ int s_order[kMaxSlots], s_dm[kMaxSlots], s_dl[kMaxSlots];
    const int i = blockIdx.y, ti = blockIdx.x, lane = threadIdx.x;
    const float t = thr.t[ti];
    const int nd = clampi(dcount[i], 0, D), ng = clampi(gcount[i], 0, G);
    // descending score, ties by ascending slot, by counting.  The key orders every float32 (-0 as +0; NaN by its bits), so
    // the ranks are a permutation whatever the scores hold
    for (int d = lane; d < D; d += 64) {
        s_dm[d] = -1;
        if (d < nd) {
            const float s = scores[(int64_t)i * D + d];
            s_key[d] = okey(s == 0.0f ? 0.0f : s);
            s_dl[d] = dlabels[(int64_t)i * D + d];
        }
    }
    __syncthreads();
    for (int d = lane; d < nd; d += 64) {
        const unsigned k = s_key[d];
        int rank = 0;
        for (int e = 0; e < nd; ++e) {
            const unsigned ke = s_key[e];
            rank += (ke > k) || (ke == k && e < d);
        }
        s_order[rank] = d;
    }
    __syncthreads();
    int gl[4], gm[4];
    for (int j = 0; j < 4; ++j) {
        const int g = lane + 64 * j;
        gl[j] = g < ng ? glabels[(int64_t)i * G + g] : 0;
        gm[j] = -1;
    }
    const float* row0 = iou + (int64_t)i * D * G;
    for (int r = 0; r < nd; ++r) {
        const int d = s_order[r], dl = s_dl[d];
        const float* row = row0 + (int64_t)d * G;
        u64 best = 0;                                             // a candidate's key is > 0: its IoU is >= t > 0
        for (int j = 0; j < 4; ++j) {
            const int g = lane + 64 * j;
            if (g < ng && gm[j] < 0 && (!class_aware || gl[j] == dl)) {
                const float v = row[g];
                if (v >= t) {
                    const u64 key = ((u64)__float_as_uint(v) << 32) | (unsigned)(kMaxSlots - 1 - g);
                    best = key > best ? key : best;
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const u64 other = __shfl_xor(best, o);
            best = other > best ? other : best;
        }
        if (best) {
            const int g = kMaxSlots - 1 - (int)(best & 0xffffffffu);
            if ((g & 63) == lane) {
                for (int j = 0; j < 4; ++j)
                    if (j == (g >> 6)) gm[j] = d;
                s_dm[d] = g;
            }
        }
    }
    __syncthreads();
    int* dm = det_match + ((int64_t)i * T + ti) * D;
    int* gmo = gt_match + ((int64_t)i * T + ti) * G;
    for (int d = lane; d < D; d += 64) dm[d] = s_dm[d];
    for (int j = 0; j < 4; ++j) {
        const int g = lane + 64 * j;
        if (g < G) gmo[g] = gm[j];
    }
}

bool aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

void check_slots(const char* who, int n, int D, int G) {
    RFI_REQUIRE(n >= 1 && n <= 65535, std::string(who) + ": needs 1 <= n <= 65535 images");
    RFI_REQUIRE(D >= 1 && D <= kMaxSlots, std::string(who) + ": needs 1 <= D <= 256 detections per image");
    RFI_REQUIRE(G >= 1 && G <= kMaxSlots, std::string(who) + ": needs 1 <= G <= 256 ground truths per image");
}

void check_plane(const char* who, int h, int w) {
    RFI_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= (int64_t(1) << 24), std::string(who) + ": needs H, W >= 1 and H W <= 2^24");
}

}  // namespace

void launch_pack_masks(rfi_ctx* ctx, const uint8_t* masks, int64_t m, int h, int w, uint64_t* bits, int* area, int* extent) {
    check_plane("pack_masks", h, w);
    RFI_REQUIRE(m >= 1 && m <= 0x7fffffff, "pack_masks: needs 1 <= m <= 2^31 - 1 planes");
    RFI_REQUIRE(aligned(bits, 8) && aligned(area, 4) && aligned(extent, 4), "pack_masks: bits must be 8-byte, area and extent 4-byte aligned");
    const int wc = (w + 63) / 64;
    ProfScope ps(ctx, FAM_METRICS, 0, (double)m * h * (w + 8.0 * wc));
    hipLaunchKernelGGL(pack_masks_kernel, dim3((unsigned)m), dim3(kPackBlock), 0, ctx->stream, masks, h, w, wc, reinterpret_cast<u64*>(bits), area,
                       extent);
    check_launch("pack_masks");
}

void launch_mask_iou(rfi_ctx* ctx, const uint64_t* det_bits, const int* det_area, const int* det_extent, const int* det_count,
                     const int* det_base, int64_t det_planes, const uint64_t* gt_bits, const int* gt_area, const int* gt_extent,
                     const int* gt_count, const int* gt_base, int64_t gt_planes, int n, int D, int G, int h, int w, int* inter, float* iou) {
    check_slots("mask_iou", n, D, G);
    check_plane("mask_iou", h, w);
    RFI_REQUIRE(det_planes >= 0 && gt_planes >= 0 && det_planes <= 0x7fffffff && gt_planes <= 0x7fffffff,
                "mask_iou: needs 0 <= planes <= 2^31 - 1 on both sides");
    RFI_REQUIRE(aligned(det_bits, 8) && aligned(gt_bits, 8), "mask_iou: bits must be 8-byte aligned");
    RFI_REQUIRE(aligned(det_area, 4) && aligned(det_extent, 4) && aligned(det_count, 4) && aligned(det_base, 4) && aligned(gt_area, 4) &&
                    aligned(gt_extent, 4) && aligned(gt_count, 4) && aligned(gt_base, 4) && aligned(inter, 4) && aligned(iou, 4),
                "mask_iou: int32 and float32 arrays must be 4-byte aligned");
    const int wc = (w + 63) / 64;
    const Side det{reinterpret_cast<const u64*>(det_bits), det_area, det_extent, det_count, det_base, det_planes};
    const Side gt{reinterpret_cast<const u64*>(gt_bits), gt_area, gt_extent, gt_count, gt_base, gt_planes};
    ProfScope ps(ctx, FAM_METRICS);
    hipLaunchKernelGGL(mask_iou_kernel, dim3(D, n), dim3(kBlock), 0, ctx->stream, det, gt, D, G, h, wc, inter, iou);
    check_launch("mask_iou");
}

void launch_box_iou(rfi_ctx* ctx, const float* det_boxes, const int* det_count, const float* gt_boxes, const int* gt_count, int n, int D,
                    int G, float* iou) {
    check_slots("box_iou", n, D, G);
    RFI_REQUIRE(aligned(det_boxes, 4) && aligned(det_count, 4) && aligned(gt_boxes, 4) && aligned(gt_count, 4) && aligned(iou, 4),
                "box_iou: int32 and float32 arrays must be 4-byte aligned");
    const int64_t total = (int64_t)n * D * G;
    ProfScope ps(ctx, FAM_METRICS);
    hipLaunchKernelGGL(box_iou_kernel, dim3(grid_of(cdiv(total, kBlock), "box_iou")), dim3(kBlock), 0, ctx->stream, det_boxes, det_count,
                       gt_boxes, gt_count, D, G, total, iou);
    check_launch("box_iou");
}

void launch_match_instances(rfi_ctx* ctx, const float* iou, const float* scores, const int* det_labels, const int* det_count,
                            const int* gt_labels, const int* gt_count, int n, int D, int G, const float* thresholds, int T, int class_aware,
                            int* det_match, int* gt_match) {
    check_slots("match_instances", n, D, G);
    RFI_REQUIRE(T >= 1 && T <= kMaxThresholds, "match_instances: needs 1 <= T <= 32 thresholds");
    Thresholds thr{};
    for (int k = 0; k < T; ++k) {
        RFI_REQUIRE(std::isfinite(thresholds[k]) && thresholds[k] > 0.0f && thresholds[k] <= 1.0f,
                    "match_instances: thresholds must be finite and in (0, 1]");
        thr.t[k] = thresholds[k];
    }
    RFI_REQUIRE(aligned(iou, 4) && aligned(scores, 4) && aligned(det_labels, 4) && aligned(det_count, 4) && aligned(gt_labels, 4) &&
                    aligned(gt_count, 4) && aligned(det_match, 4) && aligned(gt_match, 4),
                "match_instances: int32 and float32 arrays must be 4-byte aligned");
    ProfScope ps(ctx, FAM_METRICS);
    hipLaunchKernelGGL(match_instances_kernel, dim3(T, n), dim3(64), 0, ctx->stream, iou, scores, det_labels, det_count, gt_labels, gt_count, D,
                       G, T, thr, class_aware != 0, det_match, gt_match);
    check_launch("match_instances");
}

}  // namespace rfi
