// Mask R-CNN inference on the device (MaskRCNN.detect): what MaskRCNN.predict does in NumPy behind the box head and behind the
// mask head -- the per-class softmax / decode / threshold / sort in front of the detection NMS, the choice of the max_det best
// kept boxes of an image with the mask branch's RoI list, the RoI list of the proposals in front of the box head, and the
// paste of the 28 x 28 mask logits into the image plane with the union over an image's instances.  NOT in the reference (it
// has no detector): the rules are those of predict / _paste in models/mask_rcnn.py, restated in NumPy by
// tests/detect_infer_ref.py.
//
// Like detect_sample.hip: one workgroup per (image, class) set or per image, 64-bit keys (order-preserving image of the score
// in the high word, the position in the low word) sorted in LDS by a bitonic network, results written in a fixed order, every
// launch size known on the host -- no atomics on floats, nothing read back.  All arithmetic is float32.
#include "kernels.hpp"
#include "detect_sort.hpp"

namespace rfi {
namespace {

constexpr int kB = 256;

// level k of a box: 0 + [area >= t1] + [area >= t2] + [area >= t3], area = max(w h, 1e-6) in float32 (roi_compact's rule)
__device__ __forceinline__ int box_level(float4 b, float t1, float t2, float t3) {
    const float area = fmaxf((b.z - b.x) * (b.w - b.y), 1e-6f);
    return (area >= t1 ? 1 : 0) + (area >= t2 ? 1 : 0) + (area >= t3 ? 1 : 0);
}
__device__ __forceinline__ void write_roi(float* q, int image, float4 b) {
    q[0] = (float)image; q[1] = b.x; q[2] = b.y; q[3] = b.z; q[4] = b.w;
}

// ---------------------------------------------------------------- candidates of one (image, foreground class)
// head [B Pmax][5 K1]: row b Pmax + r belongs to proposal r of image b.  Thread r: softmax probability of class c, class c's
// deltas decoded against the proposal (box_decode_kernel's arithmetic) and clipped; the rows that pass both tests, sorted by
// descending probability (ties: ascending r), go to set b (K1 - 1) + c - 1
__global__ __launch_bounds__(kB) void detect_candidates_kernel(const float* __restrict__ head, const float* __restrict__ props,
                                                              const int* __restrict__ pcount, int Pmax, int K1, int npow2, float clip_h,
                                                              float clip_w, float score_thresh, float min_size, float* __restrict__ boxes,
                                                              float* __restrict__ scores, int* __restrict__ counts) {
    __shared__ u64 s_keys[kB];
    __shared__ float4 s_box[kB];
    __shared__ float s_prob[kB];
    const float kClamp = 4.135166556742356f;         // log(1000 / 16)
    const int set = blockIdx.x, b = set / (K1 - 1), c = 1 + set % (K1 - 1), r = threadIdx.x;
    const int cnt = min(max(pcount[b], 0), Pmax);
    u64 key = ~0ull;
    bool ok = false;
    if (r < cnt) {
        const float* hp = head + ((size_t)b * Pmax + r) * 5 * K1;
        float zmax = hp[0];
        for (int k = 1; k < K1; ++k) zmax = fmaxf(zmax, hp[k]);
        float sum = 0.0f;
        for (int k = 0; k < K1; ++k) sum += expf(hp[k] - zmax);
        const float prob = expf(hp[c] - zmax) / sum;
        const float4 a = *reinterpret_cast<const float4*>(props + ((size_t)b * Pmax + r) * 4);
        const float* dp = hp + K1 + 4 * c;            // (K1 need not be a multiple of 4: scalar loads)
        const float d0 = dp[0], d1 = dp[1], d2 = dp[2], d3 = dp[3];
        const float w = a.z - a.x, h = a.w - a.y, cx = a.x + 0.5f * w, cy = a.y + 0.5f * h;
        const float dw = fminf(d2, kClamp), dh = fminf(d3, kClamp);
        const float pcx = d0 * w + cx, pcy = d1 * h + cy, pw = expf(dw) * w, ph = expf(dh) * h;
        float4 box = make_float4(pcx - 0.5f * pw, pcy - 0.5f * ph, pcx + 0.5f * pw, pcy + 0.5f * ph);
        box.x = fminf(fmaxf(box.x, 0.0f), clip_w); box.z = fminf(fmaxf(box.z, 0.0f), clip_w);
        box.y = fminf(fmaxf(box.y, 0.0f), clip_h); box.w = fminf(fmaxf(box.w, 0.0f), clip_h);
        ok = prob > score_thresh && (box.z - box.x) >= min_size && (box.w - box.y) >= min_size;
        s_box[r] = box;
        s_prob[r] = prob;
        if (ok) key = ((u64)desc_key(prob) << 32) | (u64)r;
    }
    if (r < npow2) s_keys[r] = key;
    const int total = __syncthreads_count(ok ? 1 : 0);
    bitonic_sort(s_keys, npow2);
    if (r < Pmax) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        float sc = -INFINITY;
        if (r < total) {
            const int src = (int)(s_keys[r] & 0xffffffffull);
            v = s_box[src];
            sc = s_prob[src];
        }
        *reinterpret_cast<float4*>(boxes + ((size_t)set * Pmax + r) * 4) = v;
        scores[(size_t)set * Pmax + r] = sc;
    }
    if (r == 0) counts[set] = total;
}

// ---------------------------------------------------------------- detections of one image: the max_det best kept candidates
// over its classes (descending score, ties class-major, then by position in the class's sorted set)
struct DetOut {
    float* boxes;                      // [B][max_det][4], zeros behind count
    float* scores;                     // [B][max_det]
    int* labels;                       // [B][max_det]
    int* count;                        // [B]
    float* rois;                       // [B max_det][5] (image, x1, y1, x2, y2); padding rows: a zero box of their own image
    int* level;                        // [B max_det]
};
__global__ __launch_bounds__(kB) void detect_select_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                          const unsigned char* __restrict__ keep, int CK, int K, int npow2, int max_det,
                                                          float t1, float t2, float t3, DetOut o) {
    extern __shared__ u64 s_sel[];
    __shared__ int s_kept;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) s_kept = 0;
    __syncthreads();
    int mine = 0;
    for (int e = threadIdx.x; e < npow2; e += kB) {
        u64 key = ~0ull;
        if (e < CK && keep[(size_t)b * CK + e]) {
            key = ((u64)desc_key(scores[(size_t)b * CK + e]) << 32) | (u64)e;
            ++mine;
        }
        s_sel[e] = key;
    }
    if (mine) atomicAdd(&s_kept, mine);
    bitonic_sort(s_sel, npow2);
    const int nsel = min(s_kept, max_det);
    for (int r = threadIdx.x; r < max_det; r += kB) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        float sc = 0.0f;
        int lab = 0;
        if (r < nsel) {
            const int e = (int)(s_sel[r] & 0xffffffffull);
            v = *reinterpret_cast<const float4*>(boxes + ((size_t)b * CK + e) * 4);
            sc = scores[(size_t)b * CK + e];
            lab = 1 + e / K;
        }
        const size_t q = (size_t)b * max_det + r;
        *reinterpret_cast<float4*>(o.boxes + q * 4) = v;
        o.scores[q] = sc;
        o.labels[q] = lab;
        write_roi(o.rois + q * 5, b, v);
        o.level[q] = box_level(v, t1, t2, t3);
    }
    if (threadIdx.x == 0) o.count[b] = nsel;
}

// ---------------------------------------------------------------- proposals -> RoI rows at a fixed stride of Pmax per image
__global__ __launch_bounds__(kB) void rois_from_boxes_kernel(const float* __restrict__ props, const int* __restrict__ pcount, int B, int Pmax,
                                                            float t1, float t2, float t3, float* __restrict__ rois, int* __restrict__ level) {
    const int total = B * Pmax;
    for (int q = blockIdx.x * kB + threadIdx.x; q < total; q += gridDim.x * kB) {
        const int b = q / Pmax, r = q % Pmax;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < min(pcount[b], Pmax)) v = *reinterpret_cast<const float4*>(props + (size_t)q * 4);
        write_roi(rois + (size_t)q * 5, b, v);
        level[q] = box_level(v, t1, t2, t3);
    }
}

// ---------------------------------------------------------------- paste: M x M mask logits -> the image plane
// A thread owns 4 consecutive pixels of a row of one image and walks that image's boxes: per box one 32-bit store of the four
// instance-mask bytes (consecutive lanes: consecutive dwords), the union kept in a register and stored once.  The box table
// of the image sits in LDS.
constexpr int kM = 28;
constexpr int kPasteMax = 256;

__device__ __forceinline__ float sigmoidf(float z) { return 1.0f / (1.0f + expf(-z)); }

__global__ __launch_bounds__(kB) void mask_paste_kernel(const float* __restrict__ logits, const float* __restrict__ det_boxes,
                                                       const int* __restrict__ det_count, int max_det, int H, int W,
                                                       unsigned char* __restrict__ rfi_mask, unsigned char* __restrict__ masks) {
    __shared__ float4 s_box[kPasteMax];
    __shared__ int4 s_win[kPasteMax];
    const int b = blockIdx.y;
    const int cnt = min(max(det_count[b], 0), max_det);
    for (int j = threadIdx.x; j < cnt; j += kB) {
        const float4 v = *reinterpret_cast<const float4*>(det_boxes + ((size_t)b * max_det + j) * 4);
        s_box[j] = v;
        s_win[j] = make_int4(max((int)floorf(v.x), 0), max((int)floorf(v.y), 0), min((int)ceilf(v.z), W), min((int)ceilf(v.w), H));
    }
    __syncthreads();
    const int W4 = W >> 2;
    const int t = blockIdx.x * kB + threadIdx.x;
    if (t >= H * W4) return;
    const int py = t / W4, px0 = (t % W4) << 2;
    const size_t plane = (size_t)H * W, pix = (size_t)py * W + px0;
    unsigned uni = 0u;
    for (int j = 0; j < max_det; ++j) {
        unsigned word = 0u;
        if (j < cnt) {
            const int4 wn = s_win[j];
            if (py >= wn.y && py < wn.w && px0 + 3 >= wn.x && px0 < wn.z) {
                const float4 bx = s_box[j];
                const float* lg = logits + ((size_t)b * max_det + j) * (kM * kM);
                const float gy = ((float)py + 0.5f - bx.y) / fmaxf(bx.w - bx.y, 1e-6f) * (float)kM - 0.5f;
                const float fyf = floorf(gy);
                const int y0 = (int)fminf(fmaxf(fyf, 0.0f), (float)(kM - 1)), y1 = min(y0 + 1, kM - 1);
                const float fy = fminf(fmaxf(gy - (float)y0, 0.0f), 1.0f);
                const float iw = fmaxf(bx.z - bx.x, 1e-6f);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int px = px0 + k;
                    if (px < wn.x || px >= wn.z) continue;
                    const float gx = ((float)px + 0.5f - bx.x) / iw * (float)kM - 0.5f;
                    const float fxf = floorf(gx);
                    const int x0 = (int)fminf(fmaxf(fxf, 0.0f), (float)(kM - 1)), x1 = min(x0 + 1, kM - 1);
                    const float fx = fminf(fmaxf(gx - (float)x0, 0.0f), 1.0f);
                    const float p00 = sigmoidf(lg[y0 * kM + x0]), p01 = sigmoidf(lg[y0 * kM + x1]);
                    const float p10 = sigmoidf(lg[y1 * kM + x0]), p11 = sigmoidf(lg[y1 * kM + x1]);
                    const float v = (p00 * (1.0f - fx) + p01 * fx) * (1.0f - fy) + (p10 * (1.0f - fx) + p11 * fx) * fy;
                    if (v > 0.5f) word |= 1u << (8 * k);
                }
            }
        }
        uni |= word;
        if (masks) *reinterpret_cast<unsigned*>(masks + ((size_t)b * max_det + j) * plane + pix) = word;
    }
    *reinterpret_cast<unsigned*>(rfi_mask + (size_t)b * plane + pix) = uni;
}

}  // namespace

// ======================================================================================== launch wrappers
void launch_detect_candidates(rfi_ctx* ctx, const float* head, const float* props, const int* pcount, int B, int Pmax, int K1, float clip_h,
                              float clip_w, float score_thresh, float min_size, float* boxes, float* scores, int* counts) {
    RFI_REQUIRE(B > 0 && Pmax > 0 && Pmax <= kB && K1 >= 2, "detect_candidates: at most 256 proposals per image, background + one class");
    RFI_REQUIRE(!((reinterpret_cast<uintptr_t>(props) | reinterpret_cast<uintptr_t>(boxes)) & 15), "detect_candidates: 16-byte aligned boxes");
    ProfScope ps(ctx, FAM_ELEMWISE, 0, (double)B * Pmax * (20.0 * K1 + 16 + (K1 - 1) * 20.0), "detect_candidates");
    hipLaunchKernelGGL(detect_candidates_kernel, dim3((unsigned)(B * (K1 - 1))), dim3(kB), 0, ctx->stream, head, props, pcount, Pmax, K1,
                       pow2_at_least(Pmax), clip_h, clip_w, score_thresh, min_size, boxes, scores, counts);
    check_launch("detect_candidates");
}

void launch_detect_select(rfi_ctx* ctx, const float* boxes, const float* scores, const unsigned char* keep, int B, int classes, int K,
                          int max_det, float t1, float t2, float t3, float* det_boxes, float* det_scores, int* det_labels, int* det_count,
                          float* rois, int* level) {
    const int CK = classes * K, np2 = pow2_at_least(CK);
    RFI_REQUIRE(B > 0 && classes > 0 && K > 0 && np2 <= 8192 && max_det > 0, "detect_select: at most 8192 candidates per image");
    RFI_REQUIRE(!((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(det_boxes)) & 15), "detect_select: 16-byte aligned boxes");
    DetOut o{det_boxes, det_scores, det_labels, det_count, rois, level};
    ProfScope ps(ctx, FAM_ELEMWISE, 0, (double)B * (CK * 5.0 + max_det * 72.0), "detect_select");
    hipLaunchKernelGGL(detect_select_kernel, dim3(B), dim3(kB), (size_t)np2 * 8, ctx->stream, boxes, scores, keep, CK, K, np2, max_det, t1, t2,
                       t3, o);
    check_launch("detect_select");
}

void launch_rois_from_boxes(rfi_ctx* ctx, const float* props, const int* pcount, int B, int Pmax, float t1, float t2, float t3, float* rois,
                            int* level) {
    RFI_REQUIRE(B > 0 && Pmax > 0 && (int64_t)B * Pmax < (1ll << 30), "rois_from_boxes: empty input");
    RFI_REQUIRE(!(reinterpret_cast<uintptr_t>(props) & 15), "rois_from_boxes: 16-byte aligned boxes");
    ProfScope ps(ctx, FAM_ELEMWISE, 0, (double)B * Pmax * 40, "rois_from_boxes");
    hipLaunchKernelGGL(rois_from_boxes_kernel, dim3((unsigned)std::min<int64_t>(cdiv((int64_t)B * Pmax, kB), 1024)), dim3(kB), 0, ctx->stream,
                       props, pcount, B, Pmax, t1, t2, t3, rois, level);
    check_launch("rois_from_boxes");
}

void launch_mask_paste(rfi_ctx* ctx, const float* logits, const float* det_boxes, const int* det_count, int B, int max_det, int H, int W,
                       unsigned char* rfi_mask, unsigned char* masks) {
    RFI_REQUIRE(B > 0 && B <= 65535 && max_det > 0 && max_det <= kPasteMax && H > 0 && W > 0 && W % 4 == 0 && (int64_t)H * W < (1ll << 31),
                "mask_paste: at most 256 instances per image, W a multiple of 4");
    RFI_REQUIRE(!(reinterpret_cast<uintptr_t>(det_boxes) & 15) && !(reinterpret_cast<uintptr_t>(rfi_mask) & 3) &&
                !(reinterpret_cast<uintptr_t>(masks) & 3), "mask_paste: 16-byte aligned boxes, 4-byte aligned masks");
    const double px = (double)B * H * W;
    ProfScope ps(ctx, FAM_ELEMWISE, 0, px * (masks ? max_det + 1 : 1), "mask_paste");
    hipLaunchKernelGGL(mask_paste_kernel, dim3((unsigned)cdiv((int64_t)H * (W / 4), kB), B), dim3(kB), 0, ctx->stream, logits, det_boxes,
                       det_count, max_det, H, W, rfi_mask, masks);
    check_launch("mask_paste");
}

}  // namespace rfi
