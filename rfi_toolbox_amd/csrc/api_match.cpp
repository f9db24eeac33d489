// extern "C" surface of librfi_hip.so, continued: instance matching (declared in include/rfi_hip.h; kernels in
// instance_match.hip).
#include "kernels.hpp"

using namespace rfi;

extern "C" {

int rfi_op_pack_masks(rfi_ctx* ctx, const uint8_t* masks, int64_t m, int h, int w, uint64_t* bits, int32_t* area, int32_t* extent) {
    return guarded([&] {
        RFI_REQUIRE(ctx && masks && bits && area && extent, "pack_masks: null argument");
        ctx->activate();
        launch_pack_masks(ctx, masks, m, h, w, bits, area, extent);
    });
}
int rfi_op_mask_iou(rfi_ctx* ctx, const uint64_t* det_bits, const int32_t* det_area, const int32_t* det_extent, const int32_t* det_count,
                    const int32_t* det_base, int64_t det_planes, const uint64_t* gt_bits, const int32_t* gt_area, const int32_t* gt_extent,
                    const int32_t* gt_count, const int32_t* gt_base, int64_t gt_planes, int n, int d, int g, int h, int w, int32_t* inter,
                    float* iou) {
    return guarded([&] {
        RFI_REQUIRE(ctx && det_bits && det_area && det_extent && det_count && det_base && gt_bits && gt_area && gt_extent && gt_count &&
                        gt_base && inter && iou,
                    "mask_iou: null argument");
        ctx->activate();
        launch_mask_iou(ctx, det_bits, det_area, det_extent, det_count, det_base, det_planes, gt_bits, gt_area, gt_extent, gt_count, gt_base,
                        gt_planes, n, d, g, h, w, inter, iou);
    });
}
int rfi_op_box_iou(rfi_ctx* ctx, const float* det_boxes, const int32_t* det_count, const float* gt_boxes, const int32_t* gt_count, int n, int d,
                   int g, float* iou) {
    return guarded([&] {
        RFI_REQUIRE(ctx && det_boxes && det_count && gt_boxes && gt_count && iou, "box_iou: null argument");
        ctx->activate();
        launch_box_iou(ctx, det_boxes, det_count, gt_boxes, gt_count, n, d, g, iou);
    });
}
int rfi_op_match_instances(rfi_ctx* ctx, const float* iou, const float* scores, const int32_t* det_labels, const int32_t* det_count,
                           const int32_t* gt_labels, const int32_t* gt_count, int n, int d, int g, const float* thresholds, int t,
                           int class_aware, int32_t* det_match, int32_t* gt_match) {
    return guarded([&] {
        RFI_REQUIRE(ctx && iou && scores && det_labels && det_count && gt_labels && gt_count && thresholds && det_match && gt_match,
                    "match_instances: null argument");
        ctx->activate();
        launch_match_instances(ctx, iou, scores, det_labels, det_count, gt_labels, gt_count, n, d, g, thresholds, t, class_aware, det_match,
                               gt_match);
    });
}
int rfi_stitch_instances(rfi_ctx* ctx, const float* boxes, const float* scores, const int32_t* labels, const int32_t* counts,
                         const uint8_t* masks, int n_planes, int c, int t, const rfi_tiling* tiling, int d, int max_events, int min_area,
                         float min_score, int class_aware, int connectivity, float* out_boxes, float* out_scores, int32_t* out_labels,
                         int32_t* out_counts, uint8_t* rfi_mask, uint8_t* out_masks) {
    return guarded([&] {
        RFI_REQUIRE(ctx && boxes && scores && labels && counts && masks && tiling && out_boxes && out_scores && out_labels && out_counts &&
                        rfi_mask,
                    "stitch_instances: null argument");
        ctx->activate();
        launch_stitch_instances(ctx, boxes, scores, labels, counts, masks, n_planes, c, t, *tiling, d, max_events, min_area, min_score,
                                class_aware, connectivity, out_boxes, out_scores, out_labels, out_counts, rfi_mask, out_masks);
    });
}

}  // extern "C"
