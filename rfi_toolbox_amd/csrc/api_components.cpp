// extern "C" surface of librfi_hip.so, continued: connected components (declared in include/rfi_hip.h; kernels in
// components.hip).
#include "kernels.hpp"

using namespace rfi;

extern "C" {

int rfi_components_limits(int32_t* tile_h, int32_t* tile_w, int32_t* scan_block) {
    return guarded([&] {
        RFI_REQUIRE(tile_h && tile_w && scan_block, "components_limits: null argument");
        int th, tw, sb;
        components_limits(&th, &tw, &sb);
        *tile_h = th;
        *tile_w = tw;
        *scan_block = sb;
    });
}
size_t rfi_components_ws_bytes(int n, int h, int w) {
    if (n < 1 || h < 1 || w < 1 || (int64_t)h * w > (int64_t(1) << 30)) return 0;
    return components_ws_bytes(n, h, w);
}
int rfi_op_label_components(rfi_ctx* ctx, const void* masks, int dtype, int n, int h, int w, int connectivity, void* workspace,
                            int32_t* labels, int32_t* n_components) {
    return guarded([&] {
        RFI_REQUIRE(ctx && masks && workspace && labels && n_components, "label_components: null argument");
        ctx->activate();
        launch_label_components(ctx, masks, dtype, n, h, w, connectivity, workspace, labels, n_components);
    });
}
int rfi_op_component_table(rfi_ctx* ctx, const int32_t* labels, int n, int h, int w, const int32_t* comp_base, int64_t total,
                           int32_t* area, int32_t* box) {
    return guarded([&] {
        RFI_REQUIRE(ctx && labels && comp_base && area && box, "component_table: null argument");
        ctx->activate();
        launch_component_table(ctx, labels, n, h, w, comp_base, total, area, box);
    });
}
int rfi_op_components_keep(rfi_ctx* ctx, const int32_t* labels, int n, int h, int w, const int32_t* comp_base, const int32_t* area,
                           int min_area, uint8_t* out) {
    return guarded([&] {
        RFI_REQUIRE(ctx && labels && comp_base && area && out, "components_keep: null argument");
        ctx->activate();
        launch_components_keep(ctx, labels, n, h, w, comp_base, area, min_area, out);
    });
}
int rfi_op_instances_select(rfi_ctx* ctx, const int32_t* n_components, const int32_t* comp_base, const int32_t* area, const int32_t* box,
                            int n, int min_area, int min_side, int max_instances, float* boxes, int32_t* labels, int32_t* count,
                            int32_t* n_survivors, int32_t* base, int32_t* component) {
    return guarded([&] {
        RFI_REQUIRE(ctx && n_components && comp_base && area && box && boxes && labels && count && n_survivors && base && component,
                    "instances_select: null argument");
        ctx->activate();
        launch_instances_select(ctx, n_components, comp_base, area, box, n, min_area, min_side, max_instances, boxes, labels, count,
                                n_survivors, base, component);
    });
}
int rfi_op_instance_masks(rfi_ctx* ctx, const int32_t* labels, int n, int h, int w, const int32_t* component, const int32_t* count,
                          const int32_t* base, int max_instances, uint8_t* masks) {
    return guarded([&] {
        RFI_REQUIRE(ctx && labels && component && count && base && masks, "instance_masks: null argument");
        ctx->activate();
        launch_instance_masks(ctx, labels, n, h, w, component, count, base, max_instances, masks);
    });
}
int rfi_op_copy_rows(rfi_ctx* ctx, const void* src, size_t src_pitch, void* dst, size_t dst_pitch, size_t width_bytes, size_t rows) {
    return guarded([&] {
        RFI_REQUIRE(ctx && src && dst, "copy_rows: null argument");
        RFI_REQUIRE(width_bytes <= src_pitch && width_bytes <= dst_pitch, "copy_rows: a row is wider than its pitch");
        if (!width_bytes || !rows) return;
        ctx->activate();
        RFI_CHECK_HIP(hipMemcpy2DAsync(dst, dst_pitch, src, src_pitch, width_bytes, rows, hipMemcpyDeviceToDevice, ctx->stream));
    });
}

}  // extern "C"
