// The per-RoI mask branch of Mask R-CNN (BASELINE.json configs[3] / north_star "per-pixel mask head"; SURVEY.md 8a row
// A11) on the same HIP kernels as the segmentation models.  NOT in the reference (it contains no detector) and
// torchvision is absent: builder-defined as the published head (He et al. 2017, fig. 4 right):
//
//   x [R, 14, 14, C]  RoIAlign-ed features (rfi_op_roi_align)
//   mask_fcn1..L      Conv3x3(C -> C, pad 1) + bias -> ReLU            (L = 4)
//   conv5_mask        ConvTranspose2d(C -> C, k 2, s 2) + bias -> ReLU
//   mask_fcn_logits   Conv1x1(C -> K)                                  logits [R, 28, 28, K]
//   loss              mean binary cross-entropy with logits over every RoI pixel (K = 1: one foreground class, RFI)
//
// oracle/mask_head_ref.py holds the same layers as plain torch.nn modules (parity unpinned by the reference).  Only the
// raw conv outputs are kept; ReLU is applied by the consumers' loads, as in model_cnn.cpp.  rfi_model_input_grad returns
// the gradient w.r.t. x, which rfi_op_roi_align_backward / rfi_op_roi_align_ml_backward gather back into the feature map.
//
// Without `upsample` it is the RPN head (Ren et al. 2015), is the same stack without the transposed conv: Conv3x3(C -> C) + ReLU, then ONE
// 1x1 conv with 5 A outputs per pixel = A objectness logits followed by A x 4 box deltas (cls_logits and bbox_pred of the
// usual implementation stacked; models/rpn_head.py splits them at the state_dict boundary).  Its loss needs per-anchor
// targets, so it lives outside the model: rfi_op_rpn_loss produces d(loss)/d(head output) and
// rfi_model_backward_dlogits runs the backward pass from there.
#include <algorithm>

#include "model.hpp"

using namespace rfi;

void ConvHeadModel::build() {
    RFI_REQUIRE(in_ch > 0 && in_ch % 4 == 0, "MaskHead: in_channels must be a positive multiple of 4 (16-byte NHWC pixels)");
    RFI_REQUIRE(out_ch > 0 && depth >= 1 && depth <= 8, "MaskHead: out_channels > 0, 1..8 conv layers");
    const bool up = upsample;
    feat = in_ch;
    out_scale = up ? 2 : 1;
    loss_kind = 1;                // sigmoid focal loss with gamma = 0 and no alpha = plain mean BCE-with-logits
    focal_alpha = -1.0f;
    focal_gamma = 0.0f;
    const int L = depth, C = in_ch;
    for (int i = 0; i < L; ++i) {
        ConvBN c;
        c.conv_name = up ? "mask_fcn" + std::to_string(i + 1) : "conv." + std::to_string(i) + ".0";
        c.has_bn = false;
        c.cin = c.cin_p = c.cout = C;
        add_conv(c);
    }
    if (up) add_up("conv5_mask", C, C);
    add_head(up ? "mask_fcn_logits" : "head", C);
    alloc_state();
    mkY.assign(L, -1); mkG.assign(L, -1);
    for (int i = 0; i < L; ++i) make_bufs({&mkY[i], &mkG[i]});
    make_bufs({&mkU, &mkGU, &gx, &head_wd, &head_w3, &head_wd3});
}

void ConvHeadModel::prepare_shape(int n, int h, int w) {
    const int L = depth, C = in_ch;
    const size_t M = (size_t)n * h * w, M4 = (size_t)out_scale * out_scale * M;
    for (int i = 0; i < L; ++i) { bufs[mkY[i]].ensure(ctx, M * C); bufs[mkG[i]].ensure(ctx, M * C); }
    bufs[mkU].ensure(ctx, upsample ? M4 * C : 16);
    bufs[mkGU].ensure(ctx, upsample ? M4 * C : 16);
    bufs[gx].ensure(ctx, M * C);
    need_red(head_bwd_ws_floats((int64_t)M4, C, out_ch));
    need_red(channel_sum_ws_floats((int64_t)M4, C));
    const Shape s{n, h, w};
    need_slab(wgrad_same(View{nullptr, C}, InXform{}, nullptr, s, 3, 1, C, C, nullptr));          // the 3x3 layers
    // the transposed conv (sized without `upsample` too, as ever: ws_slab keeps its size)
    UpConv up; up.cin = up.cout = C;
    need_slab(convt_wgrad_args(upsample ? ups[0] : up, View{nullptr, C}, View{nullptr, C}, InXform{}, s));
    if (head_on_mfma())                                   // the 1x1 head's weight gradient
        need_slab(wgrad_same(View{nullptr, C}, InXform{}, nullptr, Shape{n, out_scale * h, out_scale * w}, 1, 0, C, out_ch, nullptr));
    bufs[head_wd].ensure(ctx, (size_t)out_ch * C + 16);
    bufs[head_w3].ensure(ctx, weights_x3_floats(1, out_ch, C) + 16);
    bufs[head_wd3].ensure(ctx, weights_x3_floats(1, C, out_ch) + 16);
}

void ConvHeadModel::forward_pass(const float* x_dev, int n, int h, int w, bool) {
    const int L = depth, C = in_ch;
    const int64_t M4 = (int64_t)out_scale * out_scale * n * h * w;
    for (int i = 0; i < L; ++i) {
        ConvBN& c = convs[i];
        ConvArgs a = conv_same(i == 0 ? View{x_dev, C} : View{buf(mkY[i - 1]), C}, i == 0 ? InXform{} : act_of(convs[i - 1]),
                               Shape{n, h, w}, 3, 1, C, C, params + c.w_off, c.w3, params + c.b_off, buf(mkY[i]));
        launch_conv(ctx, a);
    }
    if (upsample) {
        ConvArgs a = convt_args(ups[0], View{buf(mkY[L - 1]), C}, act_of(convs[L - 1]), Shape{n, h, w});
        a.y = MutView{buf(mkU), C};
        launch_conv(ctx, a);
    }
    const ConvBN& cl = convs[L - 1];                  // (its scale = 1 / shift = 0 vectors serve the ReLU of U as well)
    if (head_on_mfma()) {             // a wide 1x1 head (the RPN's 5 A outputs) is a GEMM: the conv kernels, not the per-pixel VALU kernel
        // the pre-split records of this small filter are rebuilt per pass (one 5-us launch, no allocation)
        if (use_w3()) launch_weights_to_x3(ctx, params + head_w_off, 1, out_ch, C, buf(head_w3));
        ConvArgs a = conv_same(View{head_in(), C}, act_of(cl), Shape{n, out_scale * h, out_scale * w}, 1, 0, C, out_ch,
                               params + head_w_off, buf(head_w3), params + head_b_off, buf(logits));
        launch_conv(ctx, a);
        return;
    }
    launch_head_fwd(ctx, head_in(), M4, C, cl.scale(), cl.shift(), params + head_w_off, params + head_b_off,
                    out_ch, buf(logits));
}

void ConvHeadModel::backward_pass(const float* x_dev, const uint8_t* labels_dev, int n, int h, int w) {
    const int L = depth, C = in_ch;
    const int64_t M = (int64_t)n * h * w, M4 = (int64_t)out_scale * out_scale * M;
    const Shape s{n, h, w}, s4{n, out_scale * h, out_scale * w};
    if (!ext_dlogits) {               // (rfi_model_backward_dlogits: the caller's loss kernel has filled dlogits)
        if (loss_kind == 1) launch_focal_bwd(ctx, buf(logits), labels_dev, M4 * out_ch, focal_alpha, focal_gamma, buf(dlogits));
        else launch_loss_bwd(ctx, buf(logits), labels_dev, M4 * out_ch, d_sums, buf(dlogits));
    }
    const ConvBN& cl = convs[L - 1];
    if (head_on_mfma()) {
        // da = dlogits . W (a 1x1 conv with the transposed filter), dW = dlogits^T . act (the 1x1 weight gradient), db = column sums
        launch_weight_to_dgrad(ctx, params + head_w_off, 1, out_ch, C, 0, buf(head_wd));
        if (use_w3()) launch_weights_to_x3(ctx, buf(head_wd), 1, C, out_ch, buf(head_wd3));
        ConvArgs a = conv_same(View{buf(dlogits), out_ch}, InXform{}, s4, 1, 0, out_ch, C, buf(head_wd), buf(head_wd3), nullptr,
                               head_din());
        launch_conv(ctx, a);
        launch_channel_sum(ctx, View{buf(dlogits), out_ch}, M4, out_ch, buf(ws_red), grads + head_b_off);
        wgrad_on_side(wgrad_same(View{head_in(), C}, act_of(cl), buf(dlogits), s4, 1, 0, C, out_ch, grads + head_w_off), nullptr);
    } else
    launch_head_bwd(ctx, head_in(), M4, C, cl.scale(), cl.shift(), params + head_w_off, out_ch, buf(dlogits), head_din(), buf(ws_red),
                    grads + head_w_off, grads + head_b_off);
    // transposed conv: dU = dUa * (U > 0); bias, weight and input gradients
    if (upsample) {
        const UpConv& u = ups[0];
        launch_relu_bwd(ctx, buf(mkGU), buf(mkU), M4 * C);
        launch_channel_sum(ctx, View{buf(mkGU), C}, M4, C, buf(ws_red), grads + u.b_off);
        convt_backward(u, View{buf(mkGU), C}, View{buf(mkY[L - 1]), C}, act_of(convs[L - 1]), s, buf(mkG[L - 1]));
    }
    for (int i = L - 1; i >= 0; --i) {
        ConvBN& c = convs[i];
        float* dA = buf(mkG[i]);
        launch_relu_bwd(ctx, dA, buf(mkY[i]), M * C);                       // dA -> dY
        launch_channel_sum(ctx, View{dA, C}, M, C, buf(ws_red), grads + c.b_off);
        wgrad_on_side(wgrad_same(i == 0 ? View{x_dev, C} : View{buf(mkY[i - 1]), C}, i == 0 ? InXform{} : act_of(convs[i - 1]), dA, s,
                                 3, 1, C, C, grads + c.w_off), nullptr);
        ConvArgs a = conv_same(View{dA, C}, InXform{}, s, 3, 1, C, C, c.wd, c.wd3, nullptr, i == 0 ? buf(gx) : buf(mkG[i - 1]));
        launch_conv(ctx, a);
    }
    side_join_lazy();                 // (a head inside the detector's step: the caller goes on with the input gradient)
    bucket_ready(0, n_flat);
}

// L 3x3 convs, (the transposed conv,) the 1x1 head
void ConvHeadModel::algorithmic_flops(int n, int h, int w, double& fwd, double& step) const {
    const double M = (double)n * h * w, C = in_ch, s2 = (double)out_scale * out_scale;
    fwd = depth * 2.0 * M * 9.0 * C * C + (upsample ? 2.0 * M * 4.0 * C * C : 0.0) + 2.0 * s2 * M * C * out_ch;
    step = 3.0 * fwd;                 // the input gradient is computed too (it feeds the RoIAlign adjoint)
}

// y.<i> / dy.<i>: raw output of 3x3 layer i and, after a backward pass, its gradient dY_i; u / du: the same of the transposed
// conv (the mask head only); dx: the input gradient.  Read-only views of the buffers the passes keep anyway
void ConvHeadModel::debug_tensor(const std::string& name, const std::string& base, int idx, bool, CallScope&, const float*& src, size_t& n) {
    const size_t M = (size_t)pN * pH * pW;
    RFI_REQUIRE(name.find(':') == std::string::npos, "debug_tensor: the heads' tensors are float32: no padding lanes");
    if (base == "y" || base == "dy") {
        RFI_REQUIRE(idx >= 0 && idx < depth, "debug_tensor: layer index out of range");
        src = buf(base == "y" ? mkY[idx] : mkG[idx]);
        n = M * in_ch;
    } else if (name == "u" || name == "du") {
        RFI_REQUIRE(upsample, "debug_tensor: only the mask head has the transposed conv");
        src = buf(name == "u" ? mkU : mkGU);
        n = (size_t)out_scale * out_scale * M * in_ch;
    } else if (name == "dx") {
        src = buf(gx);
        n = M * in_ch;
    } else {
        throw Error("debug_tensor: unknown tensor " + name);
    }
}
