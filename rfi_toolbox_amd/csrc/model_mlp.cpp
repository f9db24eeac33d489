// The box head of Faster / Mask R-CNN (BASELINE.json configs[3]) as a stack of fully
// connected layers on the matrix cores.  NOT in the reference (no detector there) and torchvision is absent:
// builder-defined as the published head (Girshick 2015 / Lin et al. 2017: two FC layers of 1024 units + ReLU on the
// flattened 7 x 7 x 256 RoI features, then the class scores and the per-class box deltas; torchvision's TwoMLPHead +
// FastRCNNPredictor), oracle/mask_head_ref.py.
//
//   x [R, D]  ->  fc6 (D -> H) + ReLU  ->  fc7 (H -> H) + ReLU  ->  head (H -> 5 (K + 1)):  K + 1 class logits, then
//                                                                    (K + 1) x 4 box deltas (cls_score and bbox_pred stacked)
//
// A fully connected layer is a 1x1 conv over the R "pixels"; they are laid out as one [R / 32] x 32 image so that the
// conv kernels' 32-pixel-wide tiles are full.  The loss (cross-entropy + smooth L1 of the ground-truth class's deltas)
// needs per-RoI targets and lives outside the model (rfi_op_fastrcnn_loss -> rfi_model_backward_dlogits), as for the RPN.
#include <algorithm>

#include "model.hpp"

using namespace rfi;

void BoxHeadModel::build() {
    RFI_REQUIRE(in_ch > 0 && in_ch % 4 == 0 && feat > 0 && feat % 4 == 0 && out_ch > 0 && depth >= 1 && depth <= 8,
                "BoxHead: in_features and hidden width must be positive multiples of 4, 1..8 layers");
    const int L = depth;
    for (int i = 0; i < L; ++i) {
        ConvBN c;
        c.conv_name = "fc" + std::to_string(6 + i);
        c.has_bn = false;
        c.R = 1;
        c.cin = c.cin_p = i == 0 ? in_ch : feat;
        c.cout = feat;
        add_conv(c);
    }
    add_head("head", feat);
    alloc_state();
    fcY.assign(L, -1); fcG.assign(L, -1);
    for (int i = 0; i < L; ++i) make_bufs({&fcY[i], &fcG[i]});
    make_bufs({&gx});
}

namespace {
// R rows as an image: [R / 32] x 32 when possible (full 32-wide tiles), else R x 1 x 1
Shape layout_of(int rows) { return rows % 32 == 0 ? Shape{1, rows / 32, 32} : Shape{rows, 1, 1}; }
}  // namespace

void BoxHeadModel::prepare_shape(int n, int h, int w) {
    RFI_REQUIRE(h == 1 && w == 1, "BoxHead: the input is [R, in_features] (n = R, h = w = 1)");
    const size_t M = (size_t)n;
    for (int i = 0; i < depth; ++i) { bufs[fcY[i]].ensure(ctx, M * feat); bufs[fcG[i]].ensure(ctx, M * feat); }
    bufs[gx].ensure(ctx, M * in_ch);
    // (prepare() adds the loss partials of a dense head, which this one never uses: 8208 floats, under the head's
    // 2048 (feat + 1) out_ch at any width)
    need_red(head_bwd_ws_floats((int64_t)M, feat, out_ch));
    need_red(channel_sum_ws_floats((int64_t)M, feat));
    for (auto& c : convs) need_slab(wgrad_same(View{nullptr, c.cin}, InXform{}, nullptr, layout_of(n), 1, 0, c.cin, c.cout, nullptr));
}

void BoxHeadModel::forward_pass(const float* x_dev, int n, int, int, bool) {
    const int L = depth;
    const Shape s = layout_of(n);
    for (int i = 0; i < L; ++i) {
        ConvBN& c = convs[i];
        ConvArgs a = conv_same(i == 0 ? View{x_dev, in_ch} : View{buf(fcY[i - 1]), feat}, i == 0 ? InXform{} : act_of(convs[i - 1]), s,
                               1, 0, c.cin, c.cout, params + c.w_off, c.w3, params + c.b_off, buf(fcY[i]));
        launch_conv(ctx, a);
    }
    const ConvBN& cl = convs[L - 1];
    launch_head_fwd(ctx, buf(fcY[L - 1]), n, feat, cl.scale(), cl.shift(), params + head_w_off, params + head_b_off, out_ch, buf(logits));
}

// dlogits are the caller's (rfi_model_backward_dlogits): this head has no loss of its own
void BoxHeadModel::backward_pass(const float* x_dev, const uint8_t*, int n, int, int) {
    RFI_REQUIRE(ext_dlogits, "BoxHead: the loss lives outside the model (rfi_op_fastrcnn_loss + rfi_model_backward_dlogits)");
    side_bound = 0;
    const int L = depth;
    const Shape s = layout_of(n);
    const int64_t M = n;
    const ConvBN& cl = convs[L - 1];
    launch_head_bwd(ctx, buf(fcY[L - 1]), M, feat, cl.scale(), cl.shift(), params + head_w_off, out_ch, buf(dlogits), buf(fcG[L - 1]),
                    buf(ws_red), grads + head_w_off, grads + head_b_off);
    for (int i = L - 1; i >= 0; --i) {
        ConvBN& c = convs[i];
        float* dA = buf(fcG[i]);
        launch_relu_bwd(ctx, dA, buf(fcY[i]), M * c.cout);
        launch_channel_sum(ctx, View{dA, c.cout}, M, c.cout, buf(ws_red), grads + c.b_off);
        // side stream: every layer owns its gradient tensor fcG[i], nothing the weight gradient reads is rewritten in this pass
        wgrad_on_side(wgrad_same(i == 0 ? View{x_dev, in_ch} : View{buf(fcY[i - 1]), feat}, i == 0 ? InXform{} : act_of(convs[i - 1]),
                                 dA, s, 1, 0, c.cin, c.cout, grads + c.w_off), nullptr);
        ConvArgs a = conv_same(View{dA, c.cout}, InXform{}, s, 1, 0, c.cout, c.cin, c.wd, c.wd3, nullptr,
                               i == 0 ? buf(gx) : buf(fcG[i - 1]));
        launch_conv(ctx, a);
    }
    side_join_lazy();                 // (the caller goes on with the input gradient; the weight gradients are needed at the optimiser step)
    bucket_ready(0, n_flat);
}

void BoxHeadModel::algorithmic_flops(int n, int, int, double& fwd, double& step) const {
    double f = 0;
    for (auto& c : convs) f += 2.0 * n * c.cin * c.cout;
    f += 2.0 * n * (double)feat * out_ch;
    fwd = f;
    step = 3.0 * f;
}

// y.<i> / dy.<i>: raw output of FC layer i and, after a backward pass, its gradient dY_i; dx: the input gradient
void BoxHeadModel::debug_tensor(const std::string& name, const std::string& base, int idx, bool, CallScope&, const float*& src, size_t& n) {
    RFI_REQUIRE(name.find(':') == std::string::npos, "debug_tensor: the heads' tensors are float32: no padding lanes");
    if (base == "y" || base == "dy") {
        RFI_REQUIRE(idx >= 0 && idx < depth, "debug_tensor: layer index out of range");
        src = buf(base == "y" ? fcY[idx] : fcG[idx]);
        n = (size_t)pN * feat;
    } else if (name == "dx") {
        src = buf(gx);
        n = (size_t)pN * in_ch;
    } else {
        throw Error("debug_tensor: unknown tensor " + name);
    }
}
