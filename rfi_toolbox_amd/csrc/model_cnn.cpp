// The "3-layer CNN segmenter" (BASELINE.json configs[0]/[1]) on the same HIP
// kernels as the U-Net:  Conv3x3(in->C)+bias -> ReLU -> Conv3x3(C->C)+bias -> ReLU -> Conv1x1(C->out).
// Not a reference class (nearest text: README.md:379-398); trained with the reference's step
// (scripts/train_model.py:120-151) through the shared loss / clip / Adam code in model.cpp.
//
// Only the raw conv outputs Y1, Y2 are kept in HBM; ReLU is applied by the consumer's loads
// (InXform with scale 1, shift 0) exactly as the U-Net's BN+ReLU is, so the forward pass is three
// launches and writes 2*M*C + M floats.
#include <algorithm>

#include "model.hpp"

using namespace rfi;

void Cnn3Model::build() {
    RFI_REQUIRE(in_ch > 0 && out_ch > 0 && feat > 0, "SimpleCNN: channel counts must be positive");
    RFI_REQUIRE(feat % 4 == 0, "SimpleCNN: width must be a multiple of 4 (16-byte NHWC pixels)");
    const char* names[2] = {"encoder.0", "encoder.2"};
    for (int i = 0; i < 2; ++i) {
        ConvBN c;
        c.conv_name = names[i];
        c.has_bn = false;
        c.cin = i == 0 ? in_ch : feat;
        c.cin_p = i == 0 ? (int)align4((size_t)in_ch) : feat;
        c.cout = feat;
        add_conv(c);
    }
    add_head("decoder.0", feat);
    alloc_state();
    make_bufs({&cY1, &cY2, &cG1, &cG2});
}

void Cnn3Model::prepare_shape(int n, int h, int w) {
    const size_t M1 = (size_t)n * h * w;
    for (int i : {cY1, cY2, cG1, cG2}) bufs[i].ensure(ctx, M1 * feat);
    need_red(head_bwd_ws_floats((int64_t)M1, feat, out_ch));
    need_red(channel_sum_ws_floats((int64_t)M1, feat));
    for (auto& c : convs) need_slab(wgrad_same(View{nullptr, c.cin_p}, InXform{}, nullptr, Shape{n, h, w}, 3, 1, c.cin_p, c.cout, nullptr));
}

void Cnn3Model::forward_pass(const float* x_dev, int n, int h, int w, bool) {
    ConvBN& c1 = convs[0];
    ConvBN& c2 = convs[1];
    const Shape s{n, h, w};
    View x = network_input(x_dev, n, h, w);
    ConvArgs a1 = conv_same(x, InXform{}, s, 3, 1, c1.cin_p, c1.cout, params + c1.w_off, c1.w3, params + c1.b_off, buf(cY1));
    a1.algo_flops = 2.0 * n * h * w * 9.0 * c1.cin * c1.cout;
    launch_conv(ctx, a1);
    ConvArgs a2 = conv_same(View{buf(cY1), c1.cout}, act_of(c1), s, 3, 1, c2.cin_p, c2.cout, params + c2.w_off, c2.w3,
                            params + c2.b_off, buf(cY2));
    a2.algo_flops = 2.0 * n * h * w * 9.0 * c2.cin * c2.cout;
    launch_conv(ctx, a2);
    launch_head_fwd(ctx, buf(cY2), (int64_t)n * h * w, feat, c2.scale(), c2.shift(), params + head_w_off,
                    params + head_b_off, out_ch, buf(logits));
}

void Cnn3Model::backward_pass(const float* x_dev, const uint8_t* labels_dev, int n, int h, int w) {
    ConvBN& c1 = convs[0];
    ConvBN& c2 = convs[1];
    const int64_t M = (int64_t)n * h * w;
    const Shape s{n, h, w};
    if (loss_kind == 1) launch_focal_bwd(ctx, buf(logits), labels_dev, M, focal_alpha, focal_gamma, buf(dlogits));
    else launch_loss_bwd(ctx, buf(logits), labels_dev, M, d_sums, buf(dlogits));
    // head: dW, db and the gradient w.r.t. relu(Y2)
    launch_head_bwd(ctx, buf(cY2), M, feat, c2.scale(), c2.shift(), params + head_w_off, out_ch, buf(dlogits),
                    buf(cG2), buf(ws_red), grads + head_w_off, grads + head_b_off);
    auto conv_backward = [&](ConvBN& c, float* dA, const float* Y, View in, InXform in_xf, float* dx) {
        launch_relu_bwd(ctx, dA, Y, M * c.cout);                       // dA -> dY
        launch_channel_sum(ctx, View{dA, c.cout}, M, c.cout, buf(ws_red), grads + c.b_off);
        WgradArgs wa = wgrad_same(in, in_xf, dA, s, 3, 1, c.cin_p, c.cout, grads + c.w_off);
        wa.algo_flops = 2.0 * M * 9.0 * c.cin * c.cout;
        wgrad_on_side(wa, nullptr);                // wgrad on the side stream, next to the dgrad / ReLU chain
        if (dx) {
            ConvArgs a = conv_same(View{dA, c.cout}, InXform{}, s, 3, 1, c.cout, c.cin, c.wd, c.wd3, nullptr, dx);
            a.algo_flops = 2.0 * n * h * w * 9.0 * c.cin * c.cout;
            launch_conv(ctx, a);
        }
    };
    conv_backward(c2, buf(cG2), buf(cY2), View{buf(cY1), c1.cout}, act_of(c1), buf(cG1));
    conv_backward(c1, buf(cG1), buf(cY1), padded_input(x_dev), InXform{}, nullptr);
    side_join();
    bucket_ready(0, n_flat);                  // three layers: one bucket
}

// two 3x3 convs at full resolution + the 1x1 head
void Cnn3Model::algorithmic_flops(int n, int h, int w, double& fwd, double& step) const {
    const double M = (double)n * h * w;
    const double stem = 2.0 * M * 9.0 * convs[0].cin * convs[0].cout;
    fwd = stem + 2.0 * M * 9.0 * convs[1].cin * convs[1].cout + 2.0 * M * (double)feat * out_ch;
    step = 3.0 * fwd - stem;
}
