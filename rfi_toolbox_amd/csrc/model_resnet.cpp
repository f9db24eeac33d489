// U-Net with a ResNet-18-style encoder (BASELINE.json configs[2]).  NOT in the reference (it
// ships plain U-Nets only, models/unet.py) and neither torchvision nor segmentation_models_pytorch exist in this
// image: builder-defined, oracle/resnet_unet_ref.py, parity unpinned by the reference.
//
//   stem      Conv3x3(in -> f, bias=False) + BN + ReLU                                  at H
//   layer l   BasicBlock(c_{l-1} -> c_l, stride s_l) + BasicBlock(c_l -> c_l),  c_l = f 2^(l-1), s_1 = 1, s_l = 2
//             BasicBlock: conv3x3(s) + BN + ReLU + conv3x3 + BN, + shortcut (identity, or Conv1x1(s=2) + BN), ReLU
//   then      the reference's own bottleneck (MaxPool2 + DoubleConv), decoders and 1x1 head (models/unet.py:30-77)
//             fed by the four stage outputs as skip connections (model.cpp).
// The ResNet-18 topology (four stages of two BasicBlocks, widths f..8f, stride-2 3x3 + projection shortcuts between
// stages) with a full-resolution stem instead of 7x7/2 + max-pool, as ResNets for small images use: the decoder of
// this path wants a full-resolution skip, and RFI patches are 128 x 128.
//
// Stride-2 3x3 convolutions run as 2x2 / stride-1 convolutions on the space-to-depth input, the projection as a 1x1
// convolution on a channel slice of it (resnet_kernels.hip).  The ReLU after the residual add is applied by ONE
// elementwise kernel that materialises the block output (the next block needs it as its identity shortcut anyway);
// its backward masks by the stored output and hands the same dz to both BatchNorm branches.
#include <algorithm>

#include "model.hpp"

using namespace rfi;

void UNetModel::build_resnet() {
    RFI_REQUIRE(in_ch > 0 && out_ch > 0 && feat > 0 && feat % 4 == 0, "UNetResNet18: init_features must be a positive multiple of 4");
    depth = 4;
    const int D = depth;
    blocks.clear();
    auto add = [&](const std::string& cname, const std::string& bname, int cin, int cout, int R, int stride, int lvl, bool bias) {
        ConvBN c;
        c.conv_name = cname;
        c.bn_name = bname;
        c.cin = cin;
        c.cin_p = convs.empty() ? (int)align4((size_t)cin) : cin;
        c.cout = cout;
        c.R = R; c.stride = stride; c.level = lvl; c.has_bias = bias;
        return add_conv(c);
    };
    add("stem.0", "stem.1", in_ch, feat, 3, 1, 1, false);
    int cin = feat;
    for (int l = 1; l <= D; ++l) {
        const int cout = feat << (l - 1);
        for (int b = 0; b < 2; ++b) {
            ResBlock rb;
            const std::string p = "layer" + std::to_string(l) + "." + std::to_string(b);
            rb.stride = (b == 0 && l > 1) ? 2 : 1;
            rb.cin = cin; rb.cout = cout; rb.level = l;
            rb.c1 = add(p + ".conv1", p + ".bn1", cin, cout, 3, rb.stride, l, false);
            rb.c2 = add(p + ".conv2", p + ".bn2", cout, cout, 3, 1, l, false);
            if (rb.stride == 2) rb.cd = add(p + ".downsample.0", p + ".downsample.1", cin, cout, 1, 2, l, false);
            blocks.push_back(rb);
            cin = cout;
        }
    }
    i_bott = (int)convs.size();
    add("bottleneck.conv.0", "bottleneck.conv.1", cin, cin * 2, 3, 1, D + 1, true);
    add("bottleneck.conv.3", "bottleneck.conv.4", cin * 2, cin * 2, 3, 1, D + 1, true);
    cin *= 2;
    for (int l = D; l >= 1; --l) {
        const int cout = feat << (l - 1);
        add_up("decoder" + std::to_string(l) + ".up", cin, cout);
        const std::string p = "decoder" + std::to_string(l) + ".conv.conv";
        add(p + ".0", p + ".1", cin, cout, 3, 1, l, true);
        add(p + ".3", p + ".4", cout, cout, 3, 1, l, true);
        cin = cout;
    }
    add_head("final_conv", feat);
    alloc_state();
    make_slots();
    make_bufs({&rs_stemY, &rs_a0, &rs_g0, &rs_g1, &rs_dX, &rs_dS, &rs_dW, &rs_dzd, &rs_dz[0], &rs_dz[1], &rs_dA1[0], &rs_dA1[1]});
    for (auto& b : blocks) {
        make_bufs({&b.Y1, &b.Y2, &b.A});
        if (b.stride == 2) make_bufs({&b.Yd, &b.xs});
    }

    // derived filters of the stride-2 convs (2x2 form + its dgrad layout) and identity scale / shift vectors
    size_t wneed = 0;
    for (auto& c : convs)
        if (c.stride == 2 && c.R == 3)
            wneed += 2 * align4((size_t)16 * c.cin * c.cout) + align4(weights_x3_floats(4, c.cout, 4 * c.cin)) + align4(weights_x3_floats(4, 4 * c.cin, c.cout));
    const size_t cmax = (size_t)feat << D;
    rs_wpool = static_cast<float*>(ctx->alloc((wneed + 2 * cmax + 16) * sizeof(float)));
    size_t o = 0;
    for (auto& c : convs)
        if (c.stride == 2 && c.R == 3) {
            c.ws2d = rs_wpool + o; o += align4((size_t)16 * c.cin * c.cout);
            c.wds2d = rs_wpool + o; o += align4((size_t)16 * c.cin * c.cout);
            c.ws2d3 = rs_wpool + o; o += align4(weights_x3_floats(4, c.cout, 4 * c.cin));
            c.wds2d3 = rs_wpool + o; o += align4(weights_x3_floats(4, 4 * c.cin, c.cout));
        }
    rs_ones = rs_wpool + o; o += cmax;
    rs_zeros = rs_wpool + o;
    {
        std::vector<float> h(2 * cmax, 0.0f);
        for (size_t i = 0; i < cmax; ++i) h[i] = 1.0f;
        RFI_CHECK_HIP(hipMemcpyAsync(rs_ones, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        RFI_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    }
}

void UNetModel::prepare_resnet(int n, int h, int w) {
    const size_t M1 = (size_t)n * h * w;
    bufs[rs_stemY].ensure(ctx, M1 * feat);
    bufs[rs_a0].ensure(ctx, M1 * feat);
    size_t gmax = M1 * feat, wmax = 0;
    for (auto& b : blocks) {
        const size_t M = (size_t)n * (h >> (b.level - 1)) * (w >> (b.level - 1));
        for (int i : {b.Y1, b.Y2, b.A}) bufs[i].ensure(ctx, M * b.cout);
        if (b.stride == 2) {
            bufs[b.Yd].ensure(ctx, M * b.cout);
            bufs[b.xs].ensure(ctx, M * 4 * b.cin);
            wmax = std::max(wmax, (size_t)16 * b.cin * b.cout);
        }
        gmax = std::max(gmax, std::max(M * b.cout, M * 4 * b.cin));
    }
    for (int i : {rs_g0, rs_g1, rs_dz[0], rs_dz[1], rs_dA1[0], rs_dA1[1], rs_dX, rs_dS, rs_dzd}) bufs[i].ensure(ctx, gmax);
    bufs[rs_dW].ensure(ctx, wmax + 16);
}

// the 2x2 forms of the stride-2 filters (forward and input-gradient layouts); every other derived copy comes from
// the batched relayout of model.cpp
void UNetModel::refresh_resnet_weights() {
    for (int ci = 0; ci < i_bott; ++ci)
        if (convs[ci].stride == 2 && convs[ci].R == 3) refresh_s2d_forms(convs[ci]);
}

// -> the pooled output of layer 4 (input of the bottleneck); skip l is written into concat[l][..., C:2C]
View UNetModel::forward_resnet_encoder(View x, int n, int h, int w, bool train) {
    const int D = depth;
    {                                             // stem: a0 = relu(BN(conv3x3(x)))
        ConvBN& c = convs[0];
        Shape s{n, h, w};
        conv_bn(c, x, InXform{}, s, params + c.w_off, c.w3, 3, 1, c.cin_p, buf(rs_stemY), train, 2.0 * n * h * w * 9.0 * c.cin * c.cout);
        launch_bn_add_relu(ctx, buf(rs_stemY), c.scale(), c.shift(), nullptr, nullptr, nullptr, (int64_t)n * h * w, c.cout,
                           MutView{buf(rs_a0), c.cout}, MutView{});
    }
    const float* a_in = buf(rs_a0);
    for (size_t bi = 0; bi < blocks.size(); ++bi) {
        ResBlock& b = blocks[bi];
        ConvBN& c1 = convs[b.c1];
        ConvBN& c2 = convs[b.c2];
        Shape s{n, h >> (b.level - 1), w >> (b.level - 1)};
        const int64_t M = (int64_t)s.N * s.H * s.W;
        const double f1 = 2.0 * M * 9.0 * b.cin * b.cout, f2 = 2.0 * M * 9.0 * b.cout * b.cout;
        if (b.stride == 2) {
            launch_s2d(ctx, a_in, n, s.H * 2, s.W * 2, b.cin, buf(b.xs));
            conv_bn(c1, View{buf(b.xs), 4 * b.cin}, InXform{}, s, c1.ws2d, c1.ws2d3, 2, 1, 4 * b.cin, buf(b.Y1), train, f1);
            ConvBN& cd = convs[b.cd];             // projection: 1x1 on the (0, 0) slice of the space-to-depth input
            conv_bn(cd, View{buf(b.xs), 4 * b.cin}, InXform{}, s, params + cd.w_off, cd.w3, 1, 0, b.cin, buf(b.Yd), train,
                    2.0 * M * b.cin * b.cout);
        } else {
            conv_bn(c1, View{a_in, b.cin}, InXform{}, s, params + c1.w_off, c1.w3, 3, 1, b.cin, buf(b.Y1), train, f1);
        }
        conv_bn(c2, View{buf(b.Y1), b.cout}, bn_xf(c1), s, params + c2.w_off, c2.w3, 3, 1, b.cout, buf(b.Y2), train, f2);
        // a_out = relu(BN2(Y2) + shortcut); the stage output also goes into the decoder's concat buffer (the skip)
        const bool last = (bi & 1) == 1;
        MutView skip = last ? MutView{buf(concat[b.level]) + b.cout, 2 * b.cout} : MutView{};
        if (b.stride == 2) {
            ConvBN& cd = convs[b.cd];
            launch_bn_add_relu(ctx, buf(b.Y2), c2.scale(), c2.shift(), buf(b.Yd), cd.scale(), cd.shift(), M, b.cout,
                               MutView{buf(b.A), b.cout}, skip);
        } else {
            launch_bn_add_relu(ctx, buf(b.Y2), c2.scale(), c2.shift(), a_in, nullptr, nullptr, M, b.cout,
                               MutView{buf(b.A), b.cout}, skip);
        }
        a_in = buf(b.A);
    }
    // MaxPool2d(2) of the last stage (identity "BatchNorm": scale 1, shift 0; the values are already >= 0)
    const ResBlock& lb = blocks.back();
    Shape s{n, h >> (D - 1), w >> (D - 1)};
    launch_bn_relu_pool(ctx, buf(lb.A), s.N, s.H, s.W, lb.cout, rs_ones, rs_zeros,
                        MutView{buf(concat[D]) + lb.cout, 2 * lb.cout}, buf(pool[D]), 0.0f);
    return View{buf(pool[D]), lb.cout};
}

void UNetModel::backward_resnet_encoder(const float* x_dev, int n, int h, int w) {
    const int D = depth;
    // dW of a conv (R x R stride 1 `pad`) into `dw` ([taps][cy][cx]) on the side stream
    auto wgrad = [&](View x, InXform xf_x, const float* dY, int cy, int cx, Shape s, int R, int pad, float* dw, double flops) {
        WgradArgs wa = wgrad_same(x, xf_x, dY, s, R, pad, cx, cy, dw);
        wa.algo_flops = flops;
        wgrad_on_side(wa, nullptr);
    };
    // dX = conv(dY, dgrad-layout filters): R x R stride 1 `pad` (pad of the GRADIENT conv)
    auto dgrad = [&](const float* dY, int cy, const float* wd, const float* wd3, int cx, Shape s, int R, int pad, float* dx,
                     double flops) {
        ConvArgs a = conv_same(View{dY, cy}, InXform{}, s, R, pad, cy, cx, wd, wd3, nullptr, dx);
        a.algo_flops = flops;
        launch_conv(ctx, a);
    };
    // gradient w.r.t. the last stage's output: skip gradient + max-pool routing of dpool
    float* gout = buf(rs_g0);
    float* gother = buf(rs_g1);
    {
        const ResBlock& lb = blocks.back();
        Shape s{n, h >> (D - 1), w >> (D - 1)};
        launch_pool_bwd_merge(ctx, buf(lb.A), s.N, s.H, s.W, lb.cout, rs_ones, rs_zeros,
                              View{buf(dconcat[D]) + lb.cout, 2 * lb.cout}, buf(dpool[D]), gout, 0.0f);
    }
    for (int bi = (int)blocks.size() - 1; bi >= 0; --bi) {
        ResBlock& b = blocks[bi];
        ConvBN& c1 = convs[b.c1];
        ConvBN& c2 = convs[b.c2];
        Shape s{n, h >> (b.level - 1), w >> (b.level - 1)};
        const int64_t M = (int64_t)s.N * s.H * s.W;
        const double f1 = 2.0 * M * 9.0 * b.cin * b.cout, f2 = 2.0 * M * 9.0 * b.cout * b.cout;
        float* ws = buf(ws_red);
        const float* a_in = bi == 0 ? buf(rs_a0) : buf(blocks[bi - 1].A);
        // gout = gradient w.r.t. this block's output.  dz = gout * (a_out > 0) enters BOTH BatchNorm branches
        float* dz = buf(rs_dz[bi & 1]);
        launch_relu_mask(ctx, View{gout, b.cout}, View{}, View{buf(b.A), b.cout}, View{}, M, b.cout, dz);
        // ---- main branch: BN2 (no activation of its own: slope 1 = identity), conv2, BN1 + ReLU, conv1
        launch_bn_bwd_reduce(ctx, dz, buf(b.Y2), M, b.cout, c2.scale(), c2.shift(), c2.mean(), c2.invstd(), ws, c2.c1(), c2.c2(),
                             grads + c2.g_off, grads + c2.be_off, 1.0f);
        launch_bn_bwd_apply(ctx, dz, buf(b.Y2), M, b.cout, c2.scale(), c2.shift(), c2.mean(), c2.invstd(), params + c2.g_off,
                            c2.c1(), c2.c2(), ws, nullptr, 1.0f);                 // dz <- dY2
        wgrad(View{buf(b.Y1), b.cout}, bn_xf(c1), dz, b.cout, b.cout, s, 3, 1, grads + c2.w_off, f2);
        float* dA1 = buf(rs_dA1[bi & 1]);
        dgrad(dz, b.cout, c2.wd, c2.wd3, b.cout, s, 3, 1, dA1, f2);
        launch_bn_bwd_reduce(ctx, dA1, buf(b.Y1), M, b.cout, c1.scale(), c1.shift(), c1.mean(), c1.invstd(), ws, c1.c1(), c1.c2(),
                             grads + c1.g_off, grads + c1.be_off, act_slope);
        launch_bn_bwd_apply(ctx, dA1, buf(b.Y1), M, b.cout, c1.scale(), c1.shift(), c1.mean(), c1.invstd(), params + c1.g_off,
                            c1.c1(), c1.c2(), ws, nullptr, act_slope);            // dA1 <- dY1
        float* dX = buf(rs_dX);
        if (b.stride == 2) {
            // conv1 in its 2x2 form on the space-to-depth input: weight gradient in that layout, then back to 3x3
            wgrad(View{buf(b.xs), 4 * b.cin}, InXform{}, dA1, b.cout, 4 * b.cin, s, 2, 1, buf(rs_dW), f1);
            {
                SideScope side(this);             // (after the slab reduction of that wgrad, same stream)
                launch_w_s2d(ctx, grads + c1.w_off, b.cout, b.cin, buf(rs_dW), false);
                side.end();
            }
            dgrad(dA1, b.cout, c1.wds2d, c1.wds2d3, 4 * b.cin, s, 2, 0, dX, f1);             // [M][4 cin]
            // ---- projection branch: BNd on the same dz (recomputed: the first copy now holds dY2), 1x1 conv
            ConvBN& cd = convs[b.cd];
            dz = buf(rs_dzd);
            launch_relu_mask(ctx, View{gout, b.cout}, View{}, View{buf(b.A), b.cout}, View{}, M, b.cout, dz);
            launch_bn_bwd_reduce(ctx, dz, buf(b.Yd), M, b.cout, cd.scale(), cd.shift(), cd.mean(), cd.invstd(), ws, cd.c1(), cd.c2(),
                                 grads + cd.g_off, grads + cd.be_off, 1.0f);
            launch_bn_bwd_apply(ctx, dz, buf(b.Yd), M, b.cout, cd.scale(), cd.shift(), cd.mean(), cd.invstd(), params + cd.g_off,
                                cd.c1(), cd.c2(), ws, nullptr, 1.0f);             // dz <- dYd
            wgrad(View{buf(b.xs), 4 * b.cin}, InXform{}, dz, b.cout, b.cin, s, 1, 0, grads + cd.w_off, 2.0 * M * b.cin * b.cout);
            float* dS = buf(rs_dS);
            dgrad(dz, b.cout, cd.wd, cd.wd3, b.cin, s, 1, 0, dS, 2.0 * M * b.cin * b.cout);   // [M][cin]
            // back to full resolution, + the skip gradient of the previous stage (its output is this block's input)
            launch_d2s_add(ctx, dX, dS, View{buf(dconcat[b.level - 1]) + b.cin, 2 * b.cin}, n, s.H * 2, s.W * 2, b.cin, gother);
        } else {
            wgrad(View{a_in, b.cin}, InXform{}, dA1, b.cout, b.cin, s, 3, 1, grads + c1.w_off, f1);
            dgrad(dA1, b.cout, c1.wd, c1.wd3, b.cin, s, 3, 1, dX, f1);
            // identity shortcut: gin = dX + gout * (a_out > 0)
            launch_relu_mask(ctx, View{gout, b.cout}, View{}, View{buf(b.A), b.cout}, View{dX, b.cin}, M, b.cout, gother);
        }
        std::swap(gout, gother);
        bucket_ready(c1.w_off, (size_t)(bi + 1 < (int)blocks.size() ? convs[blocks[bi + 1].c1].w_off : convs[i_bott].w_off));
    }
    {                                             // stem: gout = gradient w.r.t. a0 = relu(BN(stemY))
        ConvBN& c = convs[0];
        Shape s{n, h, w};
        const int64_t M = (int64_t)n * h * w;
        float* ws = buf(ws_red);
        launch_bn_bwd_reduce(ctx, gout, buf(rs_stemY), M, c.cout, c.scale(), c.shift(), c.mean(), c.invstd(), ws, c.c1(), c.c2(),
                             grads + c.g_off, grads + c.be_off, act_slope);
        launch_bn_bwd_apply(ctx, gout, buf(rs_stemY), M, c.cout, c.scale(), c.shift(), c.mean(), c.invstd(), params + c.g_off,
                            c.c1(), c.c2(), ws, nullptr, act_slope);
        wgrad(padded_input(x_dev), InXform{}, gout, c.cout, c.cin_p, s, 3, 1, grads + c.w_off, 2.0 * M * 9.0 * c.cin * c.cout);
        bucket_ready(0, convs[blocks[0].c1].w_off);
    }
}
