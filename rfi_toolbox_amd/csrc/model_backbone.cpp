// ResNet-50-FPN backbone of the Mask R-CNN path (BASELINE.json configs[3]).  NOT in the
// reference (no detector there) and torchvision is absent: builder-defined as the published networks (He et al. 2016,
// ResNet-50 with the stride on the 3x3 conv of a Bottleneck; Lin et al. 2017, FPN) with the layer names and the frozen
// BatchNorm of the usual detection backbone; oracle/backbone_ref.py holds it as plain torch.nn modules.
//
//   body.conv1 7x7/2 (bias=False) + bn1 + ReLU -> MaxPool(3, 2, 1)                                  H/4, w channels
//   body.layer1..4: [3, 4, 6, 3] Bottlenecks (1x1 -> 3x3(stride) -> 1x1, x4 expansion, projection shortcut in the first
//                   block of a stage), strides 1, 2, 2, 2                                            C2..C5: 4w, 8w, 16w, 32w
//   fpn.inner_blocks.i 1x1 (+bias), top-down nearest-2x merge, fpn.layer_blocks.i 3x3 (+bias)         P2..P5: F channels
//   P6 = P5[:, ::2, ::2]                                                                             (LastLevelMaxPool)
//
// Every BatchNorm is FROZEN (per-channel affine from its buffers, as detection fine-tuning does): a conv's raw output is
// stored and the affine (+ ReLU) is applied by its consumers' loads, exactly like the train-mode BatchNorm of the U-Net
// but with constant coefficients, so the backward pass needs no statistics: dY = dA * scale * [z > 0].  Trainable: every
// conv weight and the FPN biases (flat parameter buffer; clip + Adam as everywhere).  The 7x7 stem (3 input channels)
// runs as a GEMM on its K-packed (im2col) input: K = 147 -> 160; on the direct VALU kernels it took 3.8 of 18.5 ms of
// the forward + backward pass at batch 64 x 128^2.  Stride-2 3x3 convs and projections use the space-to-depth forms of
// resnet_kernels.hip; everything else is the MFMA conv / split weight-gradient kernels.
#include <algorithm>

#include "model.hpp"

using namespace rfi;

namespace {
const int kBlocksPerStage[4] = {3, 4, 6, 3};
}

void BackboneModel::build() {
    RFI_REQUIRE(in_ch > 0 && feat > 0 && feat % 4 == 0 && out_ch > 0 && out_ch % 4 == 0,
                "ResNet50FPN: base width and FPN channels must be positive multiples of 4");
    depth = 4;
    const int w0 = feat, F = out_ch;
    bb.clear();
    auto add = [&](const std::string& cname, const std::string& bname, int cin, int cout, int R, int stride, int lvl, bool bn,
                   bool bias) {
        ConvBN c;
        c.conv_name = cname;
        c.bn_name = bname;
        c.cin = c.cin_p = cin;
        c.cout = cout;
        c.R = R; c.stride = stride; c.level = lvl;
        c.has_bn = bn; c.frozen_bn = true; c.has_bias = bias;
        return add_conv(c);
    };
    add("body.conv1", "body.bn1", in_ch, w0, 7, 2, 1, true, false);          // level = log2 of the OUTPUT stride
    int cin = w0;
    for (int s = 0; s < 4; ++s) {
        const int width = w0 << s, cout = 4 * width;
        for (int b = 0; b < kBlocksPerStage[s]; ++b) {
            BBlock k;
            const std::string p = "body.layer" + std::to_string(s + 1) + "." + std::to_string(b);
            k.stage = s;
            k.stride = (b == 0 && s > 0) ? 2 : 1;
            k.cin = cin; k.width = width; k.cout = cout;
            k.lvl_in = k.stride == 2 ? s + 1 : s + 2;      // resolution H >> lvl: layer1 at 2, layer2 at 3, ...
            k.lvl = s + 2;
            k.c1 = add(p + ".conv1", p + ".bn1", cin, width, 1, 1, k.lvl_in, true, false);
            k.c2 = add(p + ".conv2", p + ".bn2", width, width, 3, k.stride, k.lvl, true, false);
            k.c3 = add(p + ".conv3", p + ".bn3", width, cout, 1, 1, k.lvl, true, false);
            if (b == 0) k.cd = add(p + ".downsample.0", p + ".downsample.1", cin, cout, 1, k.stride, k.lvl, true, false);
            bb.push_back(k);
            cin = cout;
        }
    }
    for (int i = 0; i < 4; ++i)
        fpn_inner[i] = add("fpn.inner_blocks." + std::to_string(i) + ".0", "", 4 * (w0 << i), F, 1, 1, i + 2, false, true);
    for (int i = 0; i < 4; ++i)
        fpn_layer[i] = add("fpn.layer_blocks." + std::to_string(i) + ".0", "", F, F, 3, 1, i + 2, false, true);
    head_w_off = head_b_off = n_flat;     // (no head)
    alloc_state();
    make_bufs({&bY0, &bP0, &bArg, &fP6, &fdP6, &bdW, &bS, &bCol, &bWp});
    for (auto& k : bb) {
        make_bufs({&k.Y1, &k.Y2, &k.Y3, &k.A});
        if (k.cd >= 0) make_bufs({&k.Yd});
        if (k.stride == 2) make_bufs({&k.xs1, &k.xsA});
    }
    for (int i = 0; i < 4; ++i) make_bufs({&fL[i], &fM[i], &fP[i], &fdM[i], &fdP[i], &bT[i][0], &bT[i][1], &bT[i][2]});
    for (int& g : bG) make_bufs({&g});

    // 2x2 forms of the stride-2 3x3 filters, 4x tiled affine coefficients of their inputs, identity vectors
    const size_t cmax = (size_t)32 * w0;
    size_t need = 2 * cmax + 16;
    // (+ the 3 x bf16 records of those forms and of the K-packed stem filters: a launch without them splits a temporary copy and
    // drains the stream to free it -- eight stalls per step, 0.2 to several ms each in the rocprofv3 timeline of the detector)
    for (auto& k : bb)
        if (k.stride == 2)
            need += 2 * align4((size_t)16 * k.width * k.width) + 2 * align4((size_t)4 * k.width) +
                    align4(weights_x3_floats(4, k.width, 4 * k.width)) + align4(weights_x3_floats(4, 4 * k.width, k.width));
    need += align4(weights_x3_floats(1, w0, stem_kp())) + 16;
    rs_wpool = static_cast<float*>(ctx->alloc(need * sizeof(float)));
    size_t o = 0;
    rs_ones = rs_wpool + o; o += cmax;
    rs_zeros = rs_wpool + o; o += cmax;
    for (auto& k : bb)
        if (k.stride == 2) {
            ConvBN& c = convs[k.c2];
            c.ws2d = rs_wpool + o; o += align4((size_t)16 * k.width * k.width);
            c.wds2d = rs_wpool + o; o += align4((size_t)16 * k.width * k.width);
            k.sc4 = rs_wpool + o; o += align4((size_t)4 * k.width);
            k.sh4 = rs_wpool + o; o += align4((size_t)4 * k.width);
            c.ws2d3 = rs_wpool + o; o += align4(weights_x3_floats(4, k.width, 4 * k.width));
            c.wds2d3 = rs_wpool + o; o += align4(weights_x3_floats(4, 4 * k.width, k.width));
        }
    bb_stem_w3 = rs_wpool + o; o += align4(weights_x3_floats(1, w0, stem_kp()));
    {
        std::vector<float> h(2 * cmax, 0.0f);
        for (size_t i = 0; i < cmax; ++i) h[i] = 1.0f;
        RFI_CHECK_HIP(hipMemcpyAsync(rs_ones, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        RFI_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    }
    for (auto& c : convs)             // frozen gamma = 1, beta = 0 until loaded (slots 2 and 3 of the per-channel state)
        if (c.has_bn) {
            std::vector<float> g((size_t)2 * c.cout, 0.0f);
            for (int i = 0; i < c.cout; ++i) g[i] = 1.0f;
            RFI_CHECK_HIP(hipMemcpyAsync(c.frozen_weight(), g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
            RFI_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        }
}

namespace {
// a 1x1 conv does not see the image structure: on small maps (W < 32) run it on the same pixels laid out as one
// [M / 32] x 32 image, so that the 32-pixel-wide tiles of the kernels are full instead of mostly padding
Shape flat_1x1(Shape s, int R) {
    const int64_t M = (int64_t)s.N * s.H * s.W;
    return R == 1 && s.W < 32 && M % 32 == 0 ? Shape{1, (int)(M / 32), 32} : s;
}
}  // namespace

void BackboneModel::prepare_shape(int n, int h, int w) {
    RFI_REQUIRE(h % 64 == 0 && w % 64 == 0, "ResNet50FPN: H and W must be multiples of 64");
    const int F = out_ch;
    auto px = [&](int lvl) { return (size_t)n * (h >> lvl) * (w >> lvl); };
    bufs[bY0].ensure(ctx, px(1) * feat);
    bufs[bP0].ensure(ctx, px(2) * feat);
    bufs[bArg].ensure(ctx, px(2) * feat / 4 + 4);
    size_t gmax = px(1) * feat, wmax = 16;
    for (auto& k : bb) {
        bufs[k.Y1].ensure(ctx, px(k.lvl_in) * k.width);
        bufs[k.Y2].ensure(ctx, px(k.lvl) * k.width);
        bufs[k.Y3].ensure(ctx, px(k.lvl) * k.cout);
        bufs[k.A].ensure(ctx, px(k.lvl) * k.cout);
        if (k.cd >= 0) bufs[k.Yd].ensure(ctx, px(k.lvl) * k.cout);
        if (k.stride == 2) {
            bufs[k.xs1].ensure(ctx, px(k.lvl) * 4 * k.width);
            bufs[k.xsA].ensure(ctx, px(k.lvl) * 4 * k.cin);
            wmax = std::max(wmax, (size_t)16 * k.width * k.width);
        }
        gmax = std::max({gmax, px(k.lvl_in) * k.width, px(k.lvl_in) * k.cin, px(k.lvl) * k.cout, px(k.lvl) * 4 * k.width});
    }
    for (int i = 0; i < 4; ++i) {
        const size_t m = px(i + 2) * F;
        for (int b : {fL[i], fM[i], fP[i], fdM[i], fdP[i]}) bufs[b].ensure(ctx, m);
        gmax = std::max(gmax, m);
    }
    bufs[fP6].ensure(ctx, px(6) * F);
    bufs[fdP6].ensure(ctx, px(6) * F);
    for (int i = 0; i < 6; ++i) bufs[bG[i]].ensure(ctx, gmax);
    for (int r = 0; r < 4; ++r) for (int p = 0; p < 3; ++p) bufs[bT[r][p]].ensure(ctx, gmax);
    bufs[bS].ensure(ctx, gmax);
    bufs[bCol].ensure(ctx, px(1) * stem_kp());
    bufs[bWp].ensure(ctx, (size_t)feat * stem_kp() + 16);
    bufs[bdW].ensure(ctx, wmax + 16);
    const int cmax = 32 * feat;
    need_red(bn_bwd_ws_floats((int64_t)px(1), cmax));
    need_red(channel_sum_ws_floats((int64_t)px(2), std::max(cmax, F)));
    for (auto& c : convs) {
        // in the form backward_pass launches it: a stride-2 3x3 conv as 2x2 on its space-to-depth input (of which a stride-2
        // 1x1 projection reads a channel slice), the stem K-packed as a 1x1 conv
        int R = c.R, pad = c.R / 2, cx = c.cin;
        if (c.R == 3 && c.stride == 2) { R = 2; pad = 1; cx = 4 * c.cin; }
        if (c.R == 7) { R = 1; pad = 0; cx = stem_kp(); }
        const View x{nullptr, c.R == 1 && c.stride == 2 ? 4 * c.cin : cx};
        const Shape s{n, h >> c.level, w >> c.level};
        for (const Shape& l : {s, flat_1x1(s, R)})      // (a small 1x1 map in both layouts, as ever: ws_slab keeps its size)
            need_slab(wgrad_same(x, InXform{}, nullptr, l, R, pad, cx, c.cout, nullptr));
    }
}

// frozen BatchNorm coefficients and the derived filter copies the batched relayout does not cover (both directions at
// once: this model never splits its rebuild)
void BackboneModel::refresh_model_weights(Half) {
    if (stale & FROZEN) {
        for (auto& c : convs)
            if (c.has_bn) launch_bn_eval_coeffs(ctx, c.cout, c.frozen_weight(), c.frozen_bias(), c.running_mean(), c.running_var(), c.scale(), c.shift());
        for (auto& k : bb)
            if (k.stride == 2) {                  // the 2x2 conv reads the space-to-depth of conv1's RAW output: coefficients x 4
                const ConvBN& c1 = convs[k.c1];
                for (int r = 0; r < 4; ++r) {
                    RFI_CHECK_HIP(hipMemcpyAsync(k.sc4 + r * k.width, c1.scale(), k.width * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
                    RFI_CHECK_HIP(hipMemcpyAsync(k.sh4 + r * k.width, c1.shift(), k.width * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
                }
            }
        stale &= ~FROZEN;
    }
    for (auto& k : bb)
        if (k.stride == 2) refresh_s2d_forms(convs[k.c2]);
}

namespace {

// every conv of the backbone is stride 1 on its own output grid s (stride 2: the 2x2 form on the space-to-depth input)
void conv(rfi_model* m, View in, InXform xf, Shape s, const float* w, const float* w3, const float* bias, int cin, int cout, int R,
          int pad, float* Y) {
    ConvArgs a = m->conv_same(in, xf, flat_1x1(s, R), R, pad, cin, cout, w, w3, bias, Y);
    launch_conv(m->ctx, a);
}
// (the caller decides the stream: backward_backbone puts the weight gradients on the side stream)
WgradArgs wgrad(const rfi_model* m, View x, InXform xf_x, const float* dY, int cy, int cx, Shape s, int R, int pad, float* dw) {
    return m->wgrad_same(x, xf_x, dY, flat_1x1(s, R), R, pad, cx, cy, dw);
}
// dA (gradient w.r.t. act(Y * scale + shift), or w.r.t. the affine output when slope = 1) -> dY in place: dA * scale * act'
void affine_bwd(BackboneModel* m, const ConvBN& c, float* dA, const float* Y, int64_t M, float slope) {
    launch_bn_bwd_apply(m->ctx, dA, Y, M, c.cout, c.scale(), c.shift(), m->rs_zeros, m->rs_ones, c.scale(), m->rs_zeros, m->rs_zeros,
                        m->buf(m->ws_red), nullptr, slope);
}

}  // namespace

void BackboneModel::forward_pass(const float* x_dev, int n, int h, int w, bool) {
    {   // stem: 7x7 / 2 as a GEMM on its K-packed input (K = 49 C padded to a multiple of 16), then max-pool of the activated output
        ConvBN& c = convs[0];
        const int Kp = stem_kp();
        launch_im2col(ctx, x_dev, n, h, w, in_ch, 7, 2, 3, h / 2, w / 2, Kp, buf(bCol));
        launch_w_pack(ctx, params + c.w_off, 49, c.cout, in_ch, Kp, buf(bWp), true);
        if (use_w3()) launch_weights_to_x3(ctx, buf(bWp), 1, c.cout, Kp, bb_stem_w3);
        conv(this, View{buf(bCol), Kp}, InXform{}, Shape{n, h / 2, w / 2}, buf(bWp), bb_stem_w3, nullptr, Kp, c.cout, 1, 0, buf(bY0));
        launch_maxpool3_fwd(ctx, buf(bY0), n, h / 2, w / 2, c.cout, c.scale(), c.shift(), buf(bP0), reinterpret_cast<unsigned*>(buf(bArg)));
    }
    const float* a_in = buf(bP0);
    for (auto& k : bb) {
        ConvBN &c1 = convs[k.c1], &c2 = convs[k.c2], &c3 = convs[k.c3];
        const Shape si{n, h >> k.lvl_in, w >> k.lvl_in}, so{n, h >> k.lvl, w >> k.lvl};
        conv(this, View{a_in, k.cin}, InXform{}, si, params + c1.w_off, c1.w3, nullptr, k.cin, k.width, 1, 0, buf(k.Y1));
        if (k.stride == 2) {
            launch_s2d(ctx, buf(k.Y1), n, si.H, si.W, k.width, buf(k.xs1));
            conv(this, View{buf(k.xs1), 4 * k.width}, InXform{k.sc4, k.sh4, 1, 0.0f}, so, c2.ws2d, c2.ws2d3, nullptr, 4 * k.width,
                 k.width, 2, 1, buf(k.Y2));
        } else {
            conv(this, View{buf(k.Y1), k.width}, act_of(c1), so, params + c2.w_off, c2.w3, nullptr, k.width, k.width, 3, 1, buf(k.Y2));
        }
        conv(this, View{buf(k.Y2), k.width}, act_of(c2), so, params + c3.w_off, c3.w3, nullptr, k.width, k.cout, 1, 0, buf(k.Y3));
        const int64_t M = (int64_t)so.N * so.H * so.W;
        if (k.cd >= 0) {
            ConvBN& cd = convs[k.cd];
            if (k.stride == 2) {
                launch_s2d(ctx, a_in, n, si.H, si.W, k.cin, buf(k.xsA));
                conv(this, View{buf(k.xsA), 4 * k.cin}, InXform{}, so, params + cd.w_off, cd.w3, nullptr, k.cin, k.cout, 1, 0, buf(k.Yd));
            } else {
                conv(this, View{a_in, k.cin}, InXform{}, so, params + cd.w_off, cd.w3, nullptr, k.cin, k.cout, 1, 0, buf(k.Yd));
            }
            launch_bn_add_relu(ctx, buf(k.Y3), c3.scale(), c3.shift(), buf(k.Yd), cd.scale(), cd.shift(), M, k.cout,
                               MutView{buf(k.A), k.cout}, MutView{});
        } else {
            launch_bn_add_relu(ctx, buf(k.Y3), c3.scale(), c3.shift(), a_in, nullptr, nullptr, M, k.cout, MutView{buf(k.A), k.cout}, MutView{});
        }
        a_in = buf(k.A);
    }
    // FPN: laterals, top-down merge, output convs, extra level
    const int F = out_ch;
    int last[4], bi = -1;
    for (int s = 0; s < 4; ++s) { bi += kBlocksPerStage[s]; last[s] = bi; }
    for (int i = 3; i >= 0; --i) {
        const BBlock& k = bb[last[i]];
        const Shape s{n, h >> (i + 2), w >> (i + 2)};
        ConvBN& ci = convs[fpn_inner[i]];
        conv(this, View{buf(k.A), k.cout}, InXform{}, s, params + ci.w_off, ci.w3, params + ci.b_off, k.cout, F, 1, 0, buf(fL[i]));
        if (i == 3) launch_copy_d2d(ctx, buf(fM[i]), buf(fL[i]), (size_t)s.N * s.H * s.W * F * sizeof(float));
        else launch_fpn_merge_fwd(ctx, buf(fL[i]), buf(fM[i + 1]), s.N, s.H, s.W, F, buf(fM[i]));
        ConvBN& cl = convs[fpn_layer[i]];
        conv(this, View{buf(fM[i]), F}, InXform{}, s, params + cl.w_off, cl.w3, params + cl.b_off, F, F, 3, 1, buf(fP[i]));
    }
    launch_subsample2(ctx, buf(fP[3]), n, h >> 5, w >> 5, F, buf(fP6));
}

// dP2..dP6 sit in fdP[0..3] / fdP6 (rfi_backbone_backward copies them there)
void BackboneModel::backward_pass(const float* x_dev, const uint8_t*, int n, int h, int w) {
    side_bound = 2;                   // (measured 31.8 / 32.2 / 32.9 ms per step of the detector at bound 2 / bound 5 / no side stream)
    const int F = out_ch;
    int last[4], bi = -1;
    for (int s = 0; s < 4; ++s) { bi += kBlocksPerStage[s]; last[s] = bi; }
    float* ws = buf(ws_red);
    // ---- FPN.  dM_i = dgrad(layer_block_i)(dP_i) + nearest-2x adjoint of dM_{i-1}; dL_i = dM_i; dC_i = dgrad(inner_i)(dM_i)
    launch_subsample2_bwd_add(ctx, buf(fdP6), n, h >> 5, w >> 5, F, buf(fdP[3]));
    float* dC[4] = {buf(bG[2]), buf(bG[3]), buf(bG[4]), buf(bG[5])};
    for (int i = 0; i < 4; ++i) {                   // fine to coarse: dM_i needs dM_{i-1}
        const Shape s{n, h >> (i + 2), w >> (i + 2)};
        const int64_t M = (int64_t)s.N * s.H * s.W;
        ConvBN& cl = convs[fpn_layer[i]];
        launch_channel_sum(ctx, View{buf(fdP[i]), F}, M, F, ws, grads + cl.b_off);
        wgrad_on_side(wgrad(this, View{buf(fM[i]), F}, InXform{}, buf(fdP[i]), F, F, s, 3, 1, grads + cl.w_off), nullptr);
        conv(this, View{buf(fdP[i]), F}, InXform{}, s, cl.wd, cl.wd3, nullptr, F, F, 3, 1, buf(fdM[i]));
        if (i > 0) {                                // + the share of M_{i-1} = L_{i-1} + up(M_i)
            launch_fpn_merge_bwd_top(ctx, buf(fdM[i - 1]), n, h >> (i + 1), w >> (i + 1), F, buf(bG[0]));
            launch_add_inplace(ctx, buf(fdM[i]), buf(bG[0]), M * F);
        }
        const BBlock& k = bb[last[i]];
        ConvBN& ci = convs[fpn_inner[i]];
        launch_channel_sum(ctx, View{buf(fdM[i]), F}, M, F, ws, grads + ci.b_off);
        wgrad_on_side(wgrad(this, View{buf(k.A), k.cout}, InXform{}, buf(fdM[i]), F, k.cout, s, 1, 0, grads + ci.w_off), nullptr);
        conv(this, View{buf(fdM[i]), F}, InXform{}, s, ci.wd, ci.wd3, nullptr, F, k.cout, 1, 0, dC[i]);
    }
    // ---- body, last block first.  gout: gradient w.r.t. the block output A
    float* gout = buf(bG[0]);
    float* gother = buf(bG[1]);
    {
        const BBlock& k = bb.back();
        launch_copy_d2d(ctx, gout, dC[3], (size_t)n * (h >> 5) * (w >> 5) * k.cout * sizeof(float));
    }
    for (int b = (int)bb.size() - 1; b >= 0; --b) {
        BBlock& k = bb[b];
        ConvBN &c1 = convs[k.c1], &c2 = convs[k.c2], &c3 = convs[k.c3];
        const Shape si{n, h >> k.lvl_in, w >> k.lvl_in}, so{n, h >> k.lvl, w >> k.lvl};
        const int64_t Mo = (int64_t)so.N * so.H * so.W, Mi = (int64_t)si.N * si.H * si.W;
        const float* a_in = b == 0 ? buf(bP0) : buf(bb[b - 1].A);
        // The weight gradients run on the side stream next to this chain (its masks, affine backward passes, space-to-depth
        // forms and shortcut adds are memory-bound).  What they read -- dY3, dY2, dY1, dYd -- lives in buffers of its own by
        // block index mod 3: block b - 3 rewrites them, and with a run-ahead bound of up to 5 side launches the main stream has
        // waited for every weight gradient of block b by then (a block issues at least three: after block b - 2's last,
        // launch i + 8 counted from block b's first, it has waited for launch i + 3 or later)
        const int par = b % 3;
        float* t3 = buf(bT[0][par]);                // dz -> dY3            [Mo][cout]
        float* dA2 = buf(bT[1][par]);               // dA2 -> dY2           [Mo][width]
        float* dA1 = buf(bT[2][par]);               // dA1 -> dY1           [Mi][width]
        float* td = buf(bT[3][par]);                // dz -> dYd            [Mo][cout]
        // dz = gout * [A > 0] -> dY3 = dz * scale3
        launch_relu_mask(ctx, View{gout, k.cout}, View{}, View{buf(k.A), k.cout}, View{}, Mo, k.cout, t3);
        affine_bwd(this, c3, t3, buf(k.Y3), Mo, 1.0f);
        wgrad_on_side(wgrad(this, View{buf(k.Y2), k.width}, act_of(c2), t3, k.cout, k.width, so, 1, 0, grads + c3.w_off), nullptr);
        conv(this, View{t3, k.cout}, InXform{}, so, c3.wd, c3.wd3, nullptr, k.cout, k.width, 1, 0, dA2);
        affine_bwd(this, c2, dA2, buf(k.Y2), Mo, 0.0f);                   // -> dY2
        if (k.stride == 2) {
            {
                SideScope side(this);               // (the 2x2-form gradient goes back to the 3x3 layout behind its slab reduction)
                launch_wgrad(ctx, wgrad(this, View{buf(k.xs1), 4 * k.width}, InXform{k.sc4, k.sh4, 1, 0.0f}, dA2, k.width, 4 * k.width,
                                        so, 2, 1, buf(bdW)));
                launch_w_s2d(ctx, grads + c2.w_off, c2.cout, c2.cin, buf(bdW), false);
                side.end();
            }
            float* dXs = buf(bS);                   // scratch [Mo][4 width]
            conv(this, View{dA2, k.width}, InXform{}, so, c2.wds2d, c2.wds2d3, nullptr, k.width, 4 * k.width, 2, 0, dXs);
            launch_d2s_add(ctx, dXs, nullptr, View{}, n, si.H, si.W, k.width, dA1);
        } else {
            wgrad_on_side(wgrad(this, View{buf(k.Y1), k.width}, act_of(c1), dA2, k.width, k.width, so, 3, 1, grads + c2.w_off), nullptr);
            conv(this, View{dA2, k.width}, InXform{}, so, c2.wd, c2.wd3, nullptr, k.width, k.width, 3, 1, dA1);
        }
        affine_bwd(this, c1, dA1, buf(k.Y1), Mi, 0.0f);                   // -> dY1
        wgrad_on_side(wgrad(this, View{a_in, k.cin}, InXform{}, dA1, k.width, k.cin, si, 1, 0, grads + c1.w_off), nullptr);
        float* dX = gother;                                               // [Mi][cin]
        conv(this, View{dA1, k.width}, InXform{}, si, c1.wd, c1.wd3, nullptr, k.width, k.cin, 1, 0, dX);
        if (k.cd >= 0) {
            ConvBN& cd = convs[k.cd];
            launch_relu_mask(ctx, View{gout, k.cout}, View{}, View{buf(k.A), k.cout}, View{}, Mo, k.cout, td);
            affine_bwd(this, cd, td, buf(k.Yd), Mo, 1.0f);                // -> dYd
            if (k.stride == 2) {
                wgrad_on_side(wgrad(this, View{buf(k.xsA), 4 * k.cin}, InXform{}, td, k.cout, k.cin, so, 1, 0, grads + cd.w_off), nullptr);
                float* dS = buf(bS);
                conv(this, View{td, k.cout}, InXform{}, so, cd.wd, cd.wd3, nullptr, k.cout, k.cin, 1, 0, dS);
                launch_subsample2_bwd_add(ctx, dS, n, si.H, si.W, k.cin, dX);      // the projection saw x[:, ::2, ::2]
            } else {
                wgrad_on_side(wgrad(this, View{a_in, k.cin}, InXform{}, td, k.cout, k.cin, so, 1, 0, grads + cd.w_off), nullptr);
                float* dS = buf(bS);
                conv(this, View{td, k.cout}, InXform{}, so, cd.wd, cd.wd3, nullptr, k.cout, k.cin, 1, 0, dS);
                launch_add_inplace(ctx, dX, dS, Mi * k.cin);
            }
        } else {                                    // identity shortcut: + gout * [A > 0]
            launch_relu_mask(ctx, View{gout, k.cout}, View{}, View{buf(k.A), k.cout}, View{dX, k.cin}, Mo, k.cout, dX);
        }
        // dX is the gradient w.r.t. this block's input = the previous block's output (or the pooled stem output); a stage
        // boundary also receives the lateral connection's gradient
        if (b > 0 && bb[b - 1].stage != k.stage) launch_add_inplace(ctx, dX, dC[bb[b - 1].stage], Mi * k.cin);
        std::swap(gout, gother);
    }
    {   // stem: gout = gradient w.r.t. the pooled tensor
        ConvBN& c = convs[0];
        const int H2 = h / 2, W2 = w / 2;
        float* dA0 = gother;
        launch_maxpool3_bwd(ctx, gout, reinterpret_cast<const unsigned*>(buf(bArg)), n, H2, W2, c.cout, dA0);
        affine_bwd(this, c, dA0, buf(bY0), (int64_t)n * H2 * W2, 0.0f);
        (void)x_dev;                                  // (its K-packed copy from the forward pass is the operand)
        const int Kp = stem_kp();
        {
            SideScope side(this);
            launch_wgrad(ctx, wgrad(this, View{buf(bCol), Kp}, InXform{}, dA0, c.cout, Kp, Shape{n, H2, W2}, 1, 0, buf(bWp)));
            launch_w_pack(ctx, grads + c.w_off, 49, c.cout, in_ch, Kp, buf(bWp), false);
            side.end();
        }
    }
    side_join();
    bucket_ready(0, n_flat);
}

// conv.<i>: raw (pre-BatchNorm) output of convs[i] on its own output grid; pool: the pooled stem; block.<b>: output of
// Bottleneck b; merged.<i> / dmerged.<i>: the top-down merged map of FPN level i and its gradient (after a backward pass)
void BackboneModel::debug_tensor(const std::string& name, const std::string& base, int idx, bool, CallScope&, const float*& src, size_t& n) {
    auto px = [&](int lvl) { return (size_t)pN * (pH >> lvl) * (pW >> lvl); };
    if (base == "conv") {
        RFI_REQUIRE(idx >= 0 && idx < (int)convs.size(), "debug_tensor: conv index out of range");
        int b = idx == 0 ? bY0 : -1;
        for (auto& k : bb) {
            if (idx == k.c1) b = k.Y1;
            else if (idx == k.c2) b = k.Y2;
            else if (idx == k.c3) b = k.Y3;
            else if (idx == k.cd) b = k.Yd;
        }
        for (int i = 0; i < 4; ++i) {
            if (idx == fpn_inner[i]) b = fL[i];
            else if (idx == fpn_layer[i]) b = fP[i];
        }
        RFI_REQUIRE(b >= 0, "debug_tensor: conv index out of range");
        src = buf(b);
        n = px(convs[idx].level) * convs[idx].cout;
    } else if (name == "pool") {
        src = buf(bP0);
        n = px(2) * feat;
    } else if (base == "block") {
        RFI_REQUIRE(idx >= 0 && idx < (int)bb.size(), "debug_tensor: block index out of range");
        src = buf(bb[idx].A);
        n = px(bb[idx].lvl) * bb[idx].cout;
    } else if (base == "merged" || base == "dmerged") {
        RFI_REQUIRE(idx >= 0 && idx < 4, "debug_tensor: FPN level out of range");
        src = buf(base == "merged" ? fM[idx] : fdM[idx]);
        n = px(idx + 2) * out_ch;
    } else {
        throw Error("debug_tensor: unknown tensor " + name);
    }
}

BackboneModel::~BackboneModel() {
    if (!ctx) return;
    ctx->activate();
    if (rs_wpool) ctx->release(rs_wpool);
}

// every conv once at its output resolution (the stem's 7x7 has stride 2)
void BackboneModel::algorithmic_flops(int n, int h, int w, double& fwd, double& step) const {
    double f = 0;
    for (auto& c : convs) f += 2.0 * n * (double)(h >> c.level) * (w >> c.level) * c.R * c.R * c.cin * c.cout;
    fwd = f;
    step = 3.0 * f - 2.0 * n * (double)(h >> 1) * (w >> 1) * 49.0 * convs[0].cin * convs[0].cout;
}
