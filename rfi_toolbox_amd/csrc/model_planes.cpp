// The U-Net step (rfi_toolbox/models/unet.py:41-77, scripts/train_model.py:139-151) on the PLANE kernels
// (planes.hpp): the data flow of the bfloat16 compute mode (P = 1: activations live in HBM as bf16) and of the
// float32-by-3xbf16 arithmetic on pre-split pieces (P = 3, `float32_planes`).
//
// What is stored per DoubleConv level (BatchNorm, loss, optimiser and every per-channel statistic stay float32):
//   Y1, Y2      raw conv outputs, float32 (BatchNorm statistics come out of the conv epilogue; the backward pass
//               needs the pre-BatchNorm values)
//   A1          act(BN(Y1)) as planes: written once by act_split, read by conv2 AND by conv2's weight gradient
//   skip, pool  act(BN(Y2)) and its 2x2 max-pool as planes, written by ONE kernel (bn_relu_pool_planes): read by
//               the decoder's first conv (second K-segment; torch.cat never happens), the next level's first conv
//               and both weight gradients
//   up          ConvTranspose output (float32, from the round-1 kernel) -> planes (first K-segment of the decoder)
//   dY          BatchNorm backward writes the gradient w.r.t. the raw conv output as planes: read by the
//               input-gradient conv and by the weight gradient
// The contraction kernels therefore never convert, split or transform an operand: they copy 16-byte pieces
// HBM -> LDS by LDS-DMA and feed v_mfma_f32_32x32x16_bf16.
#include <algorithm>

#include "model.hpp"

using namespace rfi;

namespace rfi {

void PlaneBuf::ensure(rfi_ctx* c, int64_t pixels, int C, int P) {
    const size_t need = plane_elems(pixels, C, P);
    nchunks = plane_chunks(C);
    pstride = (int64_t)nchunks * P * 16;
    if (need <= elems && p) {
        // a smaller shape in the allocation of a larger one: the zero area the kernels look for lies behind the tensor of THIS
        // shape (launch_pconv: x_zero = pixels * pstride * 2 bytes), where the larger shape left activations
        if (need != used && need < elems) RFI_CHECK_HIP(hipMemsetAsync(p + need, 0, 64, c->stream));
        used = need;
        return;
    }
    if (p) c->release(p);
    ctx = c;
    p = static_cast<bf16_t*>(c->alloc(need * 2 + 64));
    // zero once: channel padding is never written by the BatchNorm-backward producer, and the 64-byte tail is
    // where the LDS-DMA of out-of-image halo pixels points
    RFI_CHECK_HIP(hipMemsetAsync(p, 0, need * 2 + 64, c->stream));
    elems = used = need;
}
void PlaneBuf::free() {
    if (p && ctx) ctx->release(p);
    p = nullptr;
    elems = used = 0;
}

}  // namespace rfi

void UNetModel::make_plane_slots() {
    const int D = depth;
    auto one = [&]() { pl.emplace_back(); return (int)pl.size() - 1; };
    auto mk = [&](std::vector<int>& v) { v.assign(D + 1, -1); for (int l = 1; l <= D; ++l) v[l] = one(); };      // one per level
    mk(pA1e); mk(pSkip); mk(pPool); mk(pUp); mk(pA1d); mk(pdYa); mk(pdYb); mk(pdYaE); mk(pdYbE); mk(pUpIn);
    pXin = one(); pA1b = one(); pdYbottA = one(); pdYbottB = one();
    upf.assign(D + 1, -1);
    for (int l = 1; l <= D; ++l) upf[l] = new_buf();
    // the bfloat16 twins of the flow tensors (prepare_planes allocates them where the mode stores them)
    for (auto* v : {&encY1, &encY2, &decY1, &decY2, &gA, &gB, &dconcat, &dpool})
        for (int l = 1; l <= D; ++l) (*v)[l].b16 = one();
    for (FlowTensor* t : {&bottY1, &bottY2, &gBottA, &gBottB}) t->b16 = one();
    gAdec = gA;
    if (!resnet_encoder) return;
    rpStemY = one(); rpA0 = one(); rpdY0 = one(); rp_dA1 = one(); rp_dX = one(); rp_dz[0] = one(); rp_dz[1] = one();
    rpb.assign(blocks.size(), ResPlanes());
    for (size_t bi = 0; bi < blocks.size(); ++bi) {
        ResPlanes& r = rpb[bi];
        const ResBlock& b = blocks[bi];
        r.Y1 = one(); r.Y2 = one(); r.A1 = one(); r.dY1 = one(); r.dY2 = one();
        // a stage's output is the decoder's skip tensor; the last stage's is pooled (and copied there) by one kernel
        r.A = ((bi & 1) && b.level < D) ? pSkip[b.level] : one();
        if (b.stride == 2) { r.Yd = one(); r.dYd = one(); }
    }
}

void UNetModel::prepare_planes(int n, int h, int w) {
    const int P = planesP, D = depth;
    const bool rs = resnet_encoder;                    // ResNet-style encoder: its own tensors instead of the U-Net encoder's
    auto pixels = [&](int l) { return (int64_t)n * (h >> (l - 1)) * (w >> (l - 1)); };      // of level l (D + 1: the bottleneck)
    const int64_t M1 = pixels(1), Mb = pixels(D + 1);
    const int Cb = feat << D;
    pl[pXin].ensure(ctx, M1, in_ch, P);
    for (int l = 1; l <= D; ++l) {
        const int64_t M = pixels(l);
        const int C = feat << (l - 1);
        for (int i : {pSkip[l], pUp[l], pA1d[l], pdYa[l], pdYb[l]}) pl[i].ensure(ctx, M, C, P);
        if (!rs) for (int i : {pA1e[l], pdYaE[l], pdYbE[l]}) pl[i].ensure(ctx, M, C, P);
        if (!rs || l == D) pl[pPool[l]].ensure(ctx, M / 4, C, P);
        bufs[upf[l]].ensure(ctx, (size_t)M * C);
    }
    for (int i : {pA1b, pdYbottA, pdYbottB}) pl[i].ensure(ctx, Mb, Cb, P);
    y16_flow = P == 1 && feat % 4 == 0;
    g16_flow = y16_flow && feat % 16 == 0;
    convt_planes = g16_flow && feat % 32 == 0;
    // ---- Where every flow tensor lives (DESIGN.md section 3 has the same table): t is a bfloat16 tensor iff `half`, and its
    // bfloat16 storage is allocated here -- unless another owner has the tensor (own = false).  This block is the only place
    // that reads the gates to choose a storage.  The float32 tensors of prepare_shape stay allocated either way
    auto place = [&](FlowTensor& t, bool half, int64_t M, int C, bool own = true) {
        t.half = half;
        if (half && own) pl[t.b16].ensure(ctx, M, C, 1);
    };
    const bool y16 = y16_flow, g16 = g16_flow, ctp = convt_planes;
    for (int l = 1; l <= D; ++l) {
        const int64_t M = pixels(l);
        const int C = feat << (l - 1);
        place(encY1[l], y16, M, C, !rs);              // (the ResNet-style encoder owns its raw outputs: rpb)
        place(encY2[l], y16, M, C, !rs);
        place(decY1[l], y16, M, C);
        place(decY2[l], l == 1 ? y16 : ctp, M, C);    // the head reads level 1, a transposed conv the others
        place(gB[l], g16, M, C);
        place(dpool[l], g16, M / 4, C, !rs || l == D);
        place(dconcat[l], ctp, M, 2 * C);
        // gA.<l> has two storages in one pass, on the same tensors.  Decoder phase: the head (one output channel) writes level 1,
        // a transposed conv on the plane kernels the others.  Encoder phase: the max-pool backward writes it (the ResNet-style
        // encoder has no such tensor; the head's bfloat16 gA.1 is allocated for it at any out_ch)
        place(gAdec[l], l == 1 ? g16 && out_ch == 1 : ctp, M, C);
        place(gA[l], g16, M, C, !rs || l == 1);
    }
    place(bottY1, y16, Mb, Cb);
    place(bottY2, ctp, Mb, Cb);                        // (read by the transposed conv: float32 for the round-1 kernel)
    place(gBottA, ctp, Mb, Cb);
    place(gBottB, g16, Mb, Cb);
    if (convt_planes)                                  // the input of decoder l's transposed conv: level l + 1, 2 C channels
        for (int l = 1; l <= D; ++l) pl[pUpIn[l]].ensure(ctx, pixels(l + 1), feat << l, 1);
    if (rs) {
        RFI_REQUIRE(P == 1 && y16_flow && g16_flow, "UNetResNet18 on the plane kernels: bfloat16 flow with init_features % 16 == 0 only");
        for (int i : {rpStemY, rpA0, rpdY0, rp_dA1, rp_dX, rp_dz[0], rp_dz[1]}) pl[i].ensure(ctx, M1, feat, 1);   // (M C halves per level)
        for (size_t bi = 0; bi < blocks.size(); ++bi) {
            const ResBlock& b = blocks[bi];
            const ResPlanes& r = rpb[bi];
            const int64_t M = (int64_t)n * (h >> (b.level - 1)) * (w >> (b.level - 1));
            for (int i : {r.Y1, r.Y2, r.A1, r.A, r.dY1, r.dY2}) pl[i].ensure(ctx, M, b.cout, 1);
            if (b.stride == 2) for (int i : {r.Yd, r.dYd}) pl[i].ensure(ctx, M, b.cout, 1);
        }
    }
    // weight-gradient slabs of the plane kernel: the descriptors the backward pass will launch, from the same builders with null
    // operands (the plan comes from the shape alone: the workspace the builders point at need not exist yet)
    auto none = [](int C) { return PlaneSeg{nullptr, 0, plane_chunks(C)}; };
    for (size_t ci = 0; ci < convs.size(); ++ci) {
        const ConvBN& c = convs[ci];
        const bool two = (int)ci >= i_bott + 2 && (((int)ci - (i_bott + 2)) & 1) == 0;      // decoder conv1: [up | skip]
        const PlaneSeg in[2] = {none(two ? c.cin / 2 : c.cin), none(c.cin / 2)};
        need_slab(pwgrad_slab_floats(pwgrad_args(c, in, two ? 2 : 1, none(c.cout), Shape{n, h >> (c.level - 1), w >> (c.level - 1)})));
    }
    if (convt_planes)
        for (int k = 0; k < D; ++k)               // (decoder level D - k: the grid of its input)
            need_slab(pwgrad_slab_floats(convt_pwgrad_args(ups[k], none(ups[k].cout), none(ups[k].cin), Shape{n, h >> (D - k), w >> (D - k)})));
}

PWgradArgs UNetModel::pwgrad_args(const ConvBN& c, const PlaneSeg* in, int nseg, PlaneSeg dY, Shape s) {
    PWgradArgs wa;
    wa.xop[0] = in[0];
    if (nseg > 1) wa.xop[1] = in[1];
    wa.nseg = nseg;
    wa.seg_c[0] = nseg > 1 ? c.cin / 2 : c.cin;
    wa.seg_c[1] = nseg > 1 ? c.cin / 2 : 0;
    wa.cx_layout = c.cin_p;
    wa.yop = dY;
    wa.Cy = c.cout;
    wa.P = planesP;
    wa.N = s.N; wa.H = s.H; wa.W = s.W; wa.Hx = s.H * c.stride; wa.Wx = s.W * c.stride;
    wa.R = c.R; wa.S = c.stride; wa.pad = c.R == 3 ? 1 : 0;
    wa.dw = grads + c.w_off;
    wa.tap_stride = (int64_t)c.cin_p * c.cout;
    wa.sy = c.cin_p; wa.sx = 1;
    wa.algo_flops = 2.0 * s.N * s.H * s.W * (double)(c.R * c.R) * c.cin * c.cout;
    wa.slab = buf(ws_slab);
    wa.slab_floats = bufs[ws_slab].n;
    return wa;
}

// dW[tap][cout][cin] = sum_pixels act(prev)[i, j, cin] * dUp[2 i + a, 2 j + b, cout]
PWgradArgs UNetModel::convt_pwgrad_args(const UpConv& u, PlaneSeg dUp, PlaneSeg in, Shape s) {
    PWgradArgs wa;
    wa.xop[0] = dUp; wa.nseg = 1; wa.seg_c[0] = u.cout;
    wa.yop = in; wa.Cy = u.cin; wa.P = 1;
    wa.N = s.N; wa.H = s.H; wa.W = s.W; wa.Hx = 2 * s.H; wa.Wx = 2 * s.W;
    wa.R = 2; wa.S = 2; wa.pad = 0;
    wa.dw = grads + u.w_off;
    wa.tap_stride = (int64_t)u.cin * u.cout;
    wa.sy = 1; wa.sx = u.cin;
    wa.algo_flops = 2.0 * s.N * s.H * s.W * 4.0 * u.cin * u.cout;
    wa.slab = buf(ws_slab);
    wa.slab_floats = bufs[ws_slab].n;
    return wa;
}

// filters of every 3x3 layer in MFMA B-operand order, both directions, rebuilt with the dgrad layouts after each
// optimiser step by ONE batched launch
void UNetModel::refresh_plane_weights(Half half) {
    const int P = planesP, IB = i_bott;
    auto two_seg = [&](size_t ci) { return (int)ci >= IB + 2 && (((int)ci - (IB + 2)) & 1) == 0; };      // decoder conv1: [up | skip]
    auto has_wBd = [&](const ConvBN& c) { return c.R == 3 && c.stride == 1; };      // (the other shapes' input gradients: class tables)
    if (!wb_pool) {
        // the table: every forward-direction image first (what the forward pass reads), then the input-gradient direction
        // (dgrad layouts, parity-class tables) -- the second half can be rebuilt on the side stream under the forward pass
        size_t need = 0, cls_need = 0;
        for (size_t ci = 0; ci < convs.size(); ++ci) {
            const ConvBN& c = convs[ci];
            const bool two = two_seg(ci);
            need += wb_elems(c.R * c.R, c.cout, two ? c.cin / 2 : c.cin_p, two ? c.cin / 2 : 0, P) + 32;
            if (has_wBd(c)) need += wb_elems(9, c.cin_p, c.cout, 0, P) + 32;
        }
        for (auto& b : blocks)
            if (b.stride == 2) {
                need += wb_elems(4, b.cin, b.cout, b.cout, 1) + 32 + 3 * (wb_elems(4, b.cin, b.cout, 0, 1) + 32);
                cls_need += s2_class_floats(b.cout, b.cin);
            }
        if (P == 1)
            for (auto& u : ups) need += wb_elems(1, 4 * u.cout, u.cin, 0, 1) + 32 + wb_elems(4, u.cin, u.cout, 0, 1) + 32;
        wb_pool = static_cast<bf16_t*>(ctx->alloc(need * 2));
        RFI_CHECK_HIP(hipMemsetAsync(wb_pool, 0, need * 2, ctx->stream));       // the zero tails stay zero
        if (cls_need && !rs_cls_pool) rs_cls_pool = static_cast<float*>(ctx->alloc(cls_need * sizeof(float)));
        std::vector<WBDesc> hd;
        size_t o = 0, co = 0;
        // the image of `taps` filters [cout][cin] at `src`, its K in one or two segments: the next region of the pool (+ its
        // 32-element tail) and one descriptor
        auto image = [&](double& bytes, const float* src, int taps, int cout, int cin, int seg0, int seg1, int planes) {
            bf16_t* dst = wb_pool + o;
            const size_t e = wb_elems(taps, cout, seg0, seg1, planes);
            o += e + 32;
            hd.push_back(WBDesc{src, dst, taps, cout, cin, {seg0, seg1}, planes});
            bytes += 2.0 * e + 4.0 * taps * cin * cout;
            return dst;
        };
        for (size_t ci = 0; ci < convs.size(); ++ci) {
            ConvBN& c = convs[ci];
            const bool two = two_seg(ci);
            c.wBf = image(wb.bytes_fwd, params + c.w_off, c.R * c.R, c.cout, c.cin_p, two ? c.cin / 2 : c.cin_p, two ? c.cin / 2 : 0, P);
        }
        if (P == 1)                               // forward layout [4][cout][cin] = one 1x1 contraction with 4 cout channels
            for (auto& u : ups) u.wBf = image(wb.bytes_fwd, params + u.w_off, 1, 4 * u.cout, u.cin, u.cin, 0, 1);
        wb.n_fwd = (int)hd.size();
        wb.bytes = wb.bytes_fwd;
        for (ConvBN& c : convs)
            if (has_wBd(c)) c.wBd = image(wb.bytes, c.wd, 9, c.cin_p, c.cout, c.cout, 0, P);
        if (P == 1)                               // dgrad layout [4][cin][cout]
            for (auto& u : ups) u.wBd = image(wb.bytes, u.wd, 4, u.cin, u.cout, u.cout, 0, 1);
        for (size_t bi = 0; bi < blocks.size(); ++bi) {
            const ResBlock& b = blocks[bi];
            if (b.stride != 2) continue;
            ResPlanes& r = rpb[bi];
            r.cls = rs_cls_pool + co;
            co += s2_class_floats(b.cout, b.cin);
            for (int c = 0; c < 4; ++c)           // (class 0: two K segments)
                r.wBcls[c] = image(wb.bytes, r.cls + s2_class_offset(c, b.cout, b.cin), 4, b.cin, c == 0 ? 2 * b.cout : b.cout, b.cout,
                                   c == 0 ? b.cout : 0, 1);
        }
        wb.n = (int)hd.size();
        wb.descs = ctx->upload_table(hd.data(), hd.size() * sizeof(WBDesc));
    }
    if (half != Half::InputGrad) wb.launch(ctx, Half::Forward);
    if (half != Half::Forward) {      // (the class tables are sources of the table's second half: two launches also for Both)
        for (size_t bi = 0; bi < blocks.size(); ++bi) {
            const ResBlock& b = blocks[bi];
            if (b.stride == 2)
                launch_w_s2_classes(ctx, params + convs[b.c1].w_off, params + convs[b.cd].w_off, b.cout, b.cin, rpb[bi].cls);
        }
        wb.launch(ctx, Half::InputGrad);
    }
}

namespace {

// (s: the OUTPUT grid; a stride-2 layer reads an input of twice that size)
void run_pconv_bn(UNetModel* m, ConvBN& c, const PlaneSeg* in, int nseg, Shape s, FlowRef Y, bool train) {
    PConvArgs a;
    a.x[0] = in[0];
    if (nseg > 1) a.x[1] = in[1];
    a.nseg = nseg; a.P = m->planesP;
    a.N = s.N; a.H = s.H; a.W = s.W; a.Hin = s.H * c.stride; a.Win = s.W * c.stride;
    a.R = c.R; a.S = c.stride; a.pad = c.R == 3 ? 1 : 0;
    a.Cout = c.cout;
    a.wB = c.wBf;
    a.bias = m->params + c.b_off;
    if (Y.h) { a.y16 = Y.h; a.y_pstride = (int)Y.pstride; }
    else { a.y = Y.f; a.y_pstride = c.cout; a.round_y = m->y16_flow; }      // (float32 holding bf16-rounded values in the bf16 flow)
    a.Hout = s.H; a.Wout = s.W;
    a.algo_flops = 2.0 * s.N * s.H * s.W * (double)(c.R * c.R) * c.cin * c.cout;
    if (train) {
        a.stats = reinterpret_cast<double*>(m->buf(m->ws_red));
        a.stats_max_records = (int)(bn_stats_ws_floats(c.cout) / ((size_t)c.cout * 4));
    }
    launch_pconv(m->ctx, a);
    RFI_REQUIRE(!train || a.stats_records > 0 || !Y.h, "plane conv: no statistics records for a bfloat16 output");
    m->bn_tail(c, Y.f, (int64_t)s.N * s.H * s.W, train, a.stats_records);
}

// Conv3x3+BN+act twice: Y1 = conv(in) ; A1 = planes(act(BN(Y1))) ; Y2 = conv(A1)
void double_conv(UNetModel* m, ConvBN& c1, ConvBN& c2, const PlaneSeg* in, int nseg, Shape s, FlowRef Y1, PlaneBuf& A1,
                 FlowRef Y2, bool train) {
    run_pconv_bn(m, c1, in, nseg, s, Y1, train);
    const int64_t M = (int64_t)s.N * s.H * s.W;
    launch_act_split(m->ctx, View{Y1.f, c1.cout}, M, c1.cout, m->bn_xf(c1), m->planesP, A1.p, A1.pstride, Y1.h, Y1.pstride);
    const PlaneSeg a1 = A1.seg();
    run_pconv_bn(m, c2, &a1, 1, s, Y2, train);
}

}  // namespace

// ResNet-style encoder (model_resnet.cpp states the topology) on the bf16 flow.  Every tensor is bfloat16: raw conv outputs
// (statistics from the conv epilogues), activations as the operands of the next contraction.  Stride-2 layers read the
// full-resolution planes directly (the LDS halo tile has the stride): no space-to-depth copy.  A stage's output IS the
// decoder's skip tensor.  cur <- the pooled output of the last stage.
void UNetModel::forward_resnet_planes(PlaneSeg& cur, int n, int h, int w, bool train) {
    const int D = depth;
    {
        ConvBN& c = convs[0];
        const PlaneBuf &Y = pl[rpStemY], &A0 = pl[rpA0];
        run_pconv_bn(this, c, &cur, 1, Shape{n, h, w}, Y, train);
        launch_act_split(ctx, View{nullptr, c.cout}, (int64_t)n * h * w, c.cout, bn_xf(c), 1, A0.p, A0.pstride, Y.p, Y.pstride);
        side_rebuild_wd();                        // (the input-gradient-direction filter images: side stream, under the forward pass)
    }
    const PlaneBuf* a_in = &pl[rpA0];
    for (size_t bi = 0; bi < blocks.size(); ++bi) {
        ResBlock& b = blocks[bi];
        const ResPlanes& r = rpb[bi];
        ConvBN& c1 = convs[b.c1];
        ConvBN& c2 = convs[b.c2];
        Shape s{n, h >> (b.level - 1), w >> (b.level - 1)};
        const int64_t M = (int64_t)s.N * s.H * s.W;
        const PlaneBuf &Y1 = pl[r.Y1], &Y2 = pl[r.Y2], &A1 = pl[r.A1], &A = pl[r.A];
        const PlaneSeg in = a_in->seg();
        run_pconv_bn(this, c1, &in, 1, s, Y1, train);
        if (b.stride == 2) run_pconv_bn(this, convs[b.cd], &in, 1, s, pl[r.Yd], train);
        launch_act_split(ctx, View{nullptr, c1.cout}, M, c1.cout, bn_xf(c1), 1, A1.p, A1.pstride, Y1.p, Y1.pstride);
        const PlaneSeg a1 = A1.seg();
        run_pconv_bn(this, c2, &a1, 1, s, Y2, train);
        if (b.stride == 2) {
            ConvBN& cd = convs[b.cd];
            const PlaneBuf& Yd = pl[r.Yd];
            launch_bn_add_relu16(ctx, Y2.p, Y2.pstride, c2.scale(), c2.shift(), Yd.p, Yd.pstride, cd.scale(), cd.shift(), M, b.cout, A.p, A.pstride);
        } else {
            launch_bn_add_relu16(ctx, Y2.p, Y2.pstride, c2.scale(), c2.shift(), a_in->p, a_in->pstride, nullptr, nullptr, M, b.cout, A.p, A.pstride);
        }
        a_in = &A;
    }
    // MaxPool2d(2) of the last stage (identity "BatchNorm": scale 1, shift 0; the values are >= 0), + its copy as the skip
    const ResBlock& lb = blocks.back();
    launch_bn_relu_pool_planes(ctx, nullptr, n, h >> (D - 1), w >> (D - 1), lb.cout, rs_ones, rs_zeros, 0.0f, 1, pl[pSkip[D]].p,
                               pl[pSkip[D]].pstride, pl[pPool[D]].p, pl[pPool[D]].pstride, a_in->p, a_in->pstride);
    cur = pl[pPool[D]].seg();
}

void UNetModel::forward_planes(const float* x_dev, int n, int h, int w, bool train_mode) {
    const int D = depth, P = planesP;
    launch_act_split(ctx, View{x_dev, in_ch}, (int64_t)n * h * w, in_ch, InXform{}, P, pl[pXin].p, pl[pXin].pstride);
    PlaneSeg cur = pl[pXin].seg();
    const int IB = i_bott;
    if (resnet_encoder) forward_resnet_planes(cur, n, h, w, train_mode);
    else for (int l = 1; l <= D; ++l) {
        Shape s{n, h >> (l - 1), w >> (l - 1)};
        ConvBN& c1 = convs[2 * (l - 1)];
        ConvBN& c2 = convs[2 * (l - 1) + 1];
        const FlowRef y2 = flow(encY2[l]);
        double_conv(this, c1, c2, &cur, 1, s, flow(encY1[l]), pl[pA1e[l]], y2, train_mode);
        if (l == 1) side_rebuild_wd();            // (the input-gradient-direction filter images: side stream, under the forward pass)
        launch_bn_relu_pool_planes(ctx, y2.f, s.N, s.H, s.W, c2.cout, c2.scale(), c2.shift(), act_slope, P,
                                   pl[pSkip[l]].p, pl[pSkip[l]].pstride, pl[pPool[l]].p, pl[pPool[l]].pstride, y2.h, y2.pstride);
        cur = pl[pPool[l]].seg();
    }
    double_conv(this, convs[IB], convs[IB + 1], &cur, 1, Shape{n, h >> D, w >> D}, flow(bottY1), pl[pA1b], flow(bottY2), train_mode);
    FlowRef prevY = flow(bottY2);                 // what the next transposed conv reads, with its BatchNorm
    ConvBN* prevBN = &convs[IB + 1];
    for (int l = D; l >= 1; --l) {
        const int k = D - l;
        UpConv& u = ups[k];
        Shape sin{n, h >> l, w >> l};
        Shape s{n, h >> (l - 1), w >> (l - 1)};
        const PlaneBuf& up = pl[pUp[l]];
        if (convt_planes) {
            // ConvTranspose2d(k2, s2) on the plane kernels: the input activated once into planes, then ONE 1x1 contraction whose
            // 4 cout output channels are the four taps -- each lands on its own pixel of the 2 x 2 block (PConvArgs::zblocks)
            const int64_t Min = (int64_t)sin.N * sin.H * sin.W;
            const PlaneBuf& upin = pl[pUpIn[l]];
            launch_act_split(ctx, View{nullptr, u.cin}, Min, u.cin, bn_xf(*prevBN), 1, upin.p, upin.pstride, prevY.h, prevY.pstride);
            PConvArgs a;
            a.x[0] = upin.seg();
            a.nseg = 1; a.P = 1;
            a.N = sin.N; a.H = sin.H; a.W = sin.W; a.Hin = sin.H; a.Win = sin.W;
            a.R = 1; a.S = 1; a.pad = 0;
            a.Cout = 4 * u.cout;
            a.zblocks = u.cout / 32;
            a.wB = u.wBf;
            a.bias = params + u.b_off;
            a.y16 = up.p; a.y_pstride = (int)up.pstride;
            a.Hout = s.H; a.Wout = s.W; a.osy = 2; a.osx = 2;
            a.algo_flops = 2.0 * Min * 4.0 * u.cin * u.cout;
            launch_pconv(ctx, a);
        } else {
            // ConvTranspose2d(k2,s2): the round-1 kernel, float32 tensors (with a plane flow on, ws_need() == 0: no wave-specialised
            // copy exists for set_filters to find)
            ConvArgs a = convt_args(u, View{prevY.f, u.cin}, bn_xf(*prevBN), sin);
            // bf16 data flow with whole 16-channel chunks: the kernel writes the up-conv output as the bf16 operand of the
            // decoder's first conv directly; otherwise float32 + one conversion pass (which also zero-fills chunk padding)
            const bool direct = P == 1 && u.cout % 16 == 0 && conv_mfma_eligible(a) && up.pstride % 4 == 0;
            if (direct) {
                a.y16 = up.p;
                a.y = MutView{nullptr, (int)up.pstride};
            } else {
                a.y = MutView{buf(upf[l]), u.cout};
            }
            launch_conv(ctx, a);
            if (!direct)
                launch_act_split(ctx, View{buf(upf[l]), u.cout}, (int64_t)s.N * s.H * s.W, u.cout, InXform{}, P, up.p, up.pstride);
        }
        ConvBN& c1 = convs[IB + 2 + 2 * k];
        ConvBN& c2 = convs[IB + 2 + 2 * k + 1];
        const PlaneSeg in2[2] = {up.seg(), pl[pSkip[l]].seg()};      // cat([up, skip], dim=1) as two K-segments
        double_conv(this, c1, c2, in2, 2, s, flow(decY1[l]), pl[pA1d[l]], flow(decY2[l]), train_mode);
        prevY = flow(decY2[l]);                   // (float32 where the round-1 transposed conv reads it; the head reads either)
        prevBN = &c2;
    }
    const int64_t M1 = (int64_t)n * h * w;
    launch_head_fwd(ctx, prevY.ref(), M1, feat, prevBN->scale(), prevBN->shift(), params + head_w_off, params + head_b_off, out_ch,
                    buf(logits), act_slope);
    if (head_sigmoid) launch_sigmoid_fwd(ctx, buf(logits), M1 * out_ch, buf(probs));
}

namespace {

// dA: gradient w.r.t. the ACTIVATED output of conv c (float32, left untouched).  Writes dW / db / dgamma / dbeta
// and, if dx is a tensor, the gradient w.r.t. the conv's input (raw, `cin` channels per pixel: a float32 buffer or, in the bf16
// data flow, a dense bfloat16 [pixel][C] tensor).
// `next` (with its raw bfloat16 output next_Y): the layer whose activated output dx is the gradient of -- its BatchNorm-
// backward sums are then folded into the input-gradient conv's epilogue; returns the number of records left for it in
// the workspace (0: none, the caller's next call runs bn_bwd_reduce).
// slope_override: the activation slope of THIS layer's output instead of the model's (1: the output has no activation of its
// own -- a residual branch, whose masked gradient dA already is dz).  Layers with a stride or other taps (ResNet-style
// encoder): s is the OUTPUT grid, `in` the input of stride times that size, dx must be null (the caller runs the input
// gradient by parity classes).
int backward_pconv_bn(UNetModel* m, ConvBN& c, YRef dA, YRef Y, const PlaneSeg* in, int nseg, Shape s,
                      FlowRef dx, PlaneBuf& dYp, int have_records = 0, ConvBN* next = nullptr, YRef next_Y = YRef((const float*)nullptr),
                      const float* slope_override = nullptr) {
    rfi_ctx* ctx = m->ctx;
    const int64_t M = (int64_t)s.N * s.H * s.W;
    float* ws = m->buf(m->ws_red);
    const float slope = slope_override ? *slope_override : m->act_slope;
    RFI_REQUIRE((c.R == 3 && c.stride == 1) || !dx, "backward_pconv_bn: strided / 1x1 layers have no single input-gradient launch");
    if (have_records > 0)           // the kernel that produced dA left the BatchNorm-backward sums in the workspace
        launch_bn_bwd_finalize_records(ctx, ws, have_records, M, c.cout, c.c1(), c.c2(), m->grads + c.g_off, m->grads + c.be_off);
    else
        launch_bn_bwd_reduce(ctx, dA, Y, M, c.cout, c.scale(), c.shift(), c.mean(), c.invstd(), ws, c.c1(), c.c2(),
                             m->grads + c.g_off, m->grads + c.be_off, slope);
    const hipEvent_t dy_done = m->next_fork_event();         // completes with the kernel that writes dY
    // (dbias_deferred: the partial sums of the conv-bias gradient stay in the layer's own region; the pass finishes every
    // layer's with ONE batched launch at its end)
    const bool defer = m->dbias_deferred && c.has_bias;
    launch_bn_bwd_apply(ctx, dA, Y, M, c.cout, c.scale(), c.shift(), c.mean(), c.invstd(),
                        m->params + c.g_off, c.c1(), c.c2(), defer ? m->dbias_pool + c.dbias_rec_off : ws,
                        c.has_bias ? m->grads + c.b_off : nullptr, slope, dYp.p, dYp.pstride, m->planesP, dy_done, !defer);
    const PWgradArgs wa = m->pwgrad_args(c, in, nseg, dYp.seg(), s);
    {
        SideScope side(m, dy_done);
        launch_pwgrad(ctx, wa);
        side.end();
    }
    if (dx) {
        PConvArgs a;
        a.x[0] = dYp.seg();
        a.nseg = 1; a.P = m->planesP;
        a.N = s.N; a.H = s.H; a.W = s.W; a.Hin = s.H; a.Win = s.W;
        a.Cout = c.cin;                           // dx exists only for layers whose cin == cin_p
        a.wB = c.wBd;
        if (dx.h) { a.y16 = dx.h; a.y_pstride = (int)dx.pstride; }
        else { a.y = dx.f; a.y_pstride = c.cin; }
        a.Hout = s.H; a.Wout = s.W;
        a.algo_flops = 2.0 * s.N * s.H * s.W * 9.0 * c.cin * c.cout;
        if (next && next_Y.bf16) {
            a.stats = reinterpret_cast<double*>(ws);          // (this layer's dy sums have been finished out of it)
            a.stats_max_records = (int)(bn_stats_ws_floats(next->cout) / ((size_t)next->cout * 4));
            a.bwd_y16 = static_cast<const bf16_t*>(next_Y.p);
            a.bwd_yps = next_Y.stride(next->cout);
            a.bwd_scale = next->scale(); a.bwd_shift = next->shift();
            a.bwd_mean = next->mean(); a.bwd_invstd = next->invstd();
            a.bwd_slope = m->act_slope;                       // (`next` is a conv + BatchNorm + activation layer)
        }
        launch_pconv(ctx, a);
        return a.stats_records;
    }
    return 0;
}

}  // namespace

// Backward pass of the ResNet-style encoder on the bf16 flow.  Per BasicBlock (g = gradient w.r.t. the block's output, a sum of
// up to three tensors that is never materialised):
//   dz  = g * (a_out > 0)                                           one pass (relu_mask_sum16), read by both BatchNorm branches
//   main branch     BN2 backward (identity activation) -> dY2 planes; conv2's weight gradient (side stream) and input gradient dA1
//                   with BN1's backward sums folded into its epilogue; BN1 backward -> dY1 planes; conv1's weight gradient
//   identity block  dX = conv1's input gradient; the block's input gradient is dX + dz (the next relu_mask_sum16 adds them)
//   stride-2 block  projection: BNd backward of the same dz -> dYd planes, its weight gradient; the input gradient of conv1 AND
//                   of the projection as four 2x2 contractions, one per parity class of the input pixel, written with output
//                   stride 2 (class 0 takes the projection as a second K segment): no zero-stuffed tensor, no scatter pass
void UNetModel::backward_resnet_planes(int n, int h, int w) {
    const int D = depth;
    const float one = 1.0f;
    // gradient w.r.t. the last stage's output: skip gradient + max-pool routing of dpool (-> rp_dX, as "dX from above")
    {
        const ResBlock& lb = blocks.back();
        const PlaneBuf& A = pl[rpb.back().A];
        launch_pool_bwd_merge(ctx, A.ref(), n, h >> (D - 1), w >> (D - 1), lb.cout, rs_ones, rs_zeros, skip_grad(D, lb.cout),
                              flow(dpool[D]).ref(), nullptr, 0.0f, pl[rp_dX].p);
    }
    // (the scratch tensors rp_dA1 / rp_dX / rp_dz serve every level: as dense [M][C] tensors)
    const bf16_t* g0 = pl[rp_dX].p;               // the terms of g (dense bfloat16 [M][C]) ...
    const bf16_t* g1 = nullptr;
    YRef g2((const float*)nullptr);               // ... and the decoder's skip gradient (a view), at stage boundaries
    for (int bi = (int)blocks.size() - 1; bi >= 0; --bi) {
        ResBlock& b = blocks[bi];
        const ResPlanes& r = rpb[bi];
        ConvBN& c1 = convs[b.c1];
        ConvBN& c2 = convs[b.c2];
        Shape s{n, h >> (b.level - 1), w >> (b.level - 1)};
        const int64_t M = (int64_t)s.N * s.H * s.W;
        const PlaneBuf& a_in = bi == 0 ? pl[rpA0] : pl[rpb[bi - 1].A];
        PlaneBuf& dz = pl[rp_dz[bi & 1]];
        launch_relu_mask_sum16(ctx, g0, b.cout, g1, b.cout, g2, pl[r.A].p, pl[r.A].pstride, M, b.cout, dz.p, b.cout);
        const YRef dzr(dz.p, (int64_t)b.cout);
        const PlaneSeg a1 = pl[r.A1].seg();
        const FlowRef dA1(pl[rp_dA1].p, b.cout), dX(pl[rp_dX].p, b.cin);
        const int rec1 = backward_pconv_bn(this, c2, dzr, pl[r.Y2].ref(), &a1, 1, s, dA1, pl[r.dY2], 0, &c1, pl[r.Y1].ref(), &one);
        const PlaneSeg in = a_in.seg();
        if (b.stride == 1) {
            backward_pconv_bn(this, c1, dA1.ref(), pl[r.Y1].ref(), &in, 1, s, dX, pl[r.dY1], rec1);
            g0 = pl[rp_dX].p; g1 = dz.p; g2 = YRef((const float*)nullptr);
        } else {
            ConvBN& cd = convs[b.cd];
            backward_pconv_bn(this, c1, dA1.ref(), pl[r.Y1].ref(), &in, 1, s, FlowRef(), pl[r.dY1], rec1);
            backward_pconv_bn(this, cd, dzr, pl[r.Yd].ref(), &in, 1, s, FlowRef(), pl[r.dYd], 0, nullptr, YRef((const float*)nullptr), &one);
            for (int c = 0; c < 4; ++c) {
                PConvArgs a;
                a.x[0] = pl[r.dY1].seg();
                if (c == 0) a.x[1] = pl[r.dYd].seg();
                a.nseg = c == 0 ? 2 : 1; a.P = 1;
                a.N = s.N; a.H = s.H; a.W = s.W; a.Hin = s.H; a.Win = s.W;
                a.R = 2; a.S = 1; a.pad = 0;
                a.Cout = b.cin;
                a.wB = r.wBcls[c];
                a.y16 = pl[rp_dX].p; a.y_pstride = b.cin;
                a.Hout = 2 * s.H; a.Wout = 2 * s.W;
                a.osy = 2; a.osx = 2; a.ooy = c >> 1; a.oox = c & 1;
                // (true work: 9 taps of conv1 + the projection over the M output pixels; the zero taps of the 2x2 forms are not counted)
                a.algo_flops = c == 0 ? 2.0 * M * (9.0 * b.cin * b.cout + (double)b.cin * b.cout) : 0.0;
                launch_pconv(ctx, a);
            }
            g0 = pl[rp_dX].p; g1 = nullptr;
            g2 = skip_grad(b.level - 1, b.cin);   // the previous stage's output is also a skip
        }
        bucket_ready(c1.w_off, (size_t)(bi + 1 < (int)blocks.size() ? convs[blocks[bi + 1].c1].w_off : convs[i_bott].w_off));
    }
    {                                             // stem: g = dX + dz of the first block, materialised once
        ConvBN& c = convs[0];
        Shape s{n, h, w};
        const int64_t M = (int64_t)n * h * w;
        PlaneBuf& g = pl[rp_dz[1]];               // (block 0 used rp_dz[0])
        launch_relu_mask_sum16(ctx, g0, c.cout, g1, c.cout, YRef((const float*)nullptr), nullptr, 0, M, c.cout, g.p, c.cout);
        const PlaneSeg in = pl[pXin].seg();
        backward_pconv_bn(this, c, YRef(g.p, (int64_t)c.cout), pl[rpStemY].ref(), &in, 1, s, FlowRef(), pl[rpdY0]);
        bucket_ready(0, convs[blocks[0].c1].w_off);
    }
}

void UNetModel::debug_plane_values(int pi, size_t M, int C, int P_, bool pad, bool to_host, CallScope& sc, const float*& src, size_t& n) {
    RFI_REQUIRE(pi >= 0 && pi < (int)pl.size() && pl[pi].p, "debug_tensor: this tensor does not exist in this mode");
    const PlaneBuf& b = pl[pi];
    RFI_REQUIRE(b.nchunks == plane_chunks(C) && b.used >= plane_elems((int64_t)M, C, P_), "debug_tensor: plane tensor of another shape");
    const int Cp = 16 * b.nchunks - C;
    n = M * (size_t)(pad ? Cp : C);
    if (!to_host || !n) return;
    float* tmp = sc.temp<float>(n);
    // (the padding lanes: the last chunk's lanes C % 16 .. 15 read as Cp channels of a tensor that starts there)
    const bf16_t* in = pad ? b.p + (size_t)(b.nchunks - 1) * P_ * 16 + (C & 15) : b.p;
    launch_planes_to_f32(ctx, in, b.pstride, (int64_t)M, pad ? Cp : C, P_, tmp, pad ? Cp : C);
    src = tmp;
}

// What the ResNet-style encoder leaves behind after a pass on the bf16 flow (forward_resnet_planes / backward_resnet_planes), as
// float32 values: every tensor is bfloat16, [pixels of its level][channels].  Reported with the element count of its LAST writer:
//   xin                       the input as the stem reads it (":pad": its padding lanes)
//   stemY, a0, dY0            the stem's raw output, its activation (block 0's input), the gradient w.r.t. the raw output
//   rY1.<b> rY2.<b> rYd.<b>   raw outputs of block b's conv1 / conv2 / projection (b = 0..7; rYd on the stride-2 blocks 2, 4, 6)
//   rA1.<b>, rA.<b>           act(BN1(Y1)) and the block's output (odd b below the last level: the decoder's skip tensor itself)
//   rdY1.<b> rdY2.<b> rdYd.<b>  the BatchNorm-backward outputs of the three layers
//   rskip, rpool              the last stage's output as the decoder's skip (a copy of rA.7) and its 2x2 max
//   rdpool                    the gradient w.r.t. rpool (the bottleneck's input gradient)
//   rdz.0, rdz.1, rdA1, rdX   scratch every block reuses; the last writers run at level 1, [n h w][feat]:
//                             rdz.0 = block 0's dz (blocks 6, 4, 2 wrote it before), rdz.1 = the stem's g = dX_0 + dz_0 (blocks 7, 5,
//                             3, 1 wrote their dz there before), rdA1 = block 0's dA1 (conv2's input gradient), rdX = block 0's dX
//                             (conv1's input gradient; before: the pool backward's merge and every block's dX / class launches)
bool UNetModel::debug_tensor_resnet_planes(const std::string& name, const std::string& base, int idx, bool to_host, CallScope& sc,
                                           const float*& src, size_t& n) {
    const int D = depth;
    const bool pad = name.find(":pad") != std::string::npos;
    auto pix = [&](int l) { return (size_t)pN * (pH >> (l - 1)) * (pW >> (l - 1)); };
    auto serve = [&](int pi, size_t M, int C) { debug_plane_values(pi, M, C, 1, pad, to_host, sc, src, n); return true; };
    struct One { const char* name; int pi; size_t M; int C; };
    const One ones[] = {{"xin", pXin, pix(1), in_ch}, {"stemY", rpStemY, pix(1), feat}, {"a0", rpA0, pix(1), feat}, {"dY0", rpdY0, pix(1), feat},
                        {"rdA1", rp_dA1, pix(1), feat}, {"rdX", rp_dX, pix(1), feat},
                        {"rskip", pSkip[D], pix(D), feat << (D - 1)}, {"rpool", pPool[D], pix(D) / 4, feat << (D - 1)},
                        {"rdpool", dpool[D].b16, pix(D) / 4, feat << (D - 1)}};
    for (const One& o : ones)
        if (base == o.name) {
            RFI_REQUIRE(idx == -1, "debug_tensor: " + base + " is one tensor: no index");
            return serve(o.pi, o.M, o.C);
        }
    if (base == "rdz") {
        RFI_REQUIRE(idx == 0 || idx == 1, "debug_tensor: rdz.0 or rdz.1");
        return serve(rp_dz[idx], pix(1), feat);
    }
    struct PerBlock { const char* name; int ResPlanes::*slot; };
    const PerBlock per[] = {{"rY1", &ResPlanes::Y1}, {"rY2", &ResPlanes::Y2}, {"rYd", &ResPlanes::Yd}, {"rA1", &ResPlanes::A1}, {"rA", &ResPlanes::A},
                            {"rdY1", &ResPlanes::dY1}, {"rdY2", &ResPlanes::dY2}, {"rdYd", &ResPlanes::dYd}};
    for (const PerBlock& p : per)
        if (base == p.name) {
            RFI_REQUIRE(idx >= 0 && idx < (int)blocks.size(), "debug_tensor: block index out of range");
            const int pi = rpb[idx].*(p.slot);
            RFI_REQUIRE(pi >= 0, "debug_tensor: only a stride-2 block has a projection");
            return serve(pi, pix(blocks[idx].level), blocks[idx].cout);
        }
    return false;
}

// What the plain U-Net leaves in HBM after a pass on a plane data flow, as float32 values (parity debugging only: no pass calls
// this).  A tensor the mode stores as bfloat16 or as planes is converted into a temporary of the call (exact: every bf16 value
// is a float32 value; P = 3: the sum of the pieces); "<name>:pad" returns the lanes behind the C channels of the last
// 16-channel chunk of every pixel, [pixels][16 chunks - C] (empty when C % 16 == 0), which every consumer expects to be zero.
// Every name is a tensor of its own that the pass writes once, except gA.<l> / gB.<l>: the decoder phase and the encoder phase
// of the backward pass share them, so they hold the ENCODER's gradients afterwards (the decoder's are gone: not exposed).
void UNetModel::debug_tensor_planes(const std::string& name, const std::string& base, int idx, bool to_host, CallScope& sc, const float*& src,
                                    size_t& n) {
    const int D = depth, P = planesP;
    const bool pad = name.find(":pad") != std::string::npos;
    auto pix = [&](int l) { return (size_t)pN * (pH >> (l - 1)) * (pW >> (l - 1)); };       // pixels of level l (D + 1: the bottleneck)
    // a float32 tensor of the model
    auto f32 = [&](int bi, size_t M, int C) {
        RFI_REQUIRE(!pad, "debug_tensor: this tensor is stored as float32 in this mode: it has no padding lanes");
        RFI_REQUIRE(bi >= 0 && bufs[bi].p && bufs[bi].n >= M * C, "debug_tensor: this tensor does not exist in this mode");
        src = buf(bi);
        n = M * C;
    };
    // a plane tensor of P_ pieces (bfloat16 tensors: P_ = 1), C channels per pixel
    auto planes = [&](int pi, size_t M, int C, int P_) { debug_plane_values(pi, M, C, P_, pad, to_host, sc, src, n); };
    // the flow tensors: bfloat16 or float32, as the mode stores them
    size_t M = 0;
    int C = 0;
    if (const FlowTensor* t = flow_named(base, idx, M, C)) return t->half ? planes(t->b16, M, C, 1) : f32(t->f32, M, C);
    // the plane tensors (P pieces) and the float32 tensors that are no flow tensors: one per level l (the pixels of level
    // l + down, feat << (l - 1 + wide) channels), or a single one (xin: the input's shape; the others: the bottleneck's)
    struct Row { const char* name; const std::vector<int>* levels; int one; int P; int down, wide; };
    const Row rows[] = {{"xin", nullptr, pXin, P, 0, 0},
                        {"a1e", &pA1e, -1, P, 0, 0}, {"skip", &pSkip, -1, P, 0, 0}, {"pooled", &pPool, -1, P, 1, 0}, {"up", &pUp, -1, P, 0, 0},
                        {"a1d", &pA1d, -1, P, 0, 0}, {"a1b", nullptr, pA1b, P, 0, 0}, {"upin", &pUpIn, -1, 1, 1, 1},
                        {"dYa", &pdYa, -1, P, 0, 0}, {"dYb", &pdYb, -1, P, 0, 0}, {"dYaE", &pdYaE, -1, P, 0, 0}, {"dYbE", &pdYbE, -1, P, 0, 0},
                        {"dYbottA", nullptr, pdYbottA, P, 0, 0}, {"dYbottB", nullptr, pdYbottB, P, 0, 0},
                        // float32 (P = 0): tensors of the float32 path, where prepared; the float32 up-conv output (where act_split converts it)
                        {"concat", &concat, -1, 0, 0, 1}, {"pool", &pool, -1, 0, 1, 0}, {"upf", &upf, -1, 0, 0, 0}};
    for (const Row& r : rows) {
        if (base != r.name) continue;
        RFI_REQUIRE(base != "upin" || convt_planes, "debug_tensor: upin exists only with the transposed convs on the plane kernels");
        RFI_REQUIRE(!r.levels || (idx >= 1 && idx <= D && (int)r.levels->size() > D), "debug_tensor: level out of range");
        const int l = r.levels ? idx : D + 1;
        const int i = r.levels ? (*r.levels)[l] : r.one;
        const size_t Mr = base == "xin" ? pix(1) : pix(l + r.down);
        const int Cr = base == "xin" ? in_ch : feat << (l - 1 + r.wide);
        return r.P ? planes(i, Mr, Cr, r.P) : f32(i, Mr, Cr);
    }
    throw Error("debug_tensor: unknown tensor " + name);
}

void UNetModel::backward_planes(const float* x_dev, const uint8_t* labels_dev, int n, int h, int w) {
    (void)x_dev;
    const int D = depth, IB = i_bott;
    // every layer owns its dY plane tensor and the other side-stream inputs (forward planes, dconcat, raw conv outputs)
    // are not rewritten before side_join(): the main stream never has to wait for a weight gradient inside the pass
    side_bound = 0;
    const int64_t M1 = (int64_t)n * h * w;
    dbias_deferred = dbias_pool && !ctx->exchange_active();    // (bias gradients must be final before their bucket leaves)
    loss_backward(labels_dev, M1);
    int head_records = 0;
    {
        ConvBN& last = convs[IB + 2 + 2 * (D - 1) + 1];
        const bool hdefer = dbias_deferred && head_fin_deferred;
        // (the head always writes the float32 gA.1, and the bfloat16 one next to it where the decoder phase reads that)
        head_records = launch_head_bwd(ctx, flow(decY2[1]).ref(), M1, feat, last.scale(), last.shift(), params + head_w_off, out_ch,
                                       buf(dlogits), buf(gA[1]), hdefer ? dbias_pool + head_rec_off : buf(ws_red) + bn_bwd_ws_floats(M1, feat),
                                       grads + head_w_off, grads + head_b_off, act_slope, last.mean(), last.invstd(), buf(ws_red),
                                       flow(gAdec[1]).h, nullptr, !hdefer);
    }
    int up_records = 0;                           // BatchNorm-backward records a transposed conv's input-gradient kernel left for the layer below
    for (int l = 1; l <= D; ++l) {                // decoders, shallow to deep
        const int k = D - l;
        Shape s{n, h >> (l - 1), w >> (l - 1)};
        Shape sin{n, h >> l, w >> l};
        ConvBN& c1 = convs[IB + 2 + 2 * k];
        ConvBN& c2 = convs[IB + 2 + 2 * k + 1];
        UpConv& u = ups[k];
        const PlaneSeg a1 = pl[pA1d[l]].seg();
        // (with the transposed convs on the plane kernels the gradient arriving from decoder l - 1's is a bfloat16 tensor, the
        // BatchNorm-backward sums of c2 came out of that kernel's epilogue, and Y2 is a bfloat16 tensor)
        const int rec1 = backward_pconv_bn(this, c2, flow(gAdec[l]).ref(), flow(decY2[l]).ref(), &a1, 1, s, flow(gB[l]), pl[pdYa[l]],
                                           l == 1 ? head_records : up_records, &c1, flow(decY1[l]).ref());
        const PlaneSeg in2[2] = {pl[pUp[l]].seg(), pl[pSkip[l]].seg()};
        const FlowRef cat = flow(dconcat[l]);     // the gradient of [up | skip]
        backward_pconv_bn(this, c1, flow(gB[l]).ref(), flow(decY1[l]).ref(), in2, 2, s, cat, pl[pdYb[l]], rec1);
        ConvBN& prevBN = (l == D) ? convs[IB + 1] : convs[IB + 2 + 2 * (k - 1) + 1];
        // what the transposed conv read (with prevBN) and the gradient it sends there
        const FlowRef prevY = flow(l == D ? bottY2 : decY2[l + 1]), dprev = flow(l == D ? gBottA : gAdec[l + 1]);
        const bool udefer = dbias_deferred && u.cout % 4 == 0;
        if (convt_planes) {
            // ConvTranspose on the plane kernels: dUp = the first C channels of the bfloat16 [up | skip] gradient
            const PlaneSeg dUp{cat.h, cat.pstride, plane_chunks(u.cout)};
            launch_channel_sum(ctx, cat.ref(), (int64_t)s.N * s.H * s.W, u.cout, udefer ? dbias_pool + u.dbias_rec_off : buf(ws_red),
                               grads + u.b_off, !udefer);
            {
                SideScope side(this);
                launch_pwgrad(ctx, convt_pwgrad_args(u, dUp, pl[pUpIn[l]].seg(), sin));
                side.end();
            }
            PConvArgs a;                          // the input gradient: a 2x2 stride-2 contraction of dUp, bfloat16 out, with the
            a.x[0] = dUp; a.nseg = 1; a.P = 1;    // BatchNorm-backward sums of the layer below in the epilogue
            a.N = sin.N; a.H = sin.H; a.W = sin.W; a.Hin = s.H; a.Win = s.W;
            a.R = 2; a.S = 2; a.pad = 0;
            a.Cout = u.cin;
            a.wB = u.wBd;
            a.y16 = dprev.h; a.y_pstride = (int)dprev.pstride;
            a.Hout = sin.H; a.Wout = sin.W;
            a.algo_flops = 2.0 * sin.N * sin.H * sin.W * 4.0 * u.cin * u.cout;
            a.stats = reinterpret_cast<double*>(buf(ws_red));
            a.stats_max_records = (int)(bn_stats_ws_floats(u.cin) / ((size_t)u.cin * 4));
            a.bwd_y16 = prevY.h;
            a.bwd_yps = prevY.pstride;
            a.bwd_scale = prevBN.scale(); a.bwd_shift = prevBN.shift();
            a.bwd_mean = prevBN.mean(); a.bwd_invstd = prevBN.invstd();
            a.bwd_slope = act_slope;
            launch_pconv(ctx, a);
            up_records = a.stats_records;
        } else {
            // ConvTranspose: dUp = dconcat[..., 0:C]; the round-1 kernels on float32 tensors
            View dUp{cat.f, 2 * u.cout};
            launch_channel_sum(ctx, dUp, (int64_t)s.N * s.H * s.W, u.cout, udefer ? dbias_pool + u.dbias_rec_off : buf(ws_red), grads + u.b_off,
                               !udefer);
            convt_backward(u, dUp, View{prevY.f, u.cin}, bn_xf(prevBN), sin, dprev.f);
        }
        bucket_ready(u.w_off, l == 1 ? n_flat : ups[k + 1].w_off);      // decoder level l (+ head) is complete
    }
    {                                             // bottleneck
        Shape s{n, h >> D, w >> D};
        const PlaneSeg a1 = pl[pA1b].seg(), p4 = pl[pPool[D]].seg();
        const int rec1 = backward_pconv_bn(this, convs[IB + 1], flow(gBottA).ref(), flow(bottY2).ref(), &a1, 1, s, flow(gBottB), pl[pdYbottA],
                                           up_records, &convs[IB], flow(bottY1).ref());
        backward_pconv_bn(this, convs[IB], flow(gBottB).ref(), flow(bottY1).ref(), &p4, 1, s, flow(dpool[D]), pl[pdYbottB], rec1);
        bucket_ready(convs[IB].w_off, ups[0].w_off);
    }
    if (resnet_encoder) backward_resnet_planes(n, h, w);
    else for (int l = D; l >= 1; --l) {           // encoders, deep to shallow
        Shape s{n, h >> (l - 1), w >> (l - 1)};
        ConvBN& c1 = convs[2 * (l - 1)];
        ConvBN& c2 = convs[2 * (l - 1) + 1];
        const YRef dskip = skip_grad(l, c2.cout), Y2 = flow(encY2[l]).ref(), Y1 = flow(encY1[l]).ref();
        // (the max-pool backward always writes the float32 gA.l, and the bfloat16 one next to it where the mode reads that)
        const FlowRef dA = flow(gA[l]);
        const int have = launch_pool_bwd_merge_sums(ctx, Y2, s.N, s.H, s.W, c2.cout, c2.scale(), c2.shift(), c2.mean(), c2.invstd(), dskip,
                                                    flow(dpool[l]).ref(), buf(gA[l]), act_slope, buf(ws_red), dA.h);
        if (!have)
            launch_pool_bwd_merge(ctx, Y2, s.N, s.H, s.W, c2.cout, c2.scale(), c2.shift(), dskip, flow(dpool[l]).ref(), buf(gA[l]), act_slope,
                                  dA.h);
        const PlaneSeg a1 = pl[pA1e[l]].seg();
        const int rec1 = backward_pconv_bn(this, c2, dA.ref(), Y2, &a1, 1, s, flow(gB[l]), pl[pdYaE[l]], have, &c1, Y1);
        const PlaneSeg in = (l == 1 ? pl[pXin] : pl[pPool[l - 1]]).seg();
        backward_pconv_bn(this, c1, flow(gB[l]).ref(), Y1, &in, 1, s, l == 1 ? FlowRef() : flow(dpool[l - 1]), pl[pdYbE[l]], rec1);
        bucket_ready(c1.w_off, convs[2 * l].w_off);
    }
    if (dbias_deferred)
        launch_finish_channel_sums_batched(ctx, static_cast<const FinishSumDesc*>(dbias_descs), dbias_n, dbias_max_c);
    side_join();
    side_bound = 2;
}
