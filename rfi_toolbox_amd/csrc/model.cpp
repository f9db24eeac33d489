// U-Net graph (rfi_toolbox/models/unet.py:41-118) and the optimisation step
// (rfi_toolbox/scripts/train_model.py:139-154) orchestrated over the HIP kernels.
//
// Data layout in HBM
//   activations  NHWC fp32.  Per 3x3 conv only the RAW conv output Y (pre-BatchNorm) is kept;
//                consumers apply scale/shift/ReLU when they load it (InXform), so the activated
//                tensor is never written except where two consumers need it materialised:
//                the encoder output goes once, activated, into channels [C,2C) of the decoder's
//                concat buffer (the skip) and, pooled, into the next level's input.  ConvTranspose
//                writes channels [0,C) of the same concat buffer: torch.cat never happens.
//   parameters   one flat fp32 buffer (+ identical flat grad / Adam m / Adam v buffers) in forward
//                layer order, every tensor 16-byte aligned: conv weights [tap][cout][cin],
//                convT weights [a*2+b][cout][cin]; a second "dgrad layout" copy [tap'][cin][cout]
//                is rebuilt after each optimiser step.
//   Encoder blocks are evaluated ONCE; the reference evaluates them twice (unet.py:28), which
//   only shows in the BatchNorm running statistics (EMA applied twice, num_batches_tracked += 2).
#include "model.hpp"

#include <cmath>
#include <cstdlib>
#include <random>

using namespace rfi;

namespace rfi {

void DevBuf::ensure(rfi_ctx* c, size_t floats) {
    if (floats <= n && p) return;
    if (p) c->release(p);
    ctx = c;
    p = static_cast<float*>(c->alloc(floats * sizeof(float)));
    n = floats;
}
void DevBuf::free() {
    if (p && ctx) ctx->release(p);
    p = nullptr;
    n = 0;
}

}  // namespace rfi

rfi_model::~rfi_model() {
    if (!ctx) return;
    ctx->activate();
    for (auto& b : bufs) b.free();
    if (ws_pool) ctx->release(ws_pool);
    for (float* p : {params, grads, adam_m, adam_v, chan_pool, wd_pool, w3_pool, grad_acc})
        if (p) ctx->release(p);
    for (BatchTable* t : {&ws, &relayout, &x3}) t->release(ctx);
    if (d_sums) ctx->release(d_sums);
    if (d_scalars) ctx->release(d_scalars);
    if (wd_ready) (void)hipEventDestroy(wd_ready);
    if (lazy_ev) (void)hipEventDestroy(lazy_ev);
}

UNetModel::~UNetModel() {
    if (!ctx) return;
    ctx->activate();
    for (auto& b : pl) b.free();
    for (void* p : {(void*)wb_pool, (void*)dbias_pool, dbias_descs, (void*)rs_wpool, (void*)rs_cls_pool})
        if (p) ctx->release(p);
    wb.release(ctx);
}

// ------------------------------------------------------------------------------------ build
void UNetModel::build() {
    if (resnet_encoder) return build_resnet();
    RFI_REQUIRE(in_ch > 0 && out_ch > 0 && feat > 0, "UNet: channel counts must be positive");
    RFI_REQUIRE(depth >= 1 && depth <= 6, "UNet: depth must be in [1,6]");
    const int D = depth;
    i_bott = 2 * D;
    auto add = [&](const std::string& prefix, int conv_idx, int bn_idx, int cin, int cout, int ema, int lvl) {
        ConvBN c;
        c.conv_name = prefix + "." + std::to_string(conv_idx);
        c.bn_name = prefix + "." + std::to_string(bn_idx);
        c.cin = cin;
        // only the network input can be padded (its staging buffer is ours); inner layers read
        // tensors whose pixel stride is the true channel count
        c.cin_p = convs.empty() ? (int)align4((size_t)cin) : cin;
        c.cout = cout;
        c.ema_repeats = ema;
        c.level = lvl;
        add_conv(c);
    };
    int cin = in_ch;
    for (int l = 1; l <= D; ++l) {
        const int cout = feat << (l - 1);
        const std::string p = "encoder" + std::to_string(l) + ".conv.conv";
        add(p, 0, 1, cin, cout, 2, l);
        add(p, 3, 4, cout, cout, 2, l);
        cin = cout;
    }
    add("bottleneck.conv", 0, 1, cin, cin * 2, 1, D + 1);
    add("bottleneck.conv", 3, 4, cin * 2, cin * 2, 1, D + 1);
    cin *= 2;
    // decoder parameters come in forward order: up, conv1, conv2 per level
    for (int l = D; l >= 1; --l) {
        const int cout = feat << (l - 1);
        add_up("decoder" + std::to_string(l) + ".up", cin, cout);
        const std::string p = "decoder" + std::to_string(l) + ".conv.conv";
        add(p, 0, 1, cin, cout, 1, l);
        add(p, 3, 4, cout, cout, 1, l);
        cin = cout;
    }
    add_head("final_conv", feat);
    alloc_state();
    make_slots();
}

void UNetModel::make_slots() {
    const int D = depth;
    auto mk = [&](std::vector<int>& v) { v.assign(D + 1, -1); for (int l = 1; l <= D; ++l) v[l] = new_buf(); };
    auto mkf = [&](std::vector<FlowTensor>& v) { v.assign(D + 1, FlowTensor()); for (int l = 1; l <= D; ++l) v[l].f32 = new_buf(); };
    mkf(encY1); mkf(encY2); mk(concat); mk(pool); mkf(decY1); mkf(decY2);
    mkf(gA); mkf(gB); mkf(dconcat); mkf(dpool); mk(gAe); mk(gBe);
    make_bufs({&bottY1.f32, &bottY2.f32, &gBottA.f32, &gBottB.f32});
    make_plane_slots();
}

void UNetModel::set_planes(int P) {
    if (P == planesP) return;
    ctx->activate();
    RFI_CHECK_HIP(hipStreamSynchronize(ctx->main_stream));
    RFI_CHECK_HIP(hipStreamSynchronize(ctx->side_stream));
    for (auto& b : pl) b.free();                  // tensors and filter copies of the other P
    if (wb_pool) { ctx->release(wb_pool); wb_pool = nullptr; }
    wb.release(ctx);
    planesP = P;
    stale |= WEIGHT_DERIVED;                      // (another data flow reads other copies: every one is rebuilt)
    invalidate_shape();                           // (the flows own different tensors, and prepare_planes's table depends on the flow)
}

// ------------------------------------------------------------------------------------ prepare
void rfi_model::prepare(int n, int h, int w) {
    RFI_REQUIRE(n > 0 && h > 0 && w > 0, "forward: empty batch or image");
    join_pending_side();                          // (the last pass's weight gradients still read this model's tensors)
    if (ctx->stream != ctx->main_stream) {      // a side-stream launch threw last time: rejoin first
        ctx->stream = ctx->main_stream;
        RFI_CHECK_HIP(hipStreamSynchronize(ctx->side_stream));
        side_seq = 0;
    }
    if (side_seq != 0 || ctx->fork_ring_used != 0 || ctx->bucket_ev_used != 0 || pend_hi > pend_lo) {
        // the previous pass did not reach side_join / exchange_join (an exception mid-backward): drain every stream and
        // start from clean counters and event pools
        RFI_CHECK_HIP(hipStreamSynchronize(ctx->main_stream));
        RFI_CHECK_HIP(hipStreamSynchronize(ctx->side_stream));
        if (ctx->comm_stream) RFI_CHECK_HIP(hipStreamSynchronize(ctx->comm_stream));
        side_seq = 0;
        ctx->fork_ring_used = 0;
        ctx->bucket_ev_used = 0;
        pend_lo = pend_hi = 0;
    }
    if (n == pN && h == pH && w == pW) return;
    ctx->activate();
    prepare_shape(n, h, w);
    // what the entry points stage through, for M input pixels and Mout output pixels
    const size_t M = (size_t)n * h * w, Mout = M * out_scale * out_scale;
    const int cp = convs[0].cin_p;
    for (int i : {x_stage, x_stage2}) bufs[i].ensure(ctx, M * in_ch);
    bufs[x_pad].ensure(ctx, dense_head && cp != in_ch ? M * cp : 16);     // (network_input pads into it)
    for (int i : {logits, dlogits, out_stage}) bufs[i].ensure(ctx, dense_head ? Mout * out_ch : 16);
    bufs[lab_stage].ensure(ctx, dense_head ? (Mout + 3) / 4 + 4 : 16);
    // the workspaces: the needs every model has (gradient norm, loss), on top of what prepare_shape declared
    need_red(sumsq_ws_doubles(n_flat) * 2);
    if (dense_head) need_red(std::max({loss_ws_doubles(Mout), class_loss_ws_doubles(out_ch), masked_loss_ws_doubles(out_ch)}) * 2);
    bufs[ws_red].ensure(ctx, red_need + 16);
    bufs[ws_slab].ensure(ctx, slab_need + 16);
    pN = n; pH = h; pW = w;
}

void UNetModel::prepare_shape(int n, int h, int w) {
    const int div = 1 << depth;
    RFI_REQUIRE(h % div == 0 && w % div == 0,
                "forward: H and W must be multiples of 2^depth (" + std::to_string(div) +
                    "), as the reference's pool/up-conv/cat chain requires; got " +
                    std::to_string(h) + "x" + std::to_string(w));
    const int D = depth;
    for (int l = 1; l <= D; ++l) {
        const size_t M = (size_t)n * (h >> (l - 1)) * (w >> (l - 1));
        const size_t C = (size_t)feat << (l - 1);
        for (int i : {decY1[l].f32, decY2[l].f32, gA[l].f32, gB[l].f32}) bufs[i].ensure(ctx, M * C);
        if (!planesP && !resnet_encoder) for (int i : {gAe[l], gBe[l]}) bufs[i].ensure(ctx, M * C);   // (the encoder phase's own gradient tensors)
        if (!resnet_encoder) for (int i : {encY1[l].f32, encY2[l].f32}) bufs[i].ensure(ctx, M * C);     // (ResNet encoder: its own tensors, prepare_resnet)
        bufs[concat[l]].ensure(ctx, M * 2 * C);
        bufs[dconcat[l].f32].ensure(ctx, M * 2 * C);
        if (!resnet_encoder || l == D) {
            bufs[pool[l]].ensure(ctx, M / 4 * C);
            bufs[dpool[l].f32].ensure(ctx, M / 4 * C);
        }
    }
    {
        const size_t M = (size_t)n * (h >> D) * (w >> D);
        const size_t C = (size_t)feat << D;
        for (int i : {bottY1.f32, bottY2.f32, gBottA.f32, gBottB.f32}) bufs[i].ensure(ctx, M * C);
    }
    const size_t M1 = (size_t)n * h * w;
    bufs[probs].ensure(ctx, M1 * out_ch);          // (set_head_sigmoid: this model only)
    // workspaces
    size_t cmax = (size_t)feat << depth;
    need_red(bn_stats_ws_floats((int)cmax));
    need_red(bn_bwd_ws_floats(M1, (int)cmax));
    need_red(head_bwd_ws_floats(M1, feat, out_ch) + bn_bwd_ws_floats(M1, feat));   // (+ the BN-backward records head_bwd leaves)
    need_red(channel_sum_ws_floats(M1, (int)cmax));
    // wgrad slabs: the largest need over all layers, from the descriptors the backward passes build (model_resnet.cpp: a
    // stride-2 3x3 conv runs as its 2x2 form on the space-to-depth input, the 1x1 projection on a channel slice of that input)
    for (const ConvBN& c : convs) {
        const Shape s{n, h >> (c.level - 1), w >> (c.level - 1)};
        if (c.R == 1) need_slab(wgrad_same(View{nullptr, 4 * c.cin}, InXform{}, nullptr, s, 1, 0, c.cin, c.cout, nullptr));
        else if (c.stride == 2) need_slab(wgrad_same(View{nullptr, 4 * c.cin}, InXform{}, nullptr, s, 2, 1, 4 * c.cin, c.cout, nullptr));
        else need_slab(wgrad_same(View{nullptr, c.cin_p}, InXform{}, nullptr, s, 3, 1, c.cin_p, c.cout, nullptr));
    }
    for (int k = 0; k < D; ++k)                    // decoder level D - k: dUp is the first half of its concat gradient
        need_slab(convt_wgrad_args(ups[k], View{nullptr, 2 * ups[k].cout}, View{nullptr, ups[k].cin}, InXform{}, Shape{n, h >> (D - k), w >> (D - k)}));
    // per-layer regions for the partial sums of the conv-bias gradients + the table of the batched finisher
    // (the plane flows too: the plain U-Net's and the ResNet-encoder model's, whose encoder convs have no bias)
    if (!resnet_encoder || planesP) {
        if (dbias_pool) { ctx->release(dbias_pool); dbias_pool = nullptr; }
        if (dbias_descs) { ctx->release(dbias_descs); dbias_descs = nullptr; }
        size_t need = 0;
        std::vector<FinishSumDesc> hd;
        auto pixels = [&](const ConvBN& c) { return (int64_t)n * (h >> (c.level - 1)) * (w >> (c.level - 1)); };      // of its output
        for (ConvBN& c : convs) {
            c.dbias_rec_off = need;
            need += align4(channel_sum_ws_floats(pixels(c), c.cout)) + 4;
        }
        for (int k = 0; k < depth; ++k) {               // the transposed convs' bias gradients (decoder level l = D - k)
            const int l = depth - k;
            ups[k].dbias_rec_off = need;
            need += align4(channel_sum_ws_floats((int64_t)n * (h >> (l - 1)) * (w >> (l - 1)), ups[k].cout)) + 4;
        }
        head_rec_off = need;
        need += align4(head_bwd_ws_floats((int64_t)n * h * w, feat, out_ch)) + 4;
        dbias_pool = static_cast<float*>(ctx->alloc(need * sizeof(float)));
        dbias_max_c = 0;
        for (const ConvBN& c : convs) {
            if (!c.has_bias) continue;
            hd.push_back(FinishSumDesc{reinterpret_cast<const double*>(dbias_pool + c.dbias_rec_off), bn_bwd_apply_records(pixels(c), c.cout),
                                       (int64_t)c.cout, c.cout, grads + c.b_off});
            dbias_max_c = std::max(dbias_max_c, c.cout);
        }
        for (int k = 0; k < depth; ++k) {
            const int l = depth - k;
            const UpConv& u = ups[k];
            if (u.cout % 4) continue;                 // (launch_channel_sum keeps its own finish for such a layer)
            hd.push_back(FinishSumDesc{reinterpret_cast<const double*>(dbias_pool + u.dbias_rec_off),
                                       bn_bwd_apply_records((int64_t)n * (h >> (l - 1)) * (w >> (l - 1)), u.cout), (int64_t)u.cout, u.cout,
                                       grads + u.b_off});
            dbias_max_c = std::max(dbias_max_c, u.cout);
        }
        head_fin_deferred = feat % 4 == 0;
        if (head_fin_deferred) {                       // the head's dw (out_ch x feat) and db (out_ch), contiguous in every record
            const int recs = bn_bwd_apply_records((int64_t)n * h * w, feat);
            const int64_t stride = (int64_t)out_ch * feat + out_ch;
            const double* hp = reinterpret_cast<const double*>(dbias_pool + head_rec_off);
            hd.push_back(FinishSumDesc{hp, recs, stride, out_ch * feat, grads + head_w_off});
            hd.push_back(FinishSumDesc{hp + (size_t)out_ch * feat, recs, stride, out_ch, grads + head_b_off});
            dbias_max_c = std::max(dbias_max_c, out_ch * feat);
        }
        dbias_n = (int)hd.size();
        dbias_descs = ctx->upload_table(hd.data(), hd.size() * sizeof(FinishSumDesc));
    }
    if (planesP) prepare_planes(n, h, w);
    else if (resnet_encoder) prepare_resnet(n, h, w);
}

// ------------------------------------------------------------------------------------ derived filter copies
// the main stream waits for the side stream's half of a split rebuild
void rfi_model::wait_wd() {
    if (!wd_pending) return;
    RFI_CHECK_HIP(hipStreamWaitEvent(ctx->main_stream, wd_ready, 0));
    wd_pending = false;
}

// the side-stream half of the split rebuild, where sync_filters left it: dgrad layout + its B-operand images.  Called by the
// forward pass AFTER the first conv is enqueued (the stem is bound by its HBM writes: next to it the rebuild slowed it
// from 33 to 62 us; the convs that follow are matrix-bound)
void rfi_model::side_rebuild_wd() {
    if (!(stale & INPUT_GRAD_HALF)) return;
    if (!wd_ready) RFI_CHECK_HIP(hipEventCreateWithFlags(&wd_ready, hipEventDisableTiming));
    // the side stream waits for everything on main so far (the optimiser step); no end(): wd_ready marks this work, and the
    // scope puts the context's stream back
    SideScope side(this);
    rebuild_dgrad();
    refresh_ws_weights(Half::InputGrad);
    refresh_model_weights(Half::InputGrad);
    RFI_CHECK_HIP(hipEventRecord(wd_ready, ctx->side_stream));
    wd_pending = true;
    stale &= ~INPUT_GRAD_HALF;
}

void rfi_model::sync_filters(Half needed) {
    if (ws_P != ws_need()) stale |= WEIGHT_DERIVED;     // the images are another arithmetic's: its pool replaces them, every copy follows
    unsigned due = stale & (use_w3() ? WEIGHT_DERIVED : WEIGHT_DERIVED & ~RECORDS);
    if (!due) return;
    // Split rebuild (wd_split_ok): the forward pass needs the forward-direction copies only, so the dgrad layout and its
    // B-operand images are rebuilt on the SIDE stream (idle during the forward pass) under the first convs: their bits stay
    // set for side_rebuild_wd, and backward() waits for them (wait_wd).  The split decides before anything is rebuilt
    if (needed == Half::Forward && ctx->overlap && !ctx->profiling && ctx->stream == ctx->main_stream && wd_split_ok())
        due &= ~INPUT_GRAD_HALF;
    else
        wait_wd();                    // (an earlier side-stream half may still be writing what is rebuilt here)
    if (due & DGRAD) rebuild_dgrad();
    if (due & (IMAGES_FWD | IMAGES_BWD)) refresh_ws_weights(half_of(due, IMAGES_FWD, IMAGES_BWD));
    if (due & RECORDS) rebuild_records();
    if (due & (MODEL_FWD | MODEL_BWD)) refresh_model_weights(half_of(due, MODEL_FWD, MODEL_BWD));
    stale &= ~due;
}

void rfi_model::rebuild_dgrad() {
    if (!relayout.descs) {
        std::vector<RelayoutDesc> h;
        for (auto& c : convs) {
            h.push_back({(int64_t)c.w_off, (int64_t)(c.wd - wd_pool), c.R * c.R, c.cout, c.cin_p, 1});
            relayout.bytes += 8.0 * c.R * c.R * c.cout * c.cin_p;
        }
        for (auto& u : ups) {
            h.push_back({(int64_t)u.w_off, (int64_t)(u.wd - wd_pool), 4, u.cout, u.cin, 0});
            relayout.bytes += 8.0 * 4 * u.cout * u.cin;
        }
        relayout.n = (int)h.size();
        relayout_tiles = relayout_assign_tiles(h.data(), relayout.n);
        relayout.descs = ctx->upload_table(h.data(), h.size() * sizeof(RelayoutDesc));
    }
    launch_weight_to_dgrad_batched(ctx, static_cast<const RelayoutDesc*>(relayout.descs), relayout.n, params, wd_pool,
                                   relayout.bytes, relayout_tiles);
}

// pre-split records of both layouts of the conv-like layers (the round-2 kernels read them as is)
void rfi_model::rebuild_records() {
    if (!w3_pool) {
        size_t need = 0;
        for (auto& c : convs) need += weights_x3_floats(c.R * c.R, c.cout, c.cin_p) + weights_x3_floats(c.R * c.R, c.cin_p, c.cout);
        for (auto& u : ups) need += 2 * weights_x3_floats(4, u.cout, u.cin) + weights_x3_floats(4, u.cin, u.cout);
        w3_pool = static_cast<float*>(ctx->alloc((need + 64) * sizeof(float)));
        size_t o = 0;
        for (auto& c : convs) {
            c.w3 = w3_pool + o; o += weights_x3_floats(c.R * c.R, c.cout, c.cin_p);
            c.wd3 = w3_pool + o; o += weights_x3_floats(c.R * c.R, c.cin_p, c.cout);
        }
        for (auto& u : ups) {
            u.w3 = w3_pool + o; o += weights_x3_floats(4, u.cout, u.cin);
            u.wd3 = w3_pool + o; o += weights_x3_floats(4, u.cin, u.cout);
        }
    }
    // layers whose filters the wave-specialised kernels read (ws_by_w) need no records: launch_conv drops
    // ConvArgs::w3 for them, and a shape those kernels decline (maps under 8 x 8) gets a temporary split copy
    const RecordKey key = record_key();
    if (x3.descs && !(x3_key == key)) x3.release(ctx);
    if (!x3.descs) {
        x3_key = key;
        std::vector<X3Desc> h;
        const bool skip_ws = x3_skips_ws_layers && ws_P == 3;
        x3_reads_wd = false;
        x3_skipped.clear();
        // a layer is left out only if the wave-specialised kernels cannot decline it at the prepared shape: its maps are at
        // least 8 x 8 (conv_ws_eligible) -- a declined launch on a missing record would allocate a temporary copy and
        // synchronise the stream inside launch_conv.  (pH == 0: nothing prepared yet, keep everything)
        auto add = [&](const float* src, float* dst, int taps, int cout, int cin, int level = 0) {
            const bool small_map = pH == 0 || (level > 0 && ((pH >> (level - 1)) < 8 || (pW >> (level - 1)) < 8));
            if (skip_ws && ws_by_w.count(src) && !small_map) { x3_skipped.insert(src); return; }
            if (src < params || src >= params + n_flat) x3_reads_wd = true;
            h.push_back(X3Desc{src, dst, (int64_t)taps * cout, cin, (cin + 15) / 16});
            x3.bytes += (double)taps * cout * cin * 4 + (double)weights_x3_floats(taps, cout, cin) * 4;
        };
        for (auto& c : convs) {
            add(params + c.w_off, c.w3, c.R * c.R, c.cout, c.cin_p, c.level);
            add(c.wd, c.wd3, c.R * c.R, c.cin_p, c.cout, c.level);
        }
        for (auto& u : ups) {
            add(params + u.w_off, u.w3, 4, u.cout, u.cin);
            add(u.wd, u.wd3, 4, u.cin, u.cout);
        }
        x3.n = (int)h.size();
        x3.descs = ctx->upload_table(h.data(), h.size() * sizeof(X3Desc));
    }
    if (x3.n) launch_weights_to_x3_batched(ctx, static_cast<const X3Desc*>(x3.descs), x3.n, x3.bytes);
}

// 2 x 2 form of a stride-2 3x3 filter on the space-to-depth input, its dgrad layout and (3 x bf16 arithmetic) the records of both
void rfi_model::refresh_s2d_forms(ConvBN& c) {
    launch_w_s2d(ctx, params + c.w_off, c.cout, c.cin, c.ws2d, true);
    launch_weight_to_dgrad(ctx, c.ws2d, 4, c.cout, 4 * c.cin, 1, c.wds2d);
    if (use_w3()) {
        launch_weights_to_x3(ctx, c.ws2d, 4, c.cout, 4 * c.cin, c.ws2d3);
        launch_weights_to_x3(ctx, c.wds2d, 4, 4 * c.cin, c.cout, c.wds2d3);
    }
}

// plain U-Net, float32 tensors: when the wave-specialised copies of both directions are in use (and the pre-split records
// do not read the dgrad layouts: the list in hand says so only while it is the prepared shape's -- on smaller maps the next
// rebuild_records lists layers it left out, and would split stale dgrad layouts).  The plane flows: the forward pass reads the forward-direction images only, nothing but
// the input-gradient kernels reads the dgrad layouts -- unless pre-split records of them are in use
bool UNetModel::wd_split_ok() const {
    if (planesP) return wb_pool && wb.n_fwd > 0 && !use_w3() && training;
    return !resnet_encoder && ws_need() != 0 && ws_pool && ws_P == ws_need() && ws.n_fwd > 0 &&
           (!use_w3() || (x3.descs && !x3_reads_wd && x3_key == record_key()));
}

void UNetModel::refresh_model_weights(Half half) {
    if (planesP) refresh_plane_weights(half);                    // B-operand-order filters of the plane kernels
    else if (resnet_encoder) refresh_resnet_weights();           // 2x2 forms of the stride-2 filters
}

// filters of every 3x3 stride-1 layer in MFMA B-operand order with three planes (conv_ws.hip), both directions, rebuilt
// with the other derived copies after each optimiser step by ONE batched launch.  Callers find them by the layer's
// float32 filter pointer (set_filters -> ws_set looks up ConvArgs::w)
void rfi_model::refresh_ws_weights(Half half) {
    const int P = ws_need();
    if (P != ws_P) {                  // another arithmetic: its copies have another size
        if (ws_pool) { ctx->release(ws_pool); ws_pool = nullptr; }
        ws.release(ctx);
        ws_by_w.clear();
        ws_P = P;
    }
    if (P == 0) return;
    if (!ws_pool) {
        // conv_ws: 3x3 stride-1 layers with channels % 16 == 0; gemm_ws (P = 3): the transposed convs
        auto conv_f = [&](const ConvBN& c) { return c.R == 3 && c.stride == 1 && c.cin_p % 16 == 0; };
        auto conv_d = [&](const ConvBN& c) { return c.R == 3 && c.stride == 1 && c.cout % 16 == 0; };
        auto up_ok = [&](const UpConv& u) { return P == 3 && u.cin % 16 == 0 && u.cout % 32 == 0; };
        // gemm_ws also runs the plain 1x1 stride-1 convs (the Bottleneck and pyramid convs of the detection backbone) as GEMMs
        auto one_ok = [&](const ConvBN& c) { return P == 3 && c.R == 1 && c.stride == 1 && c.cin_p % 32 == 0 && c.cout % 32 == 0; };
        size_t need = 0;
        for (const ConvBN& c : convs) {
            if (conv_f(c)) need += wb_elems(9, c.cout, c.cin_p, 0, P) + 32;
            if (conv_d(c)) need += wb_elems(9, c.cin_p, c.cout, 0, P) + 32;
            if (one_ok(c)) need += wb_elems(1, c.cout, c.cin_p, 0, P) + wb_elems(1, c.cin_p, c.cout, 0, P) + 64;
        }
        for (const UpConv& u : ups)
            if (up_ok(u)) need += wb_elems(1, 4 * u.cout, u.cin, 0, P) + wb_elems(4, u.cin, u.cout, 0, P) + 64;
        if (need == 0) return;
        ws_pool = static_cast<bf16_t*>(ctx->alloc(need * 2));
        RFI_CHECK_HIP(hipMemsetAsync(ws_pool, 0, need * 2, ctx->stream));
        // forward-direction images first (sources in `params`), then the input-gradient direction (sources in wd_pool): the
        // two halves can be rebuilt by separate launches (a split rebuild puts the second on the side stream)
        std::vector<WBDesc> hd, hdg;
        size_t o = 0;
        double bytes_bwd = 0;
        // the image of `taps` filters [cout][cin] at `src`: the next region of the pool (+ its 32-element tail), one descriptor
        auto image = [&](std::vector<WBDesc>& table, double& bytes, const float* src, int taps, int cout, int cin) {
            bf16_t* dst = ws_pool + o;
            const size_t e = wb_elems(taps, cout, cin, 0, P);
            o += e + 32;
            table.push_back(WBDesc{src, dst, taps, cout, cin, {cin, 0}, P});
            ws_by_w[src] = dst;
            bytes += 2.0 * e + 4.0 * taps * cout * cin;
            return dst;
        };
        for (ConvBN& c : convs) {
            if (conv_f(c)) c.ws3f = image(hd, ws.bytes_fwd, params + c.w_off, 9, c.cout, c.cin_p);
            if (conv_d(c)) c.ws3d = image(hdg, bytes_bwd, c.wd, 9, c.cin_p, c.cout);
            if (one_ok(c)) {
                image(hd, ws.bytes_fwd, params + c.w_off, 1, c.cout, c.cin_p);
                image(hdg, bytes_bwd, c.wd, 1, c.cin_p, c.cout);
            }
        }
        // transposed convs (gemm_ws.hip): forward = ONE tap of 4 cout channels ([4][cout][cin] IS [4 cout][cin]); input
        // gradient = four taps of [cin][cout]
        for (UpConv& u : ups) {
            if (!up_ok(u)) continue;
            image(hd, ws.bytes_fwd, params + u.w_off, 1, 4 * u.cout, u.cin);
            image(hdg, bytes_bwd, u.wd, 4, u.cin, u.cout);
        }
        ws.n_fwd = (int)hd.size();
        ws.bytes = ws.bytes_fwd + bytes_bwd;
        hd.insert(hd.end(), hdg.begin(), hdg.end());
        ws.n = (int)hd.size();
        ws.descs = ctx->upload_table(hd.data(), hd.size() * sizeof(WBDesc));
    }
    ws.launch(ctx, half);
}

// ------------------------------------------------------------------------------------ shared launches
ConvArgs rfi_model::conv_same(View x, InXform xf, Shape s, int R, int pad, int cin, int cout, const float* w, const float* w3,
                              const float* bias, float* y) const {
    ConvArgs a;
    a.x = x;
    a.N = s.N; a.H = s.H; a.W = s.W; a.Hin = s.H; a.Win = s.W;
    a.Cin = cin; a.Cout = cout;
    set_filters(a, w, w3);            // (null w3: the kernel launcher splits a temporary copy)
    a.bias = bias;
    a.y = MutView{y, cout};
    a.Hout = s.H; a.Wout = s.W;
    a.R = R; a.S = 1; a.pad = pad;
    a.xf = xf;
    return a;
}

WgradArgs rfi_model::wgrad_same(View x, InXform xf_x, const float* dy, Shape s, int R, int pad, int cin, int cout,
                                float* dw) const {
    WgradArgs wa;
    wa.xop = x;
    wa.yop = View{dy, cout};
    wa.xf_x = xf_x;
    wa.N = s.N; wa.H = s.H; wa.W = s.W; wa.Hx = s.H; wa.Wx = s.W;
    wa.Cx = cin; wa.Cy = cout;
    wa.R = R; wa.S = 1; wa.pad = pad;
    wa.dw = dw;
    wa.tap_stride = (int64_t)cin * cout;
    wa.sy = cin; wa.sx = 1;
    set_wgrad(wa);
    return wa;
}

void rfi_model::conv_bn(ConvBN& c, View in, InXform xf, Shape s, const float* w, const float* w3, int R, int pad, int cin,
                        float* Y, bool train, double flops) {
    ConvArgs a = conv_same(in, xf, s, R, pad, cin, c.cout, w, w3, c.has_bias ? params + c.b_off : nullptr, Y);
    a.algo_flops = flops;
    float* ws = buf(ws_red);
    if (train) {            // batch statistics come out of the conv epilogue (no second pass over Y)
        a.stats = reinterpret_cast<double*>(ws);
        a.stats_max_records = (int)(bn_stats_ws_floats(c.cout) / ((size_t)c.cout * 4));
    }
    launch_conv(ctx, a);
    bn_tail(c, Y, (int64_t)s.N * s.H * s.W, train, a.stats_records);
}

void rfi_model::bn_tail(ConvBN& c, const float* Y, int64_t M, bool train, int records) {
    float* ws = buf(ws_red);
    if (train) {
        if (records == 0) launch_bn_stats(ctx, Y, M, c.cout, ws);   // (a kernel without the statistics epilogue)
        launch_bn_finalize(ctx, ws, M, c.cout, params + c.g_off, params + c.be_off, c.running_mean(), c.running_var(),
                           c.ema_repeats, c.mean(), c.invstd(), c.scale(), c.shift(), nullptr, records);
        c.nbt += c.ema_repeats;
    } else {
        launch_bn_eval_coeffs(ctx, c.cout, params + c.g_off, params + c.be_off, c.running_mean(), c.running_var(),
                              c.scale(), c.shift());
    }
}

// ConvTranspose2d(k2, s2) forward: ONE 1x1 launch over the input grid whose four filter groups (zgroups) land on the four
// pixels of each 2 x 2 output block
ConvArgs rfi_model::convt_args(const UpConv& u, View x, InXform xf, Shape s) const {
    ConvArgs a;
    a.x = x;
    a.N = s.N; a.H = s.H; a.W = s.W; a.Hin = s.H; a.Win = s.W;
    a.Cin = u.cin; a.Cout = u.cout;
    set_filters(a, params + u.w_off, u.w3);
    a.bias = params + u.b_off;
    a.Hout = 2 * s.H; a.Wout = 2 * s.W;
    a.osy = 2; a.osx = 2;
    a.R = 1; a.S = 1; a.pad = 0;
    a.zgroups = 4;
    a.xf = xf;
    return a;
}

WgradArgs rfi_model::convt_wgrad_args(const UpConv& u, View dup, View x, InXform xf, Shape s) const {
    WgradArgs wa;
    wa.xop = dup;
    wa.yop = x;
    wa.xf_y = xf;
    wa.N = s.N; wa.H = s.H; wa.W = s.W; wa.Hx = 2 * s.H; wa.Wx = 2 * s.W;
    wa.Cx = u.cout; wa.Cy = u.cin;
    wa.R = 2; wa.S = 2; wa.pad = 0;
    wa.dw = grads + u.w_off;
    wa.tap_stride = (int64_t)u.cin * u.cout;
    wa.sy = 1; wa.sx = u.cin;          // -> [tap][cout][cin]
    set_wgrad(wa);
    return wa;
}

void rfi_model::convt_backward(const UpConv& u, View dup, View x, InXform xf, Shape s, float* dx) {
    wgrad_on_side(convt_wgrad_args(u, dup, x, xf, s), nullptr);
    ConvArgs a;
    a.x = dup;
    a.N = s.N; a.H = s.H; a.W = s.W; a.Hin = 2 * s.H; a.Win = 2 * s.W;
    a.Cin = u.cout; a.Cout = u.cin;
    set_filters(a, u.wd, u.wd3);
    a.y = MutView{dx, u.cin};
    a.Hout = s.H; a.Wout = s.W;
    a.R = 2; a.S = 2; a.pad = 0;
    launch_conv(ctx, a);
}

// ------------------------------------------------------------------------------------ forward

// the first conv sees the input with its channels zero-padded to a multiple of 4 (16-byte pixels),
// so the 3-channel stem runs on the same MFMA kernels as every other layer
rfi::View rfi_model::network_input(const float* x_dev, int n, int h, int w) {
    const int cp = convs[0].cin_p;
    if (cp != in_ch) launch_pad_channels(ctx, x_dev, (int64_t)n * h * w, in_ch, cp, buf(x_pad));
    return padded_input(x_dev);
}

void rfi_model::forward(const float* x_dev, int n, int h, int w, bool train_mode) {
    prepare(n, h, w);
    if (model_copies_every_pass) stale |= MODEL_FWD | MODEL_BWD;
    sync_filters(Half::Forward);      // the derived filter copies follow the parameters
    forward_pass(x_dev, n, h, w, train_mode);
}

void UNetModel::forward_pass(const float* x_dev, int n, int h, int w, bool train_mode) {
    if (planesP) return forward_planes(x_dev, n, h, w, train_mode);
    const int D = depth, IB = i_bott;
    auto run_conv_bn = [&](ConvBN& c, View in, InXform xf, Shape s, float* Y) {
        conv_bn(c, in, xf, s, params + c.w_off, c.w3, 3, 1, c.cin_p, Y, train_mode, 2.0 * s.N * s.H * s.W * 9.0 * c.cin * c.cout);
    };
    View cur = network_input(x_dev, n, h, w);
    if (resnet_encoder) cur = forward_resnet_encoder(cur, n, h, w, train_mode);
    else for (int l = 1; l <= D; ++l) {
        Shape s{n, h >> (l - 1), w >> (l - 1)};
        ConvBN& c1 = convs[2 * (l - 1)];
        ConvBN& c2 = convs[2 * (l - 1) + 1];
        run_conv_bn(c1, cur, InXform{}, s, buf(encY1[l]));
        if (l == 1) side_rebuild_wd();
        run_conv_bn(c2, View{buf(encY1[l]), c1.cout}, bn_xf(c1), s, buf(encY2[l]));
        // one pass writes the pooled tensor and the skip (the activated output in the decoder's concat buffer).  Writing the
        // skip on the side stream under the next level's convs measured slower: 6.69 against 6.64 ms per step (round 4) --
        // the second read of Y and the skip write next to the convs cost them more than the 45 us the main stream saves
        launch_bn_relu_pool(ctx, buf(encY2[l]), s.N, s.H, s.W, c2.cout, c2.scale(), c2.shift(),
                            MutView{buf(concat[l]) + c2.cout, 2 * c2.cout}, buf(pool[l]), act_slope);
        cur = View{buf(pool[l]), c2.cout};
    }
    {
        Shape s{n, h >> D, w >> D};
        ConvBN& c1 = convs[IB];
        ConvBN& c2 = convs[IB + 1];
        run_conv_bn(c1, cur, InXform{}, s, buf(bottY1));
        run_conv_bn(c2, View{buf(bottY1), c1.cout}, bn_xf(c1), s, buf(bottY2));
    }
    const float* prevY = buf(bottY2);
    ConvBN* prevBN = &convs[IB + 1];
    for (int l = D; l >= 1; --l) {
        const int k = D - l;
        UpConv& u = ups[k];
        Shape sin{n, h >> l, w >> l};
        Shape s{n, h >> (l - 1), w >> (l - 1)};
        ConvArgs a = convt_args(u, View{prevY, u.cin}, bn_xf(*prevBN), sin);
        a.y = MutView{buf(concat[l]), 2 * u.cout};
        launch_conv(ctx, a);
        ConvBN& c1 = convs[IB + 2 + 2 * k];
        ConvBN& c2 = convs[IB + 2 + 2 * k + 1];
        run_conv_bn(c1, View{buf(concat[l]), 2 * u.cout}, InXform{}, s, buf(decY1[l]));
        run_conv_bn(c2, View{buf(decY1[l]), c1.cout}, bn_xf(c1), s, buf(decY2[l]));
        prevY = buf(decY2[l]);
        prevBN = &c2;
    }
    const int64_t M1 = (int64_t)n * h * w;
    launch_head_fwd(ctx, prevY, M1, feat, prevBN->scale(), prevBN->shift(), params + head_w_off,
                    params + head_b_off, out_ch, buf(logits), act_slope);
    if (head_sigmoid) launch_sigmoid_fwd(ctx, buf(logits), M1 * out_ch, buf(probs));
}

void rfi_model::loss_forward(const uint8_t* labels_dev, int n, int h, int w) {
    const int64_t cnt = (int64_t)n * h * w * out_scale * out_scale;
    if (masked_loss()) {          // (the setters admit the plain U-Net without the sigmoid head only)
        RFI_REQUIRE(label_mode != RFI_LABELS_MAP || out_ch == 1, "loss: the reference's BCE+dice step is defined for out_channels == 1");
        launch_masked_loss_reduce(ctx, buf(logits), labels_dev, cnt, out_ch, loss_kind, focal_alpha, focal_gamma,
                                  label_mode == RFI_LABELS_MAP, ignore_on, weights_on ? pos_weight : nullptr,
                                  reinterpret_cast<double*>(buf(ws_red)), class_sums(), d_scalars);
        return;
    }
    if (label_mode == RFI_LABELS_CLASS_BITS) {
        launch_class_loss_reduce(ctx, buf(logits), labels_dev, cnt, out_ch, loss_kind, focal_alpha, focal_gamma,
                                 reinterpret_cast<double*>(buf(ws_red)), class_sums(), d_scalars);
        return;
    }
    RFI_REQUIRE(out_ch == 1, "loss: the reference's BCE+dice step is defined for out_channels == 1");
    // UNetOverfit: BCE-with-logits + dice are applied to the model OUTPUT, i.e. to sigmoid(logits)
    if (loss_kind == 1) {
        launch_focal_reduce(ctx, buf(head_sigmoid ? probs : logits), labels_dev, cnt, focal_alpha, focal_gamma,
                            reinterpret_cast<double*>(buf(ws_red)), d_scalars);
        return;
    }
    launch_loss_reduce(ctx, buf(head_sigmoid ? probs : logits), labels_dev, cnt,
                       reinterpret_cast<double*>(buf(ws_red)), d_sums, d_scalars);
}

void rfi_model::loss_backward(const uint8_t* labels_dev, int64_t pixels) {
    if (masked_loss())
        return launch_masked_loss_bwd(ctx, buf(logits), labels_dev, pixels, out_ch, loss_kind, focal_alpha, focal_gamma,
                                      label_mode == RFI_LABELS_MAP, ignore_on, weights_on ? pos_weight : nullptr, class_sums(),
                                      buf(dlogits));
    if (label_mode == RFI_LABELS_CLASS_BITS)
        return launch_class_loss_bwd(ctx, buf(logits), labels_dev, pixels, out_ch, loss_kind, focal_alpha, focal_gamma, class_sums(),
                                     buf(dlogits));
    if (loss_kind == 1)
        launch_focal_bwd(ctx, buf(head_sigmoid ? probs : logits), labels_dev, pixels, focal_alpha, focal_gamma, buf(dlogits));
    else
        launch_loss_bwd(ctx, buf(head_sigmoid ? probs : logits), labels_dev, pixels, d_sums, buf(dlogits));
    if (head_sigmoid) launch_sigmoid_bwd(ctx, buf(probs), pixels * out_ch, buf(dlogits));
}

// ------------------------------------------------------------------------------------ backward
// Weight-gradient GEMMs have no consumer before the optimiser step, so they run on a SIDE stream
// while the main stream carries the dependent chain (BN backward -> dgrad -> next layer's BN
// backward ...).  The memory-bound BN / pooling / slab-reduce kernels then share the chip with an
// MFMA-bound kernel instead of running alone, and the one-wave-per-SIMD wgrad kernel gets co-resident
// waves.  Ordering: side waits on an event recorded after the producer of dY; the main stream may
// run at most 2 side launches ahead (gA/gB of a decoder level are rewritten by the encoder phase
// no sooner than 3 layers later); all side work is joined before clip+Adam / the all-reduce.
void rfi_model::side_begin() {
    if (!ctx->overlap) return;
    RFI_CHECK_HIP(hipEventRecord(ctx->fork_ev, ctx->main_stream));
    RFI_CHECK_HIP(hipStreamWaitEvent(ctx->side_stream, ctx->fork_ev, 0));
    ctx->stream = ctx->side_stream;
}
hipEvent_t rfi_model::next_fork_event() {
    static const bool off = getenv("RFI_NO_STOP_EVENTS") != nullptr;        // (bench.py's fallback: event-record packets instead)
    if (!ctx->overlap || off) return nullptr;
    if (ctx->fork_ring_used == ctx->fork_ring.size()) {
        hipEvent_t e;
        RFI_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->fork_ring.push_back(e);
    }
    return ctx->fork_ring[ctx->fork_ring_used++];
}
void rfi_model::side_begin_after(hipEvent_t producer_done) {
    if (!producer_done) return side_begin();
    if (!ctx->overlap) return;
    RFI_CHECK_HIP(hipStreamWaitEvent(ctx->side_stream, producer_done, 0));
    ctx->stream = ctx->side_stream;
}
void rfi_model::side_end() {
    if (!ctx->overlap) return;
    const int ring = (int)ctx->side_done.size();
    RFI_CHECK_HIP(hipEventRecord(ctx->side_done[side_seq % ring], ctx->side_stream));
    ctx->stream = ctx->main_stream;
    if (side_bound > 0 && side_seq >= side_bound)
        RFI_CHECK_HIP(hipStreamWaitEvent(ctx->main_stream, ctx->side_done[(side_seq - side_bound) % ring], 0));
    ++side_seq;
}
void rfi_model::side_join_lazy() {
    if (exchange_in_backward && ctx->exchange_active()) return side_join();      // (a bucket may leave right behind this pass)
    if (!ctx->overlap || side_seq == 0) return;
    if (!lazy_ev) RFI_CHECK_HIP(hipEventCreateWithFlags(&lazy_ev, hipEventDisableTiming));
    RFI_CHECK_HIP(hipEventRecord(lazy_ev, ctx->side_stream));
    lazy_pending = true;
    side_seq = 0;
}
void rfi_model::join_pending_side() {
    if (!lazy_pending) return;
    RFI_CHECK_HIP(hipStreamWaitEvent(ctx->main_stream, lazy_ev, 0));
    lazy_pending = false;
}
void rfi_model::side_join() {
    if (!ctx->overlap || side_seq == 0) return;
    const int ring = (int)ctx->side_done.size();
    RFI_CHECK_HIP(hipStreamWaitEvent(ctx->main_stream, ctx->side_done[(side_seq - 1) % ring], 0));
    side_seq = 0;
    ctx->fork_ring_used = 0;                      // (every wait on these events has been passed)
}

namespace rfi { void comm_bucket_allreduce(rfi_ctx* ctx, float* dptr, int64_t count); }

static hipEvent_t bucket_event(rfi_ctx* ctx) {
    if (ctx->bucket_ev_used == ctx->bucket_ev.size()) {
        hipEvent_t e;
        RFI_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->bucket_ev.push_back(e);
    }
    return ctx->bucket_ev[ctx->bucket_ev_used++];
}
// Buckets arrive in the order the backward pass completes them (decreasing offsets).  Small ones are merged with
// their successors until RFI_BUCKET_MIN_FLOATS (default 2^20 = 4 MB) have accumulated -- a sub-megabyte all-reduce is
// bound by latency, not by the links -- and the last call (lo == 0) flushes what is left.  RFI_NO_BUCKETS=1: nothing
// leaves during the pass; exchange_join sends the whole buffer in one all-reduce (the fallback if the overlapped
// exchange misbehaves on a new communicator).
void rfi_model::bucket_ready(size_t lo, size_t hi) {
    if (!exchange_in_backward || !ctx->exchange_active() || hi <= lo) return;
    static const bool no_buckets = getenv("RFI_NO_BUCKETS") != nullptr;
    const char* mf = getenv("RFI_BUCKET_MIN_FLOATS");              // (read per call: tests switch it inside one process)
    const size_t min_floats = mf ? (size_t)atoll(mf) : (size_t)1 << 20;
    if (pend_hi > pend_lo) {
        RFI_REQUIRE(hi == pend_lo || lo == pend_hi, "bucket_ready: buckets must be adjacent");
        pend_lo = std::min(pend_lo, lo);
        pend_hi = std::max(pend_hi, hi);
    } else {
        pend_lo = lo;
        pend_hi = hi;
    }
    if (no_buckets) return;                       // (exchange_join flushes)
    if (pend_hi - pend_lo < min_floats && pend_lo != 0) return;
    flush_bucket();
}
void rfi_model::flush_bucket() {
    if (pend_hi <= pend_lo) return;
    const size_t lo = pend_lo, hi = pend_hi;
    pend_lo = pend_hi = 0;
    hipEvent_t em = bucket_event(ctx);
    RFI_CHECK_HIP(hipEventRecord(em, ctx->main_stream));
    RFI_CHECK_HIP(hipStreamWaitEvent(ctx->comm_stream, em, 0));
    if (ctx->overlap) {                           // weight gradients and their slab reductions run on the side stream
        hipEvent_t es = bucket_event(ctx);
        RFI_CHECK_HIP(hipEventRecord(es, ctx->side_stream));
        RFI_CHECK_HIP(hipStreamWaitEvent(ctx->comm_stream, es, 0));
    }
    comm_bucket_allreduce(ctx, grads + lo, (int64_t)(hi - lo));
}
void rfi_model::exchange_join() {
    if (!ctx->exchange_active()) return;
    flush_bucket();                               // (RFI_NO_BUCKETS, or a model whose last bucket does not start at 0)
    hipEvent_t e = bucket_event(ctx);
    RFI_CHECK_HIP(hipEventRecord(e, ctx->comm_stream));
    RFI_CHECK_HIP(hipStreamWaitEvent(ctx->main_stream, e, 0));
    ctx->bucket_ev_used = 0;                      // the pool is reused by the next step
}

namespace {

// given dA (grad w.r.t. the ACTIVATED output of conv c, overwritten with dY), produce dW/db/dgamma/
// dbeta into the grad buffer and, if dx != null, the gradient w.r.t. the conv's (activated) input.
// `have_records` > 0: the BatchNorm-backward sums of this layer already sit in the workspace (the kernel that
// produced dA folded them into its own pass).
void backward_conv_bn(UNetModel* m, ConvBN& c, float* dA, const float* Y, View in, InXform in_xf,
                      Shape s, float* dx, int have_records,
                      const float* head_dl = nullptr, const float* head_w = nullptr) {
    rfi_ctx* ctx = m->ctx;
    const int64_t M = (int64_t)s.N * s.H * s.W;
    float* ws = m->buf(m->ws_red);
    if (have_records > 0)
        launch_bn_bwd_finalize_records(ctx, ws, have_records, M, c.cout, c.c1(), c.c2(), m->grads + c.g_off,
                                       m->grads + c.be_off);
    else
        launch_bn_bwd_reduce(ctx, dA, Y, M, c.cout, c.scale(), c.shift(), c.mean(), c.invstd(), ws, c.c1(),
                             c.c2(), m->grads + c.g_off, m->grads + c.be_off, m->act_slope);
    // the weight gradient is enqueued BEHIND the input-gradient conv of the same layer (the side stream waits for it): two
    // matrix-core kernels sharing the chip finish no sooner than one after the other, but a weight gradient that runs next
    // to the following layer's BatchNorm-backward passes (memory-bound) hides them.
    // A kernel that carries a completion signal leaves a ~5 us bubble behind it on its stream: only the kernel the side stream
    // actually waits for gets one
    const hipEvent_t dy_done = dx ? nullptr : m->next_fork_event();      // completes with the kernel that writes dY (over dA)
    // (dbias_deferred: the partial sums of the conv-bias gradient stay in the layer's own region; backward() finishes every
    // layer's in one launch at the end of the pass)
    launch_bn_bwd_apply(ctx, dA, Y, M, c.cout, c.scale(), c.shift(), c.mean(), c.invstd(),
                        m->params + c.g_off, c.c1(), c.c2(), m->dbias_deferred ? m->dbias_pool + c.dbias_rec_off : ws,
                        m->grads + c.b_off, m->act_slope, nullptr, 0, 0, dy_done, !m->dbias_deferred, head_dl, head_w);
    WgradArgs wa = m->wgrad_same(in, in_xf, dA, s, 3, 1, c.cin_p, c.cout, m->grads + c.w_off);
    wa.algo_flops = 2.0 * s.N * s.H * s.W * 9.0 * c.cin * c.cout;
    if (!dx) {
        m->wgrad_on_side(wa, dy_done);
        return;
    }
    // (dx exists only for layers whose cin == cin_p)
    ConvArgs a = m->conv_same(View{dA, c.cout}, InXform{}, s, 3, 1, c.cout, c.cin, c.wd, c.wd3, nullptr, dx);
    a.done = m->next_fork_event();      // the weight gradient starts when this kernel completes
    launch_conv(ctx, a);
    m->wgrad_on_side(wa, a.done_used ? a.done : nullptr, !a.done_used);
}

}  // namespace

// A layer's weight gradient has no consumer before the optimiser: it is a FILLER for the stretches in which the main stream
// runs memory-bound BatchNorm-backward kernels: it is enqueued on the side stream when its layer is done
void rfi_model::wgrad_on_side(const rfi::WgradArgs& wa, hipEvent_t after, bool after_everything) {
    SideScope side(this, after_everything ? nullptr : after);      // (no event: the side stream waits for everything enqueued on main so far)
    launch_wgrad(ctx, wa);
    side.end();
}

void rfi_model::backward(const float* x_dev, const uint8_t* labels_dev, int n, int h, int w) {
    join_pending_side();
    sync_filters(Half::Both);         // (the weights may have changed since the forward pass)
    wait_wd();                        // the input-gradient-direction copies of a split rebuild come from the side stream
    backward_pass(x_dev, labels_dev, n, h, w);
}

void UNetModel::backward_pass(const float* x_dev, const uint8_t* labels_dev, int n, int h, int w) {
    const int D = depth, IB = i_bott;
    const int64_t M1 = (int64_t)n * h * w;
    if (planesP) return backward_planes(x_dev, labels_dev, n, h, w);
    side_bound = resnet_encoder ? 2 : 0;          // (the ResNet-style encoder double-buffers by block parity: bound 2)
    dbias_deferred = !resnet_encoder && dbias_pool && !ctx->exchange_active();
    // loss -> dlogits -> head
    loss_backward(labels_dev, M1);
    int head_records = 0;
    // a one-channel head sends d[pixel] * w[channel] down: where its BatchNorm-backward sums come out of launch_head_bwd's own
    // pass the gradient tensor is never written -- bn_bwd_apply recomputes it from the logit gradients (268 MB of HBM traffic
    // less at batch 64 x 128^2 x 32, in the one stretch of the step where no matrix-core kernel can run)
    bool head_skip = out_ch == 1;
    {
        ConvBN& last = convs[IB + 2 + 2 * (D - 1) + 1];
        // (head partials behind the region where the next layer expects its BatchNorm-backward records)
        const bool hdefer = dbias_deferred && head_fin_deferred;
        head_records = launch_head_bwd(ctx, buf(decY2[1]), M1, feat, last.scale(), last.shift(), params + head_w_off,
                                       out_ch, buf(dlogits), buf(gA[1]),
                                       hdefer ? dbias_pool + head_rec_off : buf(ws_red) + bn_bwd_ws_floats(M1, feat),
                                       grads + head_w_off, grads + head_b_off, act_slope, last.mean(), last.invstd(),
                                       buf(ws_red), nullptr, &head_skip, !hdefer);
    }
    // decoders, shallow to deep
    for (int l = 1; l <= D; ++l) {
        const int k = D - l;
        Shape s{n, h >> (l - 1), w >> (l - 1)};
        Shape sin{n, h >> l, w >> l};
        ConvBN& c1 = convs[IB + 2 + 2 * k];
        ConvBN& c2 = convs[IB + 2 + 2 * k + 1];
        UpConv& u = ups[k];
        // conv2: input = act(decY1) ; conv1: input = concat (materialised)
        const bool from_head = l == 1 && head_skip;
        backward_conv_bn(this, c2, buf(gA[l]), buf(decY2[l]), View{buf(decY1[l]), c1.cout}, bn_xf(c1), s,
                         buf(gB[l]), l == 1 ? head_records : 0, from_head ? buf(dlogits) : nullptr,
                         from_head ? params + head_w_off : nullptr);
        backward_conv_bn(this, c1, buf(gB[l]), buf(decY1[l]), View{buf(concat[l]), 2 * u.cout}, InXform{}, s,
                         buf(dconcat[l]), 0);
        // up-conv: dUp = dconcat[..., 0:C]
        const float* prevY = (l == D) ? buf(bottY2) : buf(decY2[l + 1]);
        ConvBN& prevBN = (l == D) ? convs[IB + 1] : convs[IB + 2 + 2 * (k - 1) + 1];
        View dUp{buf(dconcat[l]), 2 * u.cout};
        {
            const bool defer = dbias_deferred && u.cout % 4 == 0;
            launch_channel_sum(ctx, dUp, (int64_t)s.N * s.H * s.W, u.cout, defer ? dbias_pool + u.dbias_rec_off : buf(ws_red),
                               grads + u.b_off, !defer);
        }
        convt_backward(u, dUp, View{prevY, u.cin}, bn_xf(prevBN), sin, (l == D) ? buf(gBottA) : buf(gA[l + 1]));
        // gradients of decoder level l (and, for l = 1, of the head) are complete: exchange them now
        bucket_ready(u.w_off, l == 1 ? n_flat : ups[k + 1].w_off);
    }
    // bottleneck
    {
        Shape s{n, h >> D, w >> D};
        ConvBN& c1 = convs[IB];
        ConvBN& c2 = convs[IB + 1];
        backward_conv_bn(this, c2, buf(gBottA), buf(bottY2), View{buf(bottY1), c1.cout}, bn_xf(c1), s, buf(gBottB), 0);
        backward_conv_bn(this, c1, buf(gBottB), buf(bottY1), View{buf(pool[D]), c1.cin}, InXform{}, s, buf(dpool[D]), 0);
        bucket_ready(c1.w_off, ups[0].w_off);
    }
    if (resnet_encoder) {             // ResNet-style encoder (model_resnet.cpp)
        backward_resnet_encoder(x_dev, n, h, w);
        side_join();
        return;
    }
    // encoders, deep to shallow.  They write their own gradient tensors (not the decoder's of the same level), so nothing
    // the weight-gradient kernels read is rewritten before side_join(): no run-ahead bound
    for (int l = D; l >= 1; --l) {
        Shape s{n, h >> (l - 1), w >> (l - 1)};
        ConvBN& c1 = convs[2 * (l - 1)];
        ConvBN& c2 = convs[2 * (l - 1) + 1];
        const std::vector<int>& gA = this->gAe;
        const std::vector<int>& gB = this->gBe;
        // max-pool routing + skip gradient, with the BatchNorm-backward sums of c2 from the same pass where the
        // shape allows (else the separate reduction inside backward_conv_bn)
        int have = launch_pool_bwd_merge_sums(ctx, buf(encY2[l]), s.N, s.H, s.W, c2.cout, c2.scale(), c2.shift(), c2.mean(),
                                              c2.invstd(), View{buf(dconcat[l]) + c2.cout, 2 * c2.cout}, buf(dpool[l]),
                                              buf(gA[l]), act_slope, buf(ws_red));
        if (!have)
            launch_pool_bwd_merge(ctx, buf(encY2[l]), s.N, s.H, s.W, c2.cout, c2.scale(), c2.shift(),
                                  View{buf(dconcat[l]) + c2.cout, 2 * c2.cout}, buf(dpool[l]), buf(gA[l]), act_slope);
        backward_conv_bn(this, c2, buf(gA[l]), buf(encY2[l]), View{buf(encY1[l]), c1.cout}, bn_xf(c1), s, buf(gB[l]), have);
        View in = (l == 1) ? padded_input(x_dev) : View{buf(pool[l - 1]), c1.cin};
        backward_conv_bn(this, c1, buf(gB[l]), buf(encY1[l]), in, InXform{}, s,
                         (l == 1) ? nullptr : buf(dpool[l - 1]), 0);
        bucket_ready(c1.w_off, convs[l == D ? IB : 2 * l].w_off);       // convs[2 l] = first conv of the next level / the bottleneck
    }
    if (dbias_deferred) launch_finish_channel_sums_batched(ctx, static_cast<const FinishSumDesc*>(dbias_descs), dbias_n, dbias_max_c);
    side_join();
    side_bound = 2;
}

// ------------------------------------------------------------------------------------ optimiser
void rfi_model::apply(const rfi_hyper& hp, float grad_scale) {
    join_pending_side();
    double* ws = reinterpret_cast<double*>(buf(ws_red));
    launch_sumsq(ctx, grads, (int64_t)n_flat, ws, d_sums + 4);
    adam_step += 1;
    AdamArgs a;
    a.p = params; a.g = grads; a.m = adam_m; a.v = adam_v; a.n = (int64_t)n_flat;
    a.beta2 = (float)hp.beta2; a.eps = (float)hp.eps; a.wd = (float)hp.weight_decay;
    a.max_norm = (float)hp.max_grad_norm; a.grad_scale = grad_scale;
    a.one_minus_beta1 = (float)(1.0 - hp.beta1);
    a.one_minus_beta2 = (float)(1.0 - hp.beta2);
    a.neg_step = (float)(-(hp.lr / (1.0 - std::pow(hp.beta1, (double)adam_step))));
    a.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(hp.beta2, (double)adam_step));
    a.sumsq = d_sums + 4;
    a.norm_out = d_scalars + 1;
    launch_adam(ctx, a);
    weights_changed();
}

// ------------------------------------------------------------------------------------ entry-point hooks
void rfi_model::set_compute_dtype(int dtype) {
    arith = dtype == 1 || dtype == 4 ? Arith::BF16 : dtype == 2 || dtype == 3 ? Arith::X3 : Arith::F32;
}
void UNetModel::set_compute_dtype(int dtype) {
    rfi_model::set_compute_dtype(dtype);
    // the ResNet-encoder U-Net has the bfloat16 flow only, for widths in whole 16-channel chunks (else: dtype 4's kernels)
    if (resnet_encoder) set_planes(dtype == 1 && feat % 16 == 0 ? 1 : 0);
    else set_planes(dtype == 1 ? 1 : (dtype == 3 ? 3 : 0));
}

void rfi_model::debug_tensor(const std::string&, const std::string&, int, bool, CallScope&, const float*&, size_t&) {
    throw Error("debug_tensor: this model exposes only logits / dlogits / chan (the U-Net and the ResNet-50-FPN backbone expose their "
                "own tensors, the ResNet-encoder U-Net its decoder's and, on the bfloat16 flow, its encoder's, the detector heads their "
                "layer outputs and gradients: see rfi_hip.h)");
}
void UNetModel::debug_tensor(const std::string& name, const std::string& base, int idx, bool to_host, CallScope& sc, const float*& src,
                             size_t& n) {
    if (planesP && !resnet_encoder) return debug_tensor_planes(name, base, idx, to_host, sc, src, n);
    if (resnet_planes() && debug_tensor_resnet_planes(name, base, idx, to_host, sc, src, n)) return;      // (its encoder's bfloat16 tensors)
    RFI_REQUIRE(name.find(':') == std::string::npos, "debug_tensor: only the plain U-Net on a plane data flow has plane tensors");
    if (resnet_encoder && (base == "encY1" || base == "encY2" || base == "pool" || base == "dpool"))
        return rfi_model::debug_tensor(name, base, idx, to_host, sc, src, n);
    size_t M = 0;
    int C = 0;
    if (const FlowTensor* t = flow_named(base, idx, M, C)) {
        // (`half` is prepare_planes's: it says nothing once the model has left the bfloat16 flow)
        const bool b16 = planesP == 1 && t->half;
        if (b16 && base == "dconcat") {           // its values as float32 (tools/race_probe.py watches it)
            if (to_host) launch_planes_to_f32(ctx, pl[t->b16].p, pl[t->b16].pstride, (int64_t)M, C, 1, buf(*t), C);
        } else {
            RFI_REQUIRE(!b16, "debug_tensor: this tensor is stored as bfloat16 in the bfloat16 compute mode");
        }
        // (the float32 path's encoder phase has gradient tensors of its own)
        const bool enc_own = !planesP && !resnet_encoder && (base == "gA" || base == "gB");
        src = enc_own ? buf((base == "gA" ? gAe : gBe)[idx]) : buf(*t);
        n = M * C;
        return;
    }
    RFI_REQUIRE(base == "concat" || base == "pool", "debug_tensor: unknown tensor " + name);
    RFI_REQUIRE(idx >= 1 && idx <= depth, "debug_tensor: level out of range");
    const size_t Ml = (size_t)pN * (pH >> (idx - 1)) * (pW >> (idx - 1)), Cl = (size_t)feat << (idx - 1);
    src = buf(base == "concat" ? concat[idx] : pool[idx]);
    n = base == "concat" ? Ml * 2 * Cl : Ml / 4 * Cl;
}

const FlowTensor* UNetModel::flow_named(const std::string& base, int idx, size_t& M, int& C) const {
    struct Row { const char* name; const std::vector<FlowTensor>* levels; const FlowTensor* bott; int pixdiv, chmul; };
    const Row rows[] = {{"encY1", &encY1, nullptr, 1, 1}, {"encY2", &encY2, nullptr, 1, 1}, {"decY1", &decY1, nullptr, 1, 1},
                        {"decY2", &decY2, nullptr, 1, 1}, {"gA", &gA, nullptr, 1, 1}, {"gB", &gB, nullptr, 1, 1},
                        {"dpool", &dpool, nullptr, 4, 1}, {"dconcat", &dconcat, nullptr, 1, 2},
                        {"bottY1", nullptr, &bottY1, 1, 1}, {"bottY2", nullptr, &bottY2, 1, 1},
                        {"gBottA", nullptr, &gBottA, 1, 1}, {"gBottB", nullptr, &gBottB, 1, 1}};
    for (const Row& r : rows) {
        if (base != r.name) continue;
        RFI_REQUIRE(!r.levels || (idx >= 1 && idx <= depth), "debug_tensor: level out of range");
        const int l = r.levels ? idx : depth + 1;           // (the bottleneck: one level below the last)
        M = (size_t)pN * (pH >> (l - 1)) * (pW >> (l - 1)) / r.pixdiv;
        C = (feat << (l - 1)) * r.chmul;
        return r.levels ? &(*r.levels)[l] : r.bott;
    }
    return nullptr;
}

void UNetModel::algorithmic_flops(int n, int h, int w, double& fwd, double& step) const {
    double f = 0, stem = 0;
    for (size_t ci = 0; ci < convs.size(); ++ci) {
        const int lvl = convs[ci].level, R = convs[ci].R;       // M = OUTPUT pixels (stride-2 convs included)
        const double M = (double)n * (h >> (lvl - 1)) * (w >> (lvl - 1));
        const double fl = 2.0 * M * R * R * convs[ci].cin * convs[ci].cout;
        f += fl;
        if (ci == 0) stem = fl;
    }
    for (int k = 0; k < depth; ++k) {
        const int l = depth - k;
        const double M = (double)n * (h >> l) * (w >> l);
        f += 2.0 * M * 4.0 * ups[k].cin * ups[k].cout;
    }
    f += 2.0 * n * h * w * (double)feat * out_ch;
    fwd = f;
    step = 3.0 * f - stem;     // fwd + dgrad + wgrad, no dgrad for the first layer
}
