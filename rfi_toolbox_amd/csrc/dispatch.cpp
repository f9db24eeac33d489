// Which kernel runs a conv-like contraction or a weight gradient, and how much slab workspace the latter may need: the one
// place that reads the IMPL_* codes, the arithmetic flags and the kernels' *_eligible predicates.  Host code only; the MFMA
// kernels' tile choice stays beside the kernels (dispatch_tiles in conv_mfma.hip, select<> in the wgrad sources).
#include <algorithm>

#include "planes.hpp"

namespace rfi {

namespace {

// an IMPL_* code taken apart: what is asked for by name (IMPL_AUTO, IMPL_DIRECT, IMPL_MFMA, IMPL_PLANES_X3 for the plane
// kernels, IMPL_WS_X3 for the wave-specialised family) and the arithmetic the code carries
struct Impl { int name; bool bf16, bf16x3; int planes; };
Impl decode(int impl) {
    switch (impl) {
        case IMPL_MFMA_BF16: return {IMPL_MFMA, true, false, 0};
        case IMPL_MFMA_BF16X3: return {IMPL_MFMA, false, true, 0};
        case IMPL_PLANES_X3: return {IMPL_PLANES_X3, false, false, 3};
        case IMPL_PLANES_BF16: return {IMPL_PLANES_X3, false, false, 1};
        case IMPL_WS_X3: return {IMPL_WS_X3, false, true, 0};
        case IMPL_WS_BF16: return {IMPL_WS_X3, true, false, 0};
        default: return {impl, false, false, 0};
    }
}

}  // namespace

// ------------------------------------------------------------------------------------ conv-like contraction
void apply_impl(ConvArgs& a, int impl) {
    const Impl i = decode(impl);
    if (i.name == IMPL_WS_X3) { a.bf16 = i.bf16; a.bf16x3 = i.bf16x3; }      // (these kernels exist in one arithmetic each)
    else { a.bf16 |= i.bf16; a.bf16x3 |= i.bf16x3; }
    if (i.planes) a.planes = i.planes;
    if (impl == IMPL_MFMA_BF16X3) a.wB3 = nullptr;          // (asked for by name: not the wave-specialised kernel on the same filters)
}

ConvKernel choose_conv(const ConvArgs& a, int impl) {
    const int name = decode(impl).name;
    if (name == IMPL_PLANES_X3) RFI_REQUIRE(a.R == 3 && a.S == 1 && a.zgroups == 1, "conv: the plane kernels cover 3x3 stride-1 convolutions");
    if (name == IMPL_WS_X3) {
        if (impl == IMPL_WS_X3 && conv_stem_eligible(a)) return ConvKernel::Stem;
        if (conv_ws_eligible(a)) return ConvKernel::ConvWs;
        RFI_REQUIRE(gemm_ws_eligible(a), "conv: shape not eligible for the wave-specialised kernels");
        RFI_REQUIRE(impl == IMPL_WS_X3, "conv: the wave-specialised GEMM kernel exists in the 3 x bf16 arithmetic only");
        return ConvKernel::GemmWs;
    }
    if (name == IMPL_AUTO) {            // the wave-specialised kernels run where the caller holds their filter copy
        if (a.bf16x3 && conv_stem_eligible(a)) return ConvKernel::Stem;
        if (a.bf16x3 && a.wB3 && conv_ws_eligible(a)) return ConvKernel::ConvWs;
        if (a.bf16 && a.wB1 && conv_ws_eligible(a)) return ConvKernel::ConvWs;
        if (a.bf16x3 && a.wB3 && gemm_ws_eligible(a)) return ConvKernel::GemmWs;
    }
    if (a.planes) return ConvKernel::Planes;
    const bool ok = conv_mfma_eligible(a);
    if (name == IMPL_MFMA) RFI_REQUIRE(ok, "conv: shape/alignment not eligible for the MFMA kernel");
    return name == IMPL_DIRECT || !ok ? ConvKernel::Direct : ConvKernel::Mfma;
}

void launch_conv(rfi_ctx* ctx, ConvArgs& a, int impl) {
    apply_impl(a, impl);
    const ConvKernel k = choose_conv(a, impl);
    RFI_REQUIRE(a.N > 0 && a.H > 0 && a.W > 0 && a.Cin > 0 && a.Cout > 0, "conv: empty shape");
    RFI_REQUIRE(a.x.pstride >= a.Cin && a.y.pstride >= a.Cout, "conv: pixel stride smaller than channels");
    RFI_REQUIRE(a.zgroups == 1 || (a.zgroups == 4 && a.R == 1), "conv: zgroups only for convT forward");
    // (the stem kernel forms 64-bit offsets: its own, wider limit is part of conv_stem_eligible)
    RFI_REQUIRE(k == ConvKernel::Stem || ((int64_t)a.N * a.Hin * a.Win * a.x.pstride < (int64_t)1 << 31 &&
                                          (int64_t)a.N * a.Hout * a.Wout * a.y.pstride < (int64_t)1 << 31 &&
                                          (int64_t)a.R * a.R * a.Cin * a.Cout * a.zgroups < (int64_t)1 << 31),
                "conv: tensor too large for 32-bit element offsets");
    // ---- the temporary filter copies of a caller that holds float32 filters only (the kernel-level API, tests; a layer of
    // the plain U-Net whose wave-specialised kernel declined the shape -- rfi_model::ws_set cleared ConvArgs::w3 for it)
    CallScope sc(ctx);
    int P = a.bf16x3 && a.wB3 ? 3 : 1;          // the wave-specialised kernels: planes of the filter copy the caller holds
    const bf16_t* wb = P == 3 ? a.wB3 : a.wB1;
    if (decode(impl).name == IMPL_WS_X3 && k != ConvKernel::Stem) {
        // B-operand order.  conv_ws: [9][Cout][Cin]; gemm_ws: the transposed conv forward as ONE tap of 4 Cout channels, its
        // input gradient as four taps, a 1x1 conv as one tap
        const bool gw = k == ConvKernel::GemmWs;
        const int taps = gw ? (a.R == 2 ? 4 : 1) : 9, cout = gw && a.zgroups == 4 ? 4 * a.Cout : a.Cout;
        P = a.bf16x3 ? 3 : 1;
        bf16_t* t = sc.temp<bf16_t>(wb_elems(taps, cout, a.Cin, 0, P) + 32);
        launch_weights_to_wb_one(ctx, WBDesc{a.w, t, taps, cout, a.Cin, {a.Cin, 0}, P});
        wb = t;
    }
    struct ClearW3 { ConvArgs* a; ~ClearW3() { if (a) a->w3 = nullptr; } } clear_w3{nullptr};      // (ConvArgs::w3 is null again on return)
    if (k == ConvKernel::Mfma && a.bf16x3 && !a.w3) {       // the pre-split 3 x bf16 records
        const int taps = a.R * a.R * a.zgroups;
        float* w3 = sc.temp<float>(weights_x3_floats(taps, a.Cout, a.Cin));
        launch_weights_to_x3(ctx, a.w, taps, a.Cout, a.Cin, w3);
        a.w3 = w3;
        clear_w3.a = &a;
    }
    switch (k) {
        case ConvKernel::Stem: return launch_conv_stem(ctx, a);
        case ConvKernel::ConvWs: return launch_conv_ws(ctx, a, wb, P);
        case ConvKernel::GemmWs: return launch_gemm_ws(ctx, a, wb);
        case ConvKernel::Planes: return launch_pconv_from_f32(ctx, a, a.planes);
        case ConvKernel::Mfma: return launch_conv_mfma(ctx, a);
        case ConvKernel::Direct:
            RFI_REQUIRE(!a.y16, "conv: bfloat16 output needs the MFMA kernel");
            return launch_conv_direct(ctx, a);
    }
}

// ------------------------------------------------------------------------------------ weight gradient
void apply_impl(WgradArgs& a, int impl) {
    const Impl i = decode(impl);
    if (i.name == IMPL_WS_X3) return;   // (names conv kernels: a weight gradient runs as IMPL_AUTO in the caller's arithmetic)
    a.bf16 |= i.bf16;
    a.bf16x3 |= i.bf16x3;
}

WgradKernel choose_wgrad(const WgradArgs& a, int impl) {
    const int name = decode(impl).name;
    if (name == IMPL_PLANES_X3) {
        RFI_REQUIRE(a.R == 3 && a.S == 1, "wgrad: the plane kernel covers 3x3 stride-1 convolutions");
        return WgradKernel::Planes;
    }
    const bool narrow = a.bf16 || a.bf16x3, split_ok = wgrad_split_eligible(a);
    const bool ok = wgrad_mfma_eligible(a) || (narrow && split_ok);
    if (name == IMPL_MFMA) RFI_REQUIRE(ok, "wgrad: shape/alignment not eligible for the MFMA kernel");
    if (name == IMPL_DIRECT || !ok) return WgradKernel::Direct;
    if (a.bf16x3 && wgrad_stem_eligible(a)) return WgradKernel::Stem;       // Cx = 4: (tap, channel) packed into the GEMM's N
    if (narrow && wgrad_ws_eligible(a) && (split_ok || (a.R == 2 && a.S == 2))) return WgradKernel::Ws;
    // R = 2 / S = 1 and R = 1 (ResNet-style encoder) exist only in the split-at-staging kernel (P = 1: bf16 mode)
    const bool only_split = (a.R == 2 && a.S == 1) || a.R == 1;
    if (only_split) RFI_REQUIRE(narrow && split_ok,
                                "wgrad: 2x2 stride-1 and 1x1 weight gradients need the bf16 or 3 x bf16 arithmetic and 4-channel alignment");
    return (a.bf16x3 || only_split) && split_ok ? WgradKernel::Split : WgradKernel::Mfma;
}

// Every kernel choose_wgrad can return for this shape in ANY arithmetic and with any pointer alignment finds room: the
// direct kernel (the fall-back of an unaligned launch) always counts, the others wherever their predicate holds.  Within the
// shapes wgrad_split accepts, wgrad_ws plans on the same tiles for 256 workgroups where wgrad_split plans for 512, so its
// term decides only for the transposed conv (R = 2, stride 2), which wgrad_split does not cover.
size_t wgrad_slab_floats(const WgradArgs& a, int impl) {
    const Impl i = decode(impl);
    size_t need = wgrad_direct_slab_floats(a);
    if (i.planes && a.R == 3 && a.S == 1) return std::max(need, pwgrad_slab_floats_f32(a));
    if (i.name == IMPL_DIRECT) return need;
    if (wgrad_split_eligible(a)) need = std::max(need, wgrad_split_slab_floats(a));
    if (wgrad_ws_eligible(a)) need = std::max(need, wgrad_ws_slab_floats(a));
    if (wgrad_mfma_eligible(a)) need = std::max(need, wgrad_mfma_slab_floats(a));
    return need;
}

void launch_wgrad(rfi_ctx* ctx, const WgradArgs& a_in, int impl) {
    WgradArgs a = a_in;
    apply_impl(a, impl);
    const WgradKernel k = choose_wgrad(a, impl);
    if (k == WgradKernel::Planes) return launch_pwgrad_from_f32(ctx, a, decode(impl).planes);      // (checks its own limits)
    RFI_REQUIRE(a.N > 0 && a.H > 0 && a.W > 0 && a.Cx > 0 && a.Cy > 0, "wgrad: empty shape");
    RFI_REQUIRE((int64_t)a.N * a.Hx * a.Wx * a.xop.pstride < (int64_t)1 << 31 &&
                    (int64_t)a.N * a.H * a.W * a.yop.pstride < (int64_t)1 << 31,
                "wgrad: tensor too large for 32-bit element offsets");
    switch (k) {
        case WgradKernel::Direct: return launch_wgrad_direct(ctx, a);
        case WgradKernel::Stem: return launch_wgrad_stem(ctx, a);
        case WgradKernel::Ws: return launch_wgrad_ws(ctx, a);
        case WgradKernel::Split: return launch_wgrad_split(ctx, a);
        default: return launch_wgrad_mfma(ctx, a);
    }
}

}  // namespace rfi
