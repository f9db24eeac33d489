// extern "C" surface of librfi_hip.so, continued: the kernel-level ops (declared in include/rfi_hip.h).
#include <algorithm>

#include "model.hpp"

using namespace rfi;

// ------------------------------------------------------------------------------------ kernel-level ops
namespace {
float* upload_lib_weight(rfi_ctx* ctx, CallScope& s, const float* dev_ref, size_t numel, bool convt,
                         int d0, int d1, int R) {
    // dev_ref holds the reference layout ON DEVICE; bounce through the host to convert
    std::vector<float> h(numel), lib;
    RFI_CHECK_HIP(hipMemcpyAsync(h.data(), dev_ref, numel * 4, hipMemcpyDeviceToHost, ctx->stream));
    RFI_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    if (convt) to_lib_convt(h.data(), d0, d1, lib);
    else to_lib_conv(h.data(), d0, d1, R, lib);
    float* d = s.temp<float>(numel);
    RFI_CHECK_HIP(hipMemcpyAsync(d, lib.data(), numel * 4, hipMemcpyHostToDevice, ctx->stream));
    RFI_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return d;
}
// the reverse: a library-layout weight gradient on the device (3x3 conv [9][d0 = cout][d1 = cin], convT [4][cout][cin]
// as d0 = cin, d1 = cout) to the reference layout at the caller's device pointer
void store_ref_wgrad(rfi_ctx* ctx, const float* lib_dev, size_t numel, bool convt, int d0, int d1, float* dst_ref) {
    std::vector<float> lib(numel), ref(numel);
    RFI_CHECK_HIP(hipMemcpyAsync(lib.data(), lib_dev, numel * 4, hipMemcpyDeviceToHost, ctx->stream));
    RFI_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    if (convt) from_lib_convt(lib.data(), d0, d1, ref.data());
    else from_lib_conv(lib.data(), d0, d1, 3, ref.data());
    RFI_CHECK_HIP(hipMemcpyAsync(dst_ref, ref.data(), numel * 4, hipMemcpyHostToDevice, ctx->stream));
    RFI_CHECK_HIP(hipStreamSynchronize(ctx->stream));
}

// ---- the stride-2 layers on the plane kernels (bfloat16 flow of the ResNet-encoder model; impl 6): temporary plane copies
struct PlaneTmp {                 // a zero-tailed bf16 tensor [pixels][chunks * 16]
    bf16_t* p = nullptr;
    int64_t ps = 0;
    int nchunks = 0;
    PlaneSeg seg() const { return PlaneSeg{p, ps, nchunks}; }
};
PlaneTmp plane_tmp(rfi_ctx* ctx, CallScope& s, int64_t pixels, int C) {
    PlaneTmp t;
    t.nchunks = plane_chunks(C);
    t.ps = (int64_t)t.nchunks * 16;
    const size_t bytes = (size_t)pixels * t.ps * 2 + 64;
    t.p = reinterpret_cast<bf16_t*>(s.temp<float>((bytes + 3) / 4));
    RFI_CHECK_HIP(hipMemsetAsync(t.p, 0, bytes, ctx->stream));
    return t;
}
PlaneTmp planes_of(rfi_ctx* ctx, CallScope& s, const float* x, int64_t pixels, int C) {
    PlaneTmp t = plane_tmp(ctx, s, pixels, C);
    launch_act_split(ctx, View{x, C}, pixels, C, InXform{}, 1, t.p, t.ps);
    return t;
}
bf16_t* wb_of(rfi_ctx* ctx, CallScope& s, const float* src, int taps, int Cout, int Cin, int seg0, int seg1) {
    const size_t e = wb_elems(taps, Cout, seg0, seg1, 1);
    bf16_t* wb = reinterpret_cast<bf16_t*>(s.temp<float>((e * 2 + 64 + 3) / 4));
    RFI_CHECK_HIP(hipMemsetAsync(wb, 0, e * 2 + 64, ctx->stream));
    launch_weights_to_wb_one(ctx, WBDesc{src, wb, taps, Cout, Cin, {seg0, seg1}, 1});
    return wb;
}
// a weight gradient on a slab workspace of the call's own
void wgrad_in_scope(rfi_ctx* ctx, CallScope& s, WgradArgs& a, int impl) {
    a.slab_floats = wgrad_slab_floats(a, impl);
    a.slab = s.temp<float>(a.slab_floats);
    launch_wgrad(ctx, a, impl);
}
}  // namespace

extern "C" {

int rfi_op_conv3x3(rfi_ctx* ctx, int impl, const float* x, int n, int h, int w, int cin,
                   const float* w_oihw, const float* bias, int cout, const float* in_scale,
                   const float* in_shift, int in_relu, float* y) {
    return guarded([&] {
        ctx->activate();
        CallScope s(ctx);
        ConvArgs a;
        a.x = View{x, cin};
        a.N = n; a.H = h; a.W = w; a.Hin = h; a.Win = w; a.Cin = cin; a.Cout = cout;
        a.w = upload_lib_weight(ctx, s, w_oihw, (size_t)9 * cin * cout, false, cout, cin, 3);
        a.bias = bias;
        a.y = MutView{y, cout};
        a.Hout = h; a.Wout = w;
        a.xf = InXform{in_scale, in_shift, in_relu};
        launch_conv(ctx, a, impl);
    });
}
int rfi_op_conv1x1(rfi_ctx* ctx, int impl, const float* x, int n, int h, int w, int cin, const float* w_oihw, const float* bias,
                   int cout, const float* in_scale, const float* in_shift, int in_relu, float* y) {
    return guarded([&] {
        ctx->activate();
        CallScope s(ctx);
        ConvArgs a;
        a.x = View{x, cin};
        a.N = n; a.H = h; a.W = w; a.Hin = h; a.Win = w; a.Cin = cin; a.Cout = cout;
        a.w = upload_lib_weight(ctx, s, w_oihw, (size_t)cin * cout, false, cout, cin, 1);
        a.bias = bias;
        a.y = MutView{y, cout};
        a.Hout = h; a.Wout = w;
        a.R = 1; a.S = 1; a.pad = 0;
        a.xf = InXform{in_scale, in_shift, in_relu};
        launch_conv(ctx, a, impl);
    });
}
int rfi_op_conv3x3_dgrad(rfi_ctx* ctx, int impl, const float* dy, int n, int h, int w, int cout,
                         const float* w_oihw, int cin, float* dx) {
    return guarded([&] {
        ctx->activate();
        CallScope s(ctx);
        float* wf = upload_lib_weight(ctx, s, w_oihw, (size_t)9 * cin * cout, false, cout, cin, 3);
        float* wd = s.temp<float>((size_t)9 * cin * cout);
        launch_weight_to_dgrad(ctx, wf, 9, cout, cin, 1, wd);
        ConvArgs a;
        a.x = View{dy, cout};
        a.N = n; a.H = h; a.W = w; a.Hin = h; a.Win = w; a.Cin = cout; a.Cout = cin;
        a.w = wd;
        a.y = MutView{dx, cin};
        a.Hout = h; a.Wout = w;
        launch_conv(ctx, a, impl);
    });
}
int rfi_op_conv3x3_wgrad(rfi_ctx* ctx, int impl, const float* x, const float* dy, int n, int h, int w,
                         int cin, int cout, const float* in_scale, const float* in_shift, int in_relu,
                         float* dw_oihw) {
    return guarded([&] {
        ctx->activate();
        CallScope s(ctx);
        WgradArgs a;
        a.xop = View{x, cin};
        a.yop = View{dy, cout};
        a.xf_x = InXform{in_scale, in_shift, in_relu};
        a.N = n; a.H = h; a.W = w; a.Hx = h; a.Wx = w; a.Cx = cin; a.Cy = cout;
        a.tap_stride = (int64_t)cin * cout;
        a.sy = cin; a.sx = 1;
        const size_t numel = (size_t)9 * cin * cout;
        a.dw = s.temp<float>(numel);
        wgrad_in_scope(ctx, s, a, impl);
        store_ref_wgrad(ctx, a.dw, numel, false, cout, cin, dw_oihw);
    });
}
// ---- stride-2 convolutions of the ResNet-style encoder (model_resnet.cpp): 3x3 / pad 1 as a 2x2 convolution on the
// space-to-depth input, 1x1 / pad 0 on a channel slice of it.  h, w: INPUT size (even); outputs are h/2 x w/2.
int rfi_op_conv_s2(rfi_ctx* ctx, int impl, int ksize, const float* x, int n, int h, int w, int cin, const float* w_oihw,
                   int cout, float* y) {
    return guarded([&] {
        RFI_REQUIRE(ksize == 3 || ksize == 1, "conv_s2: kernel size 3 or 1");
        ctx->activate();
        CallScope s(ctx);
        if (impl == IMPL_PLANES_BF16) {           // the strided contraction on the full-resolution planes, bfloat16 output
            RFI_REQUIRE(cout % 4 == 0, "conv_s2 on planes: cout % 4 == 0");
            const int64_t Mo = (int64_t)n * (h / 2) * (w / 2);
            const PlaneTmp xp = planes_of(ctx, s, x, (int64_t)n * h * w, cin);
            const float* wl = ksize == 3 ? upload_lib_weight(ctx, s, w_oihw, (size_t)9 * cin * cout, false, cout, cin, 3) : w_oihw;
            PlaneTmp yp = plane_tmp(ctx, s, Mo, cout);
            PConvArgs a;
            a.x[0] = xp.seg(); a.nseg = 1; a.P = 1;
            a.N = n; a.H = h / 2; a.W = w / 2; a.Hin = h; a.Win = w; a.Hout = h / 2; a.Wout = w / 2;
            a.R = ksize; a.S = 2; a.pad = ksize == 3 ? 1 : 0;
            a.Cout = cout;
            a.wB = wb_of(ctx, s, wl, ksize * ksize, cout, cin, cin, 0);
            a.y16 = yp.p; a.y_pstride = (int)yp.ps;
            launch_pconv(ctx, a);
            launch_planes_to_f32(ctx, yp.p, yp.ps, Mo, cout, 1, y, cout);
            return;
        }
        float* xs = s.temp<float>((size_t)n * h * w * cin);
        launch_s2d(ctx, x, n, h, w, cin, xs);
        ConvArgs a;
        a.N = n; a.H = h / 2; a.W = w / 2; a.Hin = h / 2; a.Win = w / 2; a.Cout = cout;
        a.x = View{xs, 4 * cin};
        a.y = MutView{y, cout};
        a.Hout = h / 2; a.Wout = w / 2;
        a.S = 1;
        if (ksize == 3) {
            float* w3 = upload_lib_weight(ctx, s, w_oihw, (size_t)9 * cin * cout, false, cout, cin, 3);
            float* w2 = s.temp<float>((size_t)16 * cin * cout);
            launch_w_s2d(ctx, w3, cout, cin, w2, true);
            a.w = w2; a.Cin = 4 * cin; a.R = 2; a.pad = 1;
        } else {
            a.w = w_oihw; a.Cin = cin; a.R = 1; a.pad = 0;          // [cout][cin][1][1] == [1 tap][cout][cin]
        }
        launch_conv(ctx, a, impl);
    });
}
int rfi_op_conv_s2_dgrad(rfi_ctx* ctx, int impl, int ksize, const float* dy, int n, int h, int w, int cout,
                         const float* w_oihw, int cin, float* dx) {
    return guarded([&] {
        RFI_REQUIRE(ksize == 3 || ksize == 1, "conv_s2_dgrad: kernel size 3 or 1");
        ctx->activate();
        CallScope s(ctx);
        if (impl == IMPL_PLANES_BF16) {           // four 2x2 contractions of dY, one per parity class of the input pixel
            RFI_REQUIRE(cin % 4 == 0, "conv_s2_dgrad on planes: cin % 4 == 0");
            const int64_t Mo = (int64_t)n * (h / 2) * (w / 2), Mi = (int64_t)n * h * w;
            const PlaneTmp dyp = planes_of(ctx, s, dy, Mo, cout);
            const float* w3 = ksize == 3 ? upload_lib_weight(ctx, s, w_oihw, (size_t)9 * cin * cout, false, cout, cin, 3) : nullptr;
            float* cls = s.temp<float>(s2_class_floats(cout, cin));
            launch_w_s2_classes(ctx, w3, ksize == 1 ? w_oihw : nullptr, cout, cin, cls);     // (a 1x1 layer: the second K segment of class 0)
            PlaneTmp dxp = plane_tmp(ctx, s, Mi, cin);
            bf16_t* dx16 = dxp.p;                 // dense [Mi][cin] bfloat16 (cin % 16 != 0: rows of cin elements inside the allocation)
            for (int c = 0; c < 4; ++c) {
                PConvArgs a;
                a.x[0] = dyp.seg();
                if (c == 0) a.x[1] = dyp.seg();
                a.nseg = c == 0 ? 2 : 1; a.P = 1;
                a.N = n; a.H = h / 2; a.W = w / 2; a.Hin = h / 2; a.Win = w / 2;
                a.R = 2; a.S = 1; a.pad = 0;
                a.Cout = cin;
                a.wB = wb_of(ctx, s, cls + s2_class_offset(c, cout, cin), 4, cin, c == 0 ? 2 * cout : cout, cout, c == 0 ? cout : 0);
                a.y16 = dx16; a.y_pstride = cin;
                a.Hout = h; a.Wout = w; a.osy = 2; a.osx = 2; a.ooy = c >> 1; a.oox = c & 1;
                launch_pconv(ctx, a);
            }
            launch_planes_to_f32(ctx, dx16, cin, Mi, cin, 1, dx, cin);
            return;
        }
        ConvArgs a;
        a.N = n; a.H = h / 2; a.W = w / 2; a.Hin = h / 2; a.Win = w / 2; a.Cin = cout;
        a.x = View{dy, cout};
        a.Hout = h / 2; a.Wout = w / 2;
        a.S = 1;
        float* dxp = s.temp<float>((size_t)n * h * w * cin);
        float* ds = nullptr;
        if (ksize == 3) {
            float* w3 = upload_lib_weight(ctx, s, w_oihw, (size_t)9 * cin * cout, false, cout, cin, 3);
            float* w2 = s.temp<float>((size_t)16 * cin * cout);
            float* wd = s.temp<float>((size_t)16 * cin * cout);
            launch_w_s2d(ctx, w3, cout, cin, w2, true);
            launch_weight_to_dgrad(ctx, w2, 4, cout, 4 * cin, 1, wd);
            a.w = wd; a.Cout = 4 * cin; a.R = 2; a.pad = 0;
            a.y = MutView{dxp, 4 * cin};
        } else {
            float* wd = s.temp<float>((size_t)cin * cout);
            launch_weight_to_dgrad(ctx, w_oihw, 1, cout, cin, 0, wd);
            RFI_CHECK_HIP(hipMemsetAsync(dxp, 0, (size_t)n * h * w * cin * sizeof(float), ctx->stream));
            ds = s.temp<float>((size_t)n * (h / 2) * (w / 2) * cin);
            a.w = wd; a.Cout = cin; a.R = 1; a.pad = 0;
            a.y = MutView{ds, cin};
        }
        launch_conv(ctx, a, impl);
        launch_d2s_add(ctx, dxp, ds, View{}, n, h, w, cin, dx);
    });
}
int rfi_op_conv_s2_wgrad(rfi_ctx* ctx, int impl, int ksize, const float* x, const float* dy, int n, int h, int w, int cin,
                         int cout, float* dw_oihw) {
    return guarded([&] {
        RFI_REQUIRE(ksize == 3 || ksize == 1, "conv_s2_wgrad: kernel size 3 or 1");
        ctx->activate();
        CallScope s(ctx);
        if (impl == IMPL_PLANES_BF16) {           // the strided weight gradient on the full-resolution planes
            const PlaneTmp xp = planes_of(ctx, s, x, (int64_t)n * h * w, cin);
            const PlaneTmp dyp = planes_of(ctx, s, dy, (int64_t)n * (h / 2) * (w / 2), cout);
            PWgradArgs a;
            a.xop[0] = xp.seg(); a.nseg = 1; a.seg_c[0] = cin;
            a.yop = dyp.seg(); a.Cy = cout; a.P = 1;
            a.N = n; a.H = h / 2; a.W = w / 2; a.Hx = h; a.Wx = w;
            a.R = ksize; a.S = 2; a.pad = ksize == 3 ? 1 : 0;
            a.tap_stride = (int64_t)cin * cout; a.sy = cin; a.sx = 1;
            const size_t numel = (size_t)ksize * ksize * cin * cout;
            a.dw = s.temp<float>(numel);
            a.slab_floats = pwgrad_slab_floats(a);
            a.slab = s.temp<float>(a.slab_floats);
            launch_pwgrad(ctx, a);
            if (ksize == 1) {
                RFI_CHECK_HIP(hipMemcpyAsync(dw_oihw, a.dw, numel * 4, hipMemcpyDeviceToDevice, ctx->stream));
                return;
            }
            store_ref_wgrad(ctx, a.dw, numel, false, cout, cin, dw_oihw);
            return;
        }
        float* xs = s.temp<float>((size_t)n * h * w * cin);
        launch_s2d(ctx, x, n, h, w, cin, xs);
        WgradArgs a;
        a.xop = View{xs, 4 * cin};
        a.yop = View{dy, cout};
        a.N = n; a.H = h / 2; a.W = w / 2; a.Hx = h / 2; a.Wx = w / 2; a.Cy = cout;
        a.S = 1; a.sx = 1;
        if (ksize == 3) { a.Cx = 4 * cin; a.R = 2; a.pad = 1; }
        else { a.Cx = cin; a.R = 1; a.pad = 0; }
        a.tap_stride = (int64_t)a.Cx * cout;
        a.sy = a.Cx;
        const size_t numel = (size_t)a.R * a.R * a.Cx * cout;
        a.dw = s.temp<float>(numel);
        wgrad_in_scope(ctx, s, a, impl);
        if (ksize == 1) {
            RFI_CHECK_HIP(hipMemcpyAsync(dw_oihw, a.dw, numel * 4, hipMemcpyDeviceToDevice, ctx->stream));
            return;
        }
        const size_t n3 = (size_t)9 * cin * cout;
        float* w3 = s.temp<float>(n3);
        launch_w_s2d(ctx, w3, cout, cin, a.dw, false);
        store_ref_wgrad(ctx, w3, n3, false, cout, cin, dw_oihw);
    });
}
int rfi_op_convt2x2(rfi_ctx* ctx, int impl, const float* x, int n, int h, int w, int cin,
                    const float* w_iohw, const float* bias, int cout, float* y) {
    return guarded([&] {
        ctx->activate();
        CallScope s(ctx);
        if (impl == IMPL_PLANES_BF16) {           // ONE 1x1 contraction on planes: the four taps are 4 cout output channels
            RFI_REQUIRE(cout % 32 == 0, "convt2x2 on planes: cout % 32 == 0");
            const int64_t Mi = (int64_t)n * h * w;
            const PlaneTmp xp = planes_of(ctx, s, x, Mi, cin);
            const float* wl = upload_lib_weight(ctx, s, w_iohw, (size_t)4 * cin * cout, true, cin, cout, 2);      // [4][cout][cin]
            PlaneTmp yp = plane_tmp(ctx, s, 4 * Mi, cout);
            PConvArgs a;
            a.x[0] = xp.seg(); a.nseg = 1; a.P = 1;
            a.N = n; a.H = h; a.W = w; a.Hin = h; a.Win = w;
            a.R = 1; a.S = 1; a.pad = 0;
            a.Cout = 4 * cout; a.zblocks = cout / 32;
            a.wB = wb_of(ctx, s, wl, 1, 4 * cout, cin, cin, 0);
            a.bias = bias;
            a.y16 = yp.p; a.y_pstride = (int)yp.ps;
            a.Hout = 2 * h; a.Wout = 2 * w; a.osy = 2; a.osx = 2;
            launch_pconv(ctx, a);
            launch_planes_to_f32(ctx, yp.p, yp.ps, 4 * Mi, cout, 1, y, cout);
            return;
        }
        ConvArgs a;
        a.x = View{x, cin};
        a.N = n; a.H = h; a.W = w; a.Hin = h; a.Win = w; a.Cin = cin; a.Cout = cout;
        a.w = upload_lib_weight(ctx, s, w_iohw, (size_t)4 * cin * cout, true, cin, cout, 2);
        a.bias = bias;
        a.y = MutView{y, cout};
        a.Hout = 2 * h; a.Wout = 2 * w;
        a.osy = 2; a.osx = 2;
        a.R = 1; a.S = 1; a.pad = 0; a.zgroups = 4;
        launch_conv(ctx, a, impl);
    });
}
int rfi_op_convt2x2_dgrad(rfi_ctx* ctx, int impl, const float* dy, int n, int h, int w, int cout,
                          const float* w_iohw, int cin, float* dx) {
    return guarded([&] {
        ctx->activate();
        CallScope s(ctx);
        float* wf = upload_lib_weight(ctx, s, w_iohw, (size_t)4 * cin * cout, true, cin, cout, 2);
        float* wd = s.temp<float>((size_t)4 * cin * cout);
        launch_weight_to_dgrad(ctx, wf, 4, cout, cin, 0, wd);
        if (impl == IMPL_PLANES_BF16) {           // a 2x2 stride-2 contraction of dy on planes, bfloat16 out
            RFI_REQUIRE(cin % 4 == 0, "convt2x2_dgrad on planes: cin % 4 == 0");
            const int64_t Mi = (int64_t)n * h * w;
            const PlaneTmp dyp = planes_of(ctx, s, dy, 4 * Mi, cout);
            PlaneTmp dxp = plane_tmp(ctx, s, Mi, cin);
            PConvArgs a;
            a.x[0] = dyp.seg(); a.nseg = 1; a.P = 1;
            a.N = n; a.H = h; a.W = w; a.Hin = 2 * h; a.Win = 2 * w; a.Hout = h; a.Wout = w;
            a.R = 2; a.S = 2; a.pad = 0;
            a.Cout = cin;
            a.wB = wb_of(ctx, s, wd, 4, cin, cout, cout, 0);
            a.y16 = dxp.p; a.y_pstride = (int)dxp.ps;
            launch_pconv(ctx, a);
            launch_planes_to_f32(ctx, dxp.p, dxp.ps, Mi, cin, 1, dx, cin);
            return;
        }
        ConvArgs a;               // (n,h,w) is the INPUT grid of the convT, dy is (n,2h,2w,cout)
        a.x = View{dy, cout};
        a.N = n; a.H = h; a.W = w; a.Hin = 2 * h; a.Win = 2 * w; a.Cin = cout; a.Cout = cin;
        a.w = wd;
        a.y = MutView{dx, cin};
        a.Hout = h; a.Wout = w;
        a.R = 2; a.S = 2; a.pad = 0;
        launch_conv(ctx, a, impl);
    });
}
int rfi_op_convt2x2_wgrad(rfi_ctx* ctx, int impl, const float* x, const float* dy, int n, int h, int w,
                          int cin, int cout, float* dw_iohw) {
    return guarded([&] {
        ctx->activate();
        CallScope s(ctx);
        WgradArgs a;
        a.xop = View{dy, cout};
        a.yop = View{x, cin};
        a.N = n; a.H = h; a.W = w; a.Hx = 2 * h; a.Wx = 2 * w; a.Cx = cout; a.Cy = cin;
        a.R = 2; a.S = 2; a.pad = 0;
        a.tap_stride = (int64_t)cin * cout;
        a.sy = 1; a.sx = cin;
        const size_t numel = (size_t)4 * cin * cout;
        a.dw = s.temp<float>(numel);
        if (impl == IMPL_PLANES_BF16) {           // the 2x2 stride-2 weight gradient on planes (Xop = the output gradient)
            const PlaneTmp dyp = planes_of(ctx, s, dy, (int64_t)4 * n * h * w, cout);
            const PlaneTmp xp = planes_of(ctx, s, x, (int64_t)n * h * w, cin);
            PWgradArgs pa;
            pa.xop[0] = dyp.seg(); pa.nseg = 1; pa.seg_c[0] = cout;
            pa.yop = xp.seg(); pa.Cy = cin; pa.P = 1;
            pa.N = n; pa.H = h; pa.W = w; pa.Hx = 2 * h; pa.Wx = 2 * w;
            pa.R = 2; pa.S = 2; pa.pad = 0;
            pa.dw = a.dw; pa.tap_stride = a.tap_stride; pa.sy = 1; pa.sx = cin;
            pa.slab_floats = pwgrad_slab_floats(pa);
            pa.slab = s.temp<float>(pa.slab_floats);
            launch_pwgrad(ctx, pa);
        } else {
            wgrad_in_scope(ctx, s, a, impl);
        }
        store_ref_wgrad(ctx, a.dw, numel, true, cin, cout, dw_iohw);
    });
}
int rfi_op_roi_align(rfi_ctx* ctx, const float* x, int n, int h, int w, int c, const float* rois, int r,
                     float spatial_scale, int ph, int pw, int sampling_ratio, int aligned, float* out) {
    return guarded([&] {
        ctx->activate();
        launch_roi_align_fwd(ctx, x, n, h, w, c, rois, r, spatial_scale, ph, pw, sampling_ratio, aligned != 0, out);
    });
}
int rfi_op_roi_align_backward(rfi_ctx* ctx, const float* dout, int n, int h, int w, int c, const float* rois_sorted, int r,
                              float spatial_scale, int ph, int pw, int sampling_ratio, int aligned, float* dx) {
    return guarded([&] {
        ctx->activate();
        launch_roi_align_bwd(ctx, dout, n, h, w, c, rois_sorted, r, spatial_scale, ph, pw, sampling_ratio, aligned != 0, dx);
    });
}
int rfi_op_mask_targets(rfi_ctx* ctx, const uint8_t* masks, int g, int h, int w, const float* rois, int r, int ph, int pw,
                        int sampling_ratio, uint8_t* out) {
    return guarded([&] {
        ctx->activate();
        launch_mask_targets(ctx, masks, g, h, w, rois, r, ph, pw, sampling_ratio, out);
    });
}
int rfi_op_box_decode(rfi_ctx* ctx, const float* anchors, int64_t n_anchors, const float* deltas, int64_t n, float clip_h,
                      float clip_w, float* boxes) {
    return guarded([&] {
        ctx->activate();
        launch_box_decode(ctx, anchors, n_anchors, deltas, n, clip_h, clip_w, boxes);
    });
}
int rfi_op_add_inplace(rfi_ctx* ctx, float* x, const float* y, int64_t n) {
    return guarded([&] {
        ctx->activate();
        launch_add_inplace(ctx, x, y, n);
    });
}
int rfi_op_nms(rfi_ctx* ctx, const float* boxes_sorted, int n, float iou_threshold, int32_t* keep_host, int* n_keep) {
    return guarded([&] {
        RFI_REQUIRE(keep_host && n_keep, "nms: null output");
        ctx->activate();
        if (n <= 0) { *n_keep = 0; return; }
        const int words = (n + 63) / 64;
        std::vector<unsigned long long> h((size_t)n * words), removed(words, 0ull);
        CallScope sc(ctx);
        launch_nms_mask(ctx, boxes_sorted, n, iou_threshold, sc.out(h.data(), RFI_HOST, h.size()));
        sc.finish();
        int k = 0;                                   // greedy scan in score order: keep i unless a kept box suppressed it
        for (int i = 0; i < n; ++i) {
            if (removed[i / 64] >> (i % 64) & 1ull) continue;
            keep_host[k++] = i;
            const unsigned long long* row = h.data() + (size_t)i * words;
            for (int w = i / 64; w < words; ++w) removed[w] |= row[w];
        }
        *n_keep = k;
    });
}
int rfi_op_nms_batched(rfi_ctx* ctx, const float* boxes_sorted, const int32_t* count, int sets, int k, float iou_threshold, uint8_t* keep) {
    return guarded([&] {
        ctx->activate();
        launch_nms_batched(ctx, boxes_sorted, count, sets, k, iou_threshold, keep);
    });
}
size_t rfi_op_rpn_loss_ws_bytes(void) { return rpn_loss_ws_doubles() * sizeof(double); }
// ---- the detector's box bookkeeping on the device (detect_sample.hip): nothing here synchronises or allocates
int rfi_op_rpn_loss(rfi_ctx* ctx, const float* head, int64_t pixels, int anchors_per_pixel, const int8_t* labels,
                    const float* targets, const int32_t* num_sampled_dev, float beta, float* dhead, void* workspace,
                    float* loss2_dev) {
    return guarded([&] {
        ctx->activate();
        RFI_REQUIRE(workspace && loss2_dev && num_sampled_dev, "rpn_loss: workspace, a 2-float device output and the device count");
        launch_rpn_loss(ctx, head, pixels, anchors_per_pixel, reinterpret_cast<const signed char*>(labels), targets, num_sampled_dev, beta,
                        dhead, static_cast<double*>(workspace), loss2_dev);
    });
}
int rfi_op_fastrcnn_loss(rfi_ctx* ctx, const float* head, int64_t rois, int num_classes, const int32_t* labels, const float* targets,
                         float beta, float* dhead, void* workspace, float* loss2_dev) {
    return guarded([&] {
        ctx->activate();
        RFI_REQUIRE(workspace && loss2_dev, "fastrcnn_loss: workspace (rfi_op_rpn_loss_ws_bytes) and a 2-float device output");
        launch_fastrcnn_loss(ctx, head, rois, num_classes, labels, targets, beta, dhead, static_cast<double*>(workspace), loss2_dev);
    });
}
int rfi_op_anchor_match_batched(rfi_ctx* ctx, const float* anchors, int64_t n, int64_t anchor_stride, const int32_t* anchor_count,
                                const float* gt_boxes, int images, int gt_max, const int32_t* gt_count, float fg_iou, float bg_iou,
                                int allow_low_quality, float* best_ws, int8_t* labels, int32_t* matched, float* targets) {
    return guarded([&] {
        ctx->activate();
        RFI_REQUIRE(best_ws, "anchor_match_batched: workspace of images x gt_max floats");
        launch_anchor_match_batched(ctx, anchors, n, anchor_stride, anchor_count, gt_boxes, images, gt_max, gt_count, fg_iou, bg_iou,
                                    allow_low_quality != 0, best_ws, reinterpret_cast<signed char*>(labels), matched, targets);
    });
}
int rfi_op_segsort_u64(rfi_ctx* ctx, uint64_t* keys, int n_segs, int stride) {
    return guarded([&] {
        ctx->activate();
        launch_segsort_u64(ctx, reinterpret_cast<unsigned long long*>(keys), n_segs, stride);
    });
}
int rfi_op_sample_keys(rfi_ctx* ctx, const int8_t* labels, int images, int n, const int32_t* count, uint64_t seed, uint32_t step,
                       uint32_t stream0, uint64_t* keys, int stride) {
    return guarded([&] {
        ctx->activate();
        launch_sample_keys(ctx, reinterpret_cast<const signed char*>(labels), images, n, count, seed, step, stream0,
                           reinterpret_cast<unsigned long long*>(keys), stride);
    });
}
int rfi_op_rpn_sample_apply(rfi_ctx* ctx, const uint64_t* keys_sorted, int images, int n, int stride, int batch, int max_pos,
                            const int8_t* labels, const float* targets, int levels, const int32_t* level_off_host,
                            int8_t* const* level_labels_host, float* const* level_targets_host, int32_t* n_sampled) {
    return guarded([&] {
        ctx->activate();
        RFI_REQUIRE(level_off_host && level_labels_host && level_targets_host && n_sampled, "rpn_sample_apply: null table");
        launch_rpn_sample_apply(ctx, reinterpret_cast<const unsigned long long*>(keys_sorted), images, n, stride, batch, max_pos,
                                reinterpret_cast<const signed char*>(labels), targets, levels, level_off_host,
                                reinterpret_cast<signed char* const*>(level_labels_host), level_targets_host, n_sampled);
    });
}
int rfi_op_topk_keys(rfi_ctx* ctx, const float* head, int images, int pixels, int anchors_per_pixel, uint64_t* keys, int stride) {
    return guarded([&] {
        ctx->activate();
        launch_topk_keys(ctx, head, images, pixels, anchors_per_pixel, reinterpret_cast<unsigned long long*>(keys), stride);
    });
}
int rfi_op_topk_decode(rfi_ctx* ctx, const uint64_t* keys_sorted, int images, int stride, int pixels, int anchors_per_pixel, int k,
                       const float* head, const float* anchors, float clip_h, float clip_w, float min_size, float* boxes, float* scores,
                       int32_t* counts, int levels, int level) {
    return guarded([&] {
        ctx->activate();
        launch_topk_decode(ctx, reinterpret_cast<const unsigned long long*>(keys_sorted), images, stride, pixels, anchors_per_pixel, k, head,
                           anchors, clip_h, clip_w, min_size, boxes, scores, counts, levels, level);
    });
}
int rfi_op_proposals_select(rfi_ctx* ctx, const float* boxes, const float* scores, const uint8_t* keep, int images, int levels, int k,
                            int post_nms, const float* gt_boxes, int gt_max, const int32_t* gt_count, int pmax, float* props,
                            int32_t* pcount) {
    return guarded([&] {
        ctx->activate();
        launch_proposals_select(ctx, boxes, scores, keep, images, levels, k, post_nms, gt_boxes, gt_max, gt_count, pmax, props, pcount);
    });
}
int rfi_op_roi_sample(rfi_ctx* ctx, const int8_t* labels, const int32_t* pcount, int images, int pmax, int batch, int max_pos,
                      uint64_t seed, uint32_t step, uint32_t stream0, int32_t* sel, int32_t* nsel, int32_t* npos) {
    return guarded([&] {
        ctx->activate();
        launch_roi_sample(ctx, reinterpret_cast<const signed char*>(labels), pcount, images, pmax, batch, max_pos, seed, step, stream0, sel,
                          nsel, npos);
    });
}
int rfi_op_roi_compact(rfi_ctx* ctx, const int32_t* sel, const int32_t* nsel, const int32_t* npos, int images, int batch, int pmax,
                       const float* props, const int32_t* matched, const float* targets, const int32_t* gt_labels, int gt_max,
                       const int32_t* gt_base, float t1, float t2, float t3, float* rois, int32_t* cls, float* tgt, int32_t* gt,
                       int32_t* level, int32_t* img_start, float* rois_fg, float* rois_gt, int32_t* level_fg, int32_t* fg_start,
                       int32_t* counts) {
    return guarded([&] {
        ctx->activate();
        launch_roi_compact(ctx, sel, nsel, npos, images, batch, pmax, props, matched, targets, gt_labels, gt_max, gt_base, t1, t2, t3, rois,
                           cls, tgt, gt, level, img_start, rois_fg, rois_gt, level_fg, fg_start, counts);
    });
}
// ---- detector inference on the device (detect_infer.hip): nothing here synchronises or allocates
int rfi_op_detect_candidates(rfi_ctx* ctx, const float* head, const float* props, const int32_t* pcount, int images, int pmax, int k1,
                             float clip_h, float clip_w, float score_thresh, float min_size, float* boxes, float* scores,
                             int32_t* counts) {
    return guarded([&] {
        ctx->activate();
        RFI_REQUIRE(head && props && pcount && boxes && scores && counts, "detect_candidates: null tensor");
        launch_detect_candidates(ctx, head, props, pcount, images, pmax, k1, clip_h, clip_w, score_thresh, min_size, boxes, scores, counts);
    });
}
int rfi_op_detect_select(rfi_ctx* ctx, const float* boxes, const float* scores, const uint8_t* keep, int images, int classes, int k,
                         int max_det, float t1, float t2, float t3, float* det_boxes, float* det_scores, int32_t* det_labels,
                         int32_t* det_count, float* rois, int32_t* level) {
    return guarded([&] {
        ctx->activate();
        RFI_REQUIRE(boxes && scores && keep && det_boxes && det_scores && det_labels && det_count && rois && level,
                    "detect_select: null tensor");
        launch_detect_select(ctx, boxes, scores, keep, images, classes, k, max_det, t1, t2, t3, det_boxes, det_scores, det_labels,
                             det_count, rois, level);
    });
}
int rfi_op_rois_from_boxes(rfi_ctx* ctx, const float* props, const int32_t* pcount, int images, int pmax, float t1, float t2, float t3,
                           float* rois, int32_t* level) {
    return guarded([&] {
        ctx->activate();
        RFI_REQUIRE(props && pcount && rois && level, "rois_from_boxes: null tensor");
        launch_rois_from_boxes(ctx, props, pcount, images, pmax, t1, t2, t3, rois, level);
    });
}
int rfi_op_mask_paste(rfi_ctx* ctx, const float* logits, const float* det_boxes, const int32_t* det_count, int images, int max_det, int h,
                      int w, uint8_t* rfi_mask, uint8_t* masks) {
    return guarded([&] {
        ctx->activate();
        RFI_REQUIRE(logits && det_boxes && det_count && rfi_mask, "mask_paste: null tensor");
        launch_mask_paste(ctx, logits, det_boxes, det_count, images, max_det, h, w, rfi_mask, masks);
    });
}
int rfi_op_bn_add_relu16(rfi_ctx* ctx, const uint16_t* y, const float* scale, const float* shift, const uint16_t* s, const float* s_scale,
                         const float* s_shift, int64_t m, int c, uint16_t* out) {
    return guarded([&] {
        ctx->activate();
        launch_bn_add_relu16(ctx, y, c, scale, shift, s, c, s_scale, s_shift, m, c, out, c);
    });
}
int rfi_op_relu_mask_sum16(rfi_ctx* ctx, const uint16_t* g0, const uint16_t* g1, const float* g2_f32, const uint16_t* g2_bf16,
                           int64_t g2_stride, const uint16_t* a, int64_t m, int c, uint16_t* dz) {
    return guarded([&] {
        ctx->activate();
        RFI_REQUIRE(!(g2_f32 && g2_bf16), "relu_mask_sum16: one third term at most");
        const YRef g2 = g2_bf16 ? YRef(g2_bf16, g2_stride) : YRef(g2_f32, g2_f32 ? g2_stride : (int64_t)0);
        launch_relu_mask_sum16(ctx, g0, c, g1, c, g2, a, c, m, c, dz, c);
    });
}
int rfi_op_bn_backward16(rfi_ctx* ctx, const uint16_t* da, const uint16_t* y, int64_t m, int c, const float* gamma, const float* scale,
                         const float* shift, const float* mean, const float* invstd, float slope, uint16_t* dy, float* dgamma,
                         float* dbeta, float* dbias) {
    return guarded([&] {
        ctx->activate();
        RFI_REQUIRE(m > 0 && c > 0 && c % 16 == 0, "bn_backward16: channels in whole 16-channel chunks");
        CallScope s(ctx);
        float* ws = s.temp<float>(std::max(bn_bwd_ws_floats(m, c), channel_sum_ws_floats(m, c)) + 16);
        float* c12 = s.temp<float>((size_t)2 * c);
        launch_bn_bwd_reduce(ctx, YRef(da, (int64_t)c), YRef(y, (int64_t)c), m, c, scale, shift, mean, invstd, ws, c12, c12 + c, dgamma, dbeta, slope);
        launch_bn_bwd_apply(ctx, YRef(da, (int64_t)c), YRef(y, (int64_t)c), m, c, scale, shift, mean, invstd, gamma, c12, c12 + c, ws, dbias, slope, dy,
                            (int64_t)c, 1);
    });
}
int rfi_op_roi_align_ml(rfi_ctx* ctx, const float* const* maps_host, int n, int h0, int w0, int c, float scale0, const float* rois,
                        const int32_t* level, const int32_t* count_dev, int max_rois, int ph, int pw, int sampling_ratio, float* out) {
    return guarded([&] {
        ctx->activate();
        RFI_REQUIRE(maps_host && count_dev, "roi_align_ml: null table");
        launch_roi_align_ml_fwd(ctx, maps_host, n, h0, w0, c, scale0, rois, level, count_dev, max_rois, ph, pw, sampling_ratio, out);
    });
}
int rfi_op_roi_align_ml_backward(rfi_ctx* ctx, float* const* dmaps_host, int n, int h0, int w0, int c, float scale0, const float* dout,
                                 const float* rois, const int32_t* level, const int32_t* img_start, int max_rois, int ph, int pw,
                                 int sampling_ratio) {
    return guarded([&] {
        ctx->activate();
        RFI_REQUIRE(dmaps_host && img_start, "roi_align_ml_backward: null table");
        launch_roi_align_ml_bwd(ctx, dmaps_host, n, h0, w0, c, scale0, dout, rois, level, img_start, max_rois, ph, pw, sampling_ratio);
    });
}
// a small device -> host copy that does NOT stall the host at once: begin enqueues the copy into pinned memory and an event
// behind it; whatever the caller enqueues next runs on; end waits for the event only (not for the later work)
int rfi_readback_begin(rfi_ctx* ctx, const void* src_dev, size_t bytes) {
    return guarded([&] {
        ctx->activate();
        RFI_REQUIRE(src_dev && bytes > 0 && bytes <= 2048, "readback_begin: 1 .. 2048 bytes");
        if (!ctx->readback_ev) RFI_CHECK_HIP(hipEventCreateWithFlags(&ctx->readback_ev, hipEventDisableTiming));
        RFI_CHECK_HIP(hipMemcpyAsync(reinterpret_cast<char*>(ctx->pinned) + 2048, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
        RFI_CHECK_HIP(hipEventRecord(ctx->readback_ev, ctx->stream));
        ctx->readback_bytes = bytes;
    });
}
int rfi_readback_end(rfi_ctx* ctx, void* dst_host, size_t bytes) {
    return guarded([&] {
        ctx->activate();
        RFI_REQUIRE(ctx->readback_ev && dst_host && bytes == ctx->readback_bytes, "readback_end: no matching readback_begin");
        RFI_CHECK_HIP(hipEventSynchronize(ctx->readback_ev));
        std::memcpy(dst_host, reinterpret_cast<char*>(ctx->pinned) + 2048, bytes);
        ctx->readback_bytes = 0;
    });
}
// ---- confusion counts at every threshold from one pass (threshold_sweep.hip)
int rfi_threshold_sweep(rfi_ctx* ctx, const float* scores, int scores_mem, int kind, const void* truth, int truth_dtype,
                        int truth_mem, int64_t count, int64_t group_elems, const float* thresholds_host, int n_thresholds,
                        int64_t* counts_host) {
    return guarded([&] {
        RFI_REQUIRE(ctx && scores && truth && thresholds_host && counts_host, "threshold_sweep: null argument");
        check_sweep_thresholds(thresholds_host, n_thresholds);
        RFI_REQUIRE(kind == RFI_VALUES_LOGITS || kind == RFI_VALUES_PROBS, "threshold_sweep: kind must be logits or probabilities");
        RFI_REQUIRE(truth_dtype == RFI_U8 || truth_dtype == RFI_FLOAT32, "threshold_sweep: truth must be u8 or f32");
        RFI_REQUIRE((scores_mem == RFI_HOST || scores_mem == RFI_DEVICE) && (truth_mem == RFI_HOST || truth_mem == RFI_DEVICE),
                    "threshold_sweep: bad memory kind");
        RFI_REQUIRE(count >= 1 && group_elems >= 1 && count % group_elems == 0 && count / group_elems <= 65535,
                    "threshold_sweep: count must be a positive multiple of group_elems, at most 65535 groups");
        const int64_t n_groups = count / group_elems;
        std::vector<unsigned long long> hist((size_t)n_groups * 2 * ((size_t)n_thresholds + 1));
        ctx->activate();
        CallScope sc(ctx);
        const float* ds = sc.in(scores, scores_mem, (size_t)count);
        const void* dt = sc.in(truth, truth_mem, (size_t)count * (truth_dtype == RFI_U8 ? 1 : 4));
        const float* dthr = sc.in(thresholds_host, RFI_HOST, (size_t)n_thresholds);
        launch_threshold_sweep(ctx, ds, kind, dt, truth_dtype, n_groups, group_elems, dthr, n_thresholds,
                               sc.out(hist.data(), RFI_HOST, hist.size()));
        sc.finish();
        threshold_sweep_counts(hist.data(), n_groups, n_thresholds, counts_host);
    });
}
// ---- training augmentation (augment.hip)
static void check_augment_config(const rfi_augment_config* cfg, int n, int h, int w) {
    RFI_REQUIRE(cfg, "augment: null config");
    for (float p : {cfg->p_hflip, cfg->p_vflip, cfg->p_rotate, cfg->p_ssr})
        RFI_REQUIRE(p >= 0.0f && p <= 1.0f, "augment: probabilities must be in [0, 1]");
    for (float l : {cfg->rotate_limit_deg, cfg->shift_limit, cfg->scale_limit, cfg->ssr_rotate_limit_deg})
        RFI_REQUIRE(l >= 0.0f && l <= 3.0e38f, "augment: limits must be finite and >= 0");
    RFI_REQUIRE(cfg->scale_limit < 1.0f, "augment: scale_limit must be < 1");
    RFI_REQUIRE(n >= 0 && h >= 1 && w >= 1 && (int64_t)h * w <= (int64_t(1) << 30), "augment: needs n >= 0, h, w >= 1 and h w <= 2^30");
}
int rfi_augment_params(const rfi_augment_config* cfg, uint64_t call, int n, int h, int w, int32_t* gates, double* inv) {
    return guarded([&] {
        check_augment_config(cfg, n, h, w);
        if (n == 0) return;
        RFI_REQUIRE(gates && inv, "augment_params: null output");
        augment_params_host(*cfg, call, n, h, w, gates, inv);
    });
}
int rfi_augment_batch(rfi_ctx* ctx, const float* x, int x_mem, const uint8_t* y, int y_mem, int n, int h, int w, int c,
                      const rfi_augment_config* cfg, uint64_t call, float* x_out, uint8_t* y_out) {
    return guarded([&] {
        RFI_REQUIRE(ctx, "augment_batch: null context");
        check_augment_config(cfg, n, h, w);
        RFI_REQUIRE(c >= 1 && c <= 16, "augment_batch: 1 <= c <= 16");
        if (n == 0) return;
        const int64_t px = (int64_t)n * h * w;
        RFI_REQUIRE(cdiv((int64_t)h * w, 256) * n <= 0x7fffffff, "augment_batch: batch too large for one launch");
        RFI_REQUIRE(x && y && x_out && y_out, "augment_batch: null buffer");
        const char *xi = reinterpret_cast<const char*>(x), *xo = reinterpret_cast<const char*>(x_out);
        const char *yi = reinterpret_cast<const char*>(y), *yo = reinterpret_cast<const char*>(y_out);
        RFI_REQUIRE(x_mem == RFI_HOST || xi + px * c * 4 <= xo || xo + px * c * 4 <= xi, "augment_batch: x and x_out overlap");
        RFI_REQUIRE(y_mem == RFI_HOST || yi + px <= yo || yo + px <= yi, "augment_batch: y and y_out overlap");
        ctx->activate();
        CallScope sc(ctx);
        const float* dx = sc.in(x, x_mem, (size_t)px * c);
        const uint8_t* dy = sc.in(y, y_mem, (size_t)px);
        const uintptr_t al = c % 4 == 0 ? 16 : 4;
        RFI_REQUIRE(reinterpret_cast<uintptr_t>(dx) % al == 0 && reinterpret_cast<uintptr_t>(x_out) % al == 0,
                    "augment_batch: float buffers must be 4-byte aligned (16-byte when c % 4 == 0)");
        launch_augment(ctx, dx, dy, n, h, w, c, *cfg, call, x_out, y_out);
        sc.finish();
    });
}
int rfi_op_fpn_merge(rfi_ctx* ctx, const float* lateral, const float* top, int n, int h, int w, int c, float* out) {
    return guarded([&] {
        ctx->activate();
        launch_fpn_merge_fwd(ctx, lateral, top, n, h, w, c, out);
    });
}
int rfi_op_fpn_merge_backward(rfi_ctx* ctx, const float* dout, int n, int h, int w, int c, float* dtop) {
    return guarded([&] {
        ctx->activate();
        launch_fpn_merge_bwd_top(ctx, dout, n, h, w, c, dtop);
    });
}
int rfi_op_bn_stats(rfi_ctx* ctx, const float* y, int64_t m, int c, float* mean, float* var_biased) {
    return guarded([&] {
        ctx->activate();
        CallScope s(ctx);
        float* ws = s.temp<float>(bn_stats_ws_floats(c));
        float* tmp = s.temp<float>((size_t)6 * c);
        std::vector<float> ones((size_t)c, 1.0f), zeros((size_t)c, 0.0f);
        RFI_CHECK_HIP(hipMemcpyAsync(tmp, ones.data(), c * 4, hipMemcpyHostToDevice, ctx->stream));
        RFI_CHECK_HIP(hipMemcpyAsync(tmp + c, zeros.data(), c * 4, hipMemcpyHostToDevice, ctx->stream));
        RFI_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        launch_bn_stats(ctx, y, m, c, ws);
        launch_bn_finalize(ctx, ws, m, c, tmp, tmp + c, nullptr, nullptr, 0, mean, tmp + 2 * c, tmp + 3 * c,
                           tmp + 4 * c, var_biased);
    });
}

int rfi_op_bn_relu_pool(rfi_ctx* ctx, const float* y, int n, int h, int w, int c, const float* scale,
                        const float* shift, float* skip, float* pooled) {
    return guarded([&] {
        ctx->activate();
        launch_bn_relu_pool(ctx, y, n, h, w, c, scale, shift, MutView{skip, c}, pooled);
    });
}
int rfi_op_pool_bwd_merge(rfi_ctx* ctx, const float* y, int n, int h, int w, int c, const float* scale,
                          const float* shift, const float* dskip, const float* dpool, float* da) {
    return guarded([&] {
        ctx->activate();
        launch_pool_bwd_merge(ctx, y, n, h, w, c, scale, shift, View{dskip, c}, dpool, da);
    });
}
int rfi_op_bn_relu_backward(rfi_ctx* ctx, const float* y, int64_t m, int c, const float* gamma,
                            const float* beta, float* da_inout, float* dgamma, float* dbeta, float* dbias) {
    return guarded([&] {
        ctx->activate();
        CallScope s(ctx);
        size_t wsf = bn_stats_ws_floats(c);
        if (bn_bwd_ws_floats(m, c) > wsf) wsf = bn_bwd_ws_floats(m, c);
        float* ws = s.temp<float>(wsf);
        float* t = s.temp<float>((size_t)6 * c);     // mean | invstd | scale | shift | c1 | c2
        launch_bn_stats(ctx, y, m, c, ws);
        launch_bn_finalize(ctx, ws, m, c, gamma, beta, nullptr, nullptr, 0, t, t + c, t + 2 * c, t + 3 * c,
                           nullptr);
        launch_bn_bwd_reduce(ctx, da_inout, y, m, c, t + 2 * c, t + 3 * c, t, t + c, ws, t + 4 * c, t + 5 * c,
                             dgamma, dbeta);
        launch_bn_bwd_apply(ctx, da_inout, y, m, c, t + 2 * c, t + 3 * c, t, t + c, gamma, t + 4 * c, t + 5 * c,
                            ws, dbias);
    });
}
// ---- per-patch order statistics (order_stats.hip) on their own: what rfi_preprocess_real / rfi_mad_flags build on
int rfi_op_patch_median(rfi_ctx* ctx, const double* v, int n, int per, int absdev, const double* centre, int finite_only, int f32,
                        double* median, int32_t* count) {
    return guarded([&] {
        RFI_REQUIRE(n >= 0 && per >= 1, "patch_median: n >= 0 patches of per >= 1 values");
        if (n == 0) return;
        RFI_REQUIRE(v && median, "patch_median: null tensor");
        RFI_REQUIRE(!absdev || centre, "patch_median: absolute deviations need the per-patch centres");
        ctx->activate();
        launch_patch_median(ctx, v, n, per, absdev != 0, absdev ? centre : nullptr, finite_only != 0, median, count, f32 != 0);
    });
}

}  // extern "C"
