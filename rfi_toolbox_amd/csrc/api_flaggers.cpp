// extern "C" surface of librfi_hip.so, continued: the baseline flaggers (declared in include/rfi_hip.h; kernels in
// sumthreshold.hip and casa_flaggers.hip).
#include <algorithm>
#include <initializer_list>

#include "kernels.hpp"
#include "launch_common.hpp"

using namespace rfi;

namespace {
constexpr size_t kFlagBudget = size_t(1) << 30;      // scratch of one group of planes

// The checks every entry point starts with: the context, the stack's shape and the memory kinds (pass RFI_HOST for a buffer
// that is absent).  False: the stack is empty and there is nothing to do; otherwise the context's device is current.
bool check_stack(const std::string& who, rfi_ctx* ctx, int n_planes, int c, int t, std::initializer_list<int> mems) {
    RFI_REQUIRE(ctx, who + ": null context");
    RFI_REQUIRE(n_planes >= 0 && c >= 1 && t >= 1 && c <= (1 << 20) && t <= (1 << 20), who + ": needs n_planes >= 0 and 1 <= C, T <= 2^20");
    RFI_REQUIRE((double)n_planes * c * t <= 4.0e9, who + ": stack too large for one call");
    for (int mem : mems) RFI_REQUIRE(mem == RFI_HOST || mem == RFI_DEVICE, who + ": bad memory kind");
    if (n_planes == 0) return false;
    ctx->activate();
    return true;
}
void check_dtype(const std::string& who, int dtype, bool real_ok) {
    RFI_REQUIRE(dtype == RFI_C128 || dtype == RFI_C64 || (real_ok && (dtype == RFI_F64 || dtype == RFI_F32)),
                who + ": dtype must be complex128" + (real_ok ? ", complex64, float64 or float32" : " or complex64"));
}
void check_st_config(const rfi_sumthreshold_config* cfg) {
    RFI_REQUIRE(cfg, "sumthreshold: null config");
    RFI_REQUIRE(cfg->iterations >= 1 && cfg->iterations <= 64, "sumthreshold: iterations must be in 1 .. 64");
    RFI_REQUIRE(cfg->levels >= 1 && cfg->levels <= 8, "sumthreshold: levels must be in 1 .. 8");
    RFI_REQUIRE(cfg->rho > 1.0 && cfg->rho <= 1.0e6, "sumthreshold: rho must be > 1");
    RFI_REQUIRE(cfg->base_sensitivity > 0.0 && cfg->chi_1 > 0.0, "sumthreshold: base_sensitivity and chi_1 must be > 0");
    RFI_REQUIRE(cfg->half_t >= 0 && cfg->half_f >= 0 && cfg->half_t <= (1 << 20) && cfg->half_f <= (1 << 20),
                "sumthreshold: half widths must be in 0 .. 2^20");
    RFI_REQUIRE(cfg->sir_q >= 0 && cfg->sir_q <= 1023, "sumthreshold: sir_q must be in 0 .. 1023");
}
bool in_range(double v, double lo, double hi) { return v >= lo && v <= hi; }      // (false for NaN)

// An optional host array of doubles that a flagger reads on the device: `doubles` values for every plane, which travel with
// the plane's group (RFlag's timedev and freqdev), or `doubles` values in all, uploaded once (SumThreshold's weight tables).
struct HostTable {
    const double* host;      // null: absent
    size_t doubles;
    bool per_plane;
};
const HostTable kNoTable{nullptr, 0, false};

// The one plane-group driver of the four flaggers.  The stack goes through the context's scratch in groups of k whole planes,
// k the largest number whose region stays under kFlagBudget: [tables uploaded once | workspace of the launch | staged data |
// staged prior | per-plane tables].  Host buffers are uploaded per group and the group's flags copied out, all on the
// context's stream; device buffers are used in place.  ws(planes): workspace bytes, at most planes ws(1).  run(data, prior,
// planes, workspace, device tables, dst) flags one group and returns where its flags are: dst is the group's place in a
// device flags_out, which a launch may write directly, or null when flags_out is on the host.  The driver copies the flags
// only when they are not at dst.
template <class Ws, class Run>
void flag_in_groups(rfi_ctx* ctx, const std::string& who, const void* data, int data_mem, size_t esz, const uint8_t* prior, int prior_mem,
                    int n_planes, int c, int t, const HostTable (&tables)[2], uint8_t* flags_out, int out_mem, Ws ws, Run run) {
    const size_t px = (size_t)c * t;
    const bool host_in = data_mem == RFI_HOST, host_pr = prior && prior_mem == RFI_HOST, host_out = out_mem == RFI_HOST;
    size_t fixed = 0, per_plane = ws(1) + (host_in ? al(px * esz) : 0) + (host_pr ? al(px) : 0);
    bool wait = host_in || host_pr || host_out;                  // the call returns when its host buffers are done with
    for (const HostTable& tb : tables)
        if (tb.host) {
            (tb.per_plane ? per_plane : fixed) += al(tb.doubles * 8);
            wait = wait || tb.per_plane;
        }
    RFI_REQUIRE(fixed + per_plane <= kFlagBudget,
                who + ": one " + std::to_string(c) + " x " + std::to_string(t) + " plane needs " + std::to_string((fixed + per_plane) >> 20) +
                    " MiB of workspace, over the budget of " + std::to_string(kFlagBudget >> 20) + " MiB; planes are not split");
    const int k = (int)std::min<size_t>((size_t)n_planes, (kFlagBudget - fixed) / per_plane);
    const size_t kn = (size_t)k * px;
    Carve cv{static_cast<char*>(ctx->get_scratch(fixed + k * per_plane))};        // (every region of k planes is at most k of one)
    double* d_tb[2] = {nullptr, nullptr};
    for (int e = 0; e < 2; ++e)
        if (tables[e].host && !tables[e].per_plane) {
            d_tb[e] = cv.take<double>(tables[e].doubles);
            RFI_CHECK_HIP(hipMemcpyAsync(d_tb[e], tables[e].host, tables[e].doubles * 8, hipMemcpyHostToDevice, ctx->stream));
        }
    void* d_ws = cv.take<char>(ws(k));
    char* d_in = cv.take<char>(host_in ? kn * esz : 0);
    uint8_t* d_pr = cv.take<uint8_t>(host_pr ? kn : 0);
    for (int e = 0; e < 2; ++e)
        if (tables[e].host && tables[e].per_plane) d_tb[e] = cv.take<double>(tables[e].doubles * k);
    Drain drain{ctx};
    const char* src = static_cast<const char*>(data);
    for (int p0 = 0; p0 < n_planes; p0 += k) {
        const int np = std::min(k, n_planes - p0);
        const size_t off = (size_t)p0 * px, cn = (size_t)np * px;
        const void* in = src + off * esz;
        const uint8_t* pr = prior ? prior + off : nullptr;
        if (host_in) {
            RFI_CHECK_HIP(hipMemcpyAsync(d_in, in, cn * esz, hipMemcpyHostToDevice, ctx->stream));
            in = d_in;
        }
        if (host_pr) {
            RFI_CHECK_HIP(hipMemcpyAsync(d_pr, pr, cn, hipMemcpyHostToDevice, ctx->stream));
            pr = d_pr;
        }
        for (int e = 0; e < 2; ++e)
            if (tables[e].host && tables[e].per_plane)
                RFI_CHECK_HIP(hipMemcpyAsync(d_tb[e], tables[e].host + (size_t)p0 * tables[e].doubles, (size_t)np * tables[e].doubles * 8,
                                             hipMemcpyHostToDevice, ctx->stream));
        uint8_t* dst = host_out ? nullptr : flags_out + off;
        const uint8_t* res = run(in, pr, np, d_ws, d_tb, dst);
        if (res != dst)
            RFI_CHECK_HIP(hipMemcpyAsync(flags_out + off, res, cn, host_out ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (wait) RFI_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    drain.armed = false;
}
}  // namespace

extern "C" {

// ---- statistical baseline flagger (sumthreshold.hip)
int rfi_sumthreshold_ladder(const rfi_sumthreshold_config* cfg, double sigma, int iteration, double* chi_out) {
    return guarded([&] {
        check_st_config(cfg);
        RFI_REQUIRE(chi_out, "sumthreshold_ladder: null output");
        RFI_REQUIRE(iteration >= 0 && iteration < cfg->iterations, "sumthreshold_ladder: iteration out of range");
        sumthreshold_ladder_host(*cfg, sigma, iteration, chi_out);
    });
}
int rfi_sumthreshold_pass(rfi_ctx* ctx, const float* values, int values_mem, const uint8_t* flags_in, int flags_mem, int n_planes,
                          int c, int t, int window, int axis, const double* threshold_host, const double* center_host,
                          uint8_t* flags_out, int out_mem) {
    return guarded([&] {
        RFI_REQUIRE(window >= 1 && window <= st_max_window() && (window & (window - 1)) == 0,
                    "sumthreshold_pass: window must be a power of two in 1 .. 128");
        RFI_REQUIRE(axis == 0 || axis == 1, "sumthreshold_pass: axis must be 0 (frequency) or 1 (time)");
        if (!check_stack("sumthreshold_pass", ctx, n_planes, c, t, {values_mem, flags_mem, out_mem})) return;
        RFI_REQUIRE(values && flags_in && flags_out && threshold_host && center_host, "sumthreshold_pass: null argument");
        const size_t n = (size_t)n_planes * c * t;
        CallScope sc(ctx);
        const float* x = sc.in(values, values_mem, n);
        const uint8_t* fi = sc.in(flags_in, flags_mem, n);
        uint8_t* fo = sc.out(flags_out, out_mem, n);
        RFI_REQUIRE(fi != fo, "sumthreshold_pass: flags_in and flags_out must be different buffers");
        if (window > (axis == 1 ? t : c)) {
            RFI_CHECK_HIP(hipMemcpyAsync(fo, fi, n, hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            const double* th = sc.in(threshold_host, RFI_HOST, (size_t)n_planes);
            const double* ce = sc.in(center_host, RFI_HOST, (size_t)n_planes);
            launch_st_pass(ctx, x, nullptr, fi, fo, n_planes, c, t, window, axis, ce, th, 1, nullptr, 0);
        }
        sc.finish();
    });
}
int rfi_masked_smooth(rfi_ctx* ctx, const float* values, int values_mem, const uint8_t* flags, int flags_mem, int n_planes, int c,
                      int t, const double* weights_t_host, int half_t, const double* weights_f_host, int half_f, float* out,
                      int out_mem) {
    return guarded([&] {
        RFI_REQUIRE(half_t >= 0 && half_f >= 0 && half_t <= (1 << 20) && half_f <= (1 << 20), "masked_smooth: half widths must be in 0 .. 2^20");
        if (!check_stack("masked_smooth", ctx, n_planes, c, t, {values_mem, flags_mem, out_mem})) return;
        RFI_REQUIRE(values && flags && out && weights_t_host && weights_f_host, "masked_smooth: null argument");
        const size_t n = (size_t)n_planes * c * t;
        CallScope sc(ctx);
        const float* x = sc.in(values, values_mem, n);
        const uint8_t* f = sc.in(flags, flags_mem, n);
        float* b = sc.out(out, out_mem, n);
        const double* wt = sc.in(weights_t_host, RFI_HOST, (size_t)2 * half_t + 1);
        const double* wf = sc.in(weights_f_host, RFI_HOST, (size_t)2 * half_f + 1);
        launch_st_smooth(ctx, x, f, n_planes, c, t, wt, half_t, wf, half_f, sc.temp<double>(2 * n), b);
        sc.finish();
    });
}
int rfi_sir_operator(rfi_ctx* ctx, const uint8_t* flags_in, int flags_mem, int n_planes, int c, int t, int axis, int q,
                     uint8_t* flags_out, int out_mem) {
    return guarded([&] {
        RFI_REQUIRE(axis == 0 || axis == 1, "sir_operator: axis must be 0 (frequency) or 1 (time)");
        RFI_REQUIRE(q >= 0 && q <= 1023, "sir_operator: q must be in 0 .. 1023");
        if (!check_stack("sir_operator", ctx, n_planes, c, t, {flags_mem, out_mem})) return;
        RFI_REQUIRE(flags_in && flags_out, "sir_operator: null argument");
        const size_t n = (size_t)n_planes * c * t;
        CallScope sc(ctx);
        const uint8_t* fi = sc.in(flags_in, flags_mem, n);
        uint8_t* fo = sc.out(flags_out, out_mem, n);
        if (q == 0) {
            if (fi != fo) RFI_CHECK_HIP(hipMemcpyAsync(fo, fi, n, hipMemcpyDeviceToDevice, ctx->stream));
        } else {
            launch_st_sir(ctx, fi, fo, n_planes, c, t, axis, q, sc.temp<int>(n));
        }
        sc.finish();
    });
}
int rfi_sumthreshold_flag(rfi_ctx* ctx, const void* data, int data_mem, int dtype, const uint8_t* prior, int prior_mem, int n_planes,
                          int c, int t, const rfi_sumthreshold_config* cfg, const double* weights_t_host,
                          const double* weights_f_host, uint8_t* flags_out, int out_mem) {
    return guarded([&] {
        check_dtype("sumthreshold_flag", dtype, true);
        check_st_config(cfg);
        if (!check_stack("sumthreshold_flag", ctx, n_planes, c, t, {data_mem, prior ? prior_mem : RFI_HOST, out_mem})) return;
        RFI_REQUIRE(data && flags_out && weights_t_host && weights_f_host, "sumthreshold_flag: null argument");
        const HostTable weights[2] = {{weights_t_host, (size_t)2 * cfg->half_t + 1, false}, {weights_f_host, (size_t)2 * cfg->half_f + 1, false}};
        flag_in_groups(ctx, "sumthreshold_flag", data, data_mem, dtype_bytes(dtype), prior, prior_mem, n_planes, c, t, weights, flags_out,
                       out_mem, [&](int k) { return sumthreshold_ws_bytes(k, c, t); },
                       [&](const void* in, const uint8_t* pr, int np, void* ws, const double* const* w, uint8_t* dst) {
                           return launch_sumthreshold_flag(ctx, in, dtype, pr, np, c, t, *cfg, w[0], w[1], ws, dst);
                       });
    });
}

// ---- CASA-style baseline flaggers (casa_flaggers.hip)
int rfi_tfcrop_flag(rfi_ctx* ctx, const void* data, int data_mem, int dtype, const uint8_t* prior, int prior_mem, int n_planes, int c,
                    int t, const rfi_tfcrop_config* cfg, uint8_t* flags_out, int out_mem) {
    return guarded([&] {
        check_dtype("tfcrop_flag", dtype, true);
        RFI_REQUIRE(cfg, "tfcrop_flag: null config");
        RFI_REQUIRE(cfg->ntime >= 1, "tfcrop_flag: ntime must be >= 1");
        RFI_REQUIRE((cfg->timefit == 0 || cfg->timefit == 1) && (cfg->freqfit == 0 || cfg->freqfit == 1),
                    "tfcrop_flag: timefit and freqfit must be 0 (line) or 1 (poly)");
        RFI_REQUIRE(cfg->maxnpieces >= 1, "tfcrop_flag: maxnpieces must be >= 1");
        RFI_REQUIRE(cfg->flagdimension >= RFI_TFCROP_FREQTIME && cfg->flagdimension <= RFI_TFCROP_FREQ, "tfcrop_flag: bad flagdimension");
        RFI_REQUIRE(in_range(cfg->timecutoff, 0.0, 1.0e300) && in_range(cfg->freqcutoff, 0.0, 1.0e300), "tfcrop_flag: cutoffs must be >= 0");
        if (!check_stack("tfcrop_flag", ctx, n_planes, c, t, {data_mem, prior ? prior_mem : RFI_HOST, out_mem})) return;
        RFI_REQUIRE(data && flags_out, "tfcrop_flag: null argument");
        rfi_tfcrop_config cf = *cfg;
        cf.ntime = std::min(cf.ntime, t);
        flag_in_groups(ctx, "tfcrop_flag", data, data_mem, dtype_bytes(dtype), prior, prior_mem, n_planes, c, t, {kNoTable, kNoTable},
                       flags_out, out_mem, [&](int k) { return tfcrop_ws_bytes(k, c, t, cf.ntime); },
                       [&](const void* in, const uint8_t* pr, int np, void* ws, const double* const*, uint8_t*) {
                           return launch_tfcrop_flag(ctx, in, dtype, pr, np, c, t, cf, ws);
                       });
    });
}
int rfi_rflag_flag(rfi_ctx* ctx, const void* data, int data_mem, int dtype, const uint8_t* prior, int prior_mem, int n_planes, int c,
                   int t, const rfi_rflag_config* cfg, const double* timedev_host, const double* freqdev_host, uint8_t* flags_out,
                   int out_mem) {
    return guarded([&] {
        check_dtype("rflag_flag", dtype, false);
        RFI_REQUIRE(cfg, "rflag_flag: null config");
        RFI_REQUIRE(cfg->ntime >= 1, "rflag_flag: ntime must be >= 1");
        RFI_REQUIRE(cfg->winsize >= 1 && cfg->winsize % 2 == 1, "rflag_flag: winsize must be odd and >= 1");
        RFI_REQUIRE(in_range(cfg->timedevscale, 0.0, 1.0e300) && in_range(cfg->freqdevscale, 0.0, 1.0e300), "rflag_flag: scales must be >= 0");
        if (!check_stack("rflag_flag", ctx, n_planes, c, t, {data_mem, prior ? prior_mem : RFI_HOST, out_mem})) return;
        RFI_REQUIRE(data && flags_out, "rflag_flag: null argument");
        rfi_rflag_config cf = *cfg;
        cf.ntime = std::min(cf.ntime, t);
        const HostTable devs[2] = {{timedev_host, (size_t)c, true}, {freqdev_host, 1, true}};
        flag_in_groups(ctx, "rflag_flag", data, data_mem, dtype_bytes(dtype), prior, prior_mem, n_planes, c, t, devs, flags_out, out_mem,
                       [&](int k) { return rflag_ws_bytes(k, c, t, cf.ntime); },
                       [&](const void* in, const uint8_t* pr, int np, void* ws, const double* const* dev, uint8_t*) {
                           return launch_rflag_flag(ctx, in, dtype, pr, np, c, t, cf, dev[0], dev[1], ws);
                       });
    });
}
int rfi_extend_flags(rfi_ctx* ctx, const uint8_t* flags_in, int flags_mem, int n_planes, int c, int t, const rfi_extend_config* cfg,
                     uint8_t* flags_out, int out_mem) {
    return guarded([&] {
        RFI_REQUIRE(cfg, "extend_flags: null config");
        RFI_REQUIRE(cfg->ntime >= 1, "extend_flags: ntime must be >= 1");
        RFI_REQUIRE(in_range(cfg->growtime, 0.0, 100.0) && in_range(cfg->growfreq, 0.0, 100.0),
                    "extend_flags: growtime and growfreq must be in 0 .. 100");
        if (!check_stack("extend_flags", ctx, n_planes, c, t, {flags_mem, out_mem})) return;
        RFI_REQUIRE(flags_in && flags_out, "extend_flags: null argument");
        rfi_extend_config cf = *cfg;
        cf.ntime = std::min(cf.ntime, t);
        flag_in_groups(ctx, "extend_flags", flags_in, flags_mem, 1, nullptr, RFI_HOST, n_planes, c, t, {kNoTable, kNoTable}, flags_out,
                       out_mem, [&](int k) { return extend_ws_bytes(k, c, t); },
                       [&](const void* in, const uint8_t*, int np, void* ws, const double* const*, uint8_t*) {
                           return launch_extend_flags(ctx, static_cast<const uint8_t*>(in), np, c, t, cf, ws);
                       });
    });
}

}  // extern "C"
