// The parameter table every network shares: the layer registry that lays out the flat parameter buffers (params / grads /
// Adam m / Adam v), the per-channel state and dgrad-layout pools and the state_dict entries, and the host access to
// those entries (the rfi_model_* entry functions of api.cpp).
//
// Flat offsets fix the summation order of gradient clipping and the buckets of the gradient exchange, so the layout is
// part of what a step computes: every slot is align4'd, in registration order.
#include "model.hpp"

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <random>

using namespace rfi;

namespace rfi {

void to_lib_conv(const float* oihw, int cout, int cin, int R, std::vector<float>& out, int cin_p) {
    if (cin_p < 0) cin_p = cin;
    out.assign((size_t)R * R * cout * cin_p, 0.0f);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < R * R; ++t)
                out[((size_t)t * cout + co) * cin_p + ci] = oihw[((size_t)co * cin + ci) * R * R + t];
}
void from_lib_conv(const float* lib, int cout, int cin, int R, float* oihw, int cin_p) {
    if (cin_p < 0) cin_p = cin;
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < R * R; ++t)
                oihw[((size_t)co * cin + ci) * R * R + t] = lib[((size_t)t * cout + co) * cin_p + ci];
}
void to_lib_convt(const float* iohw, int cin, int cout, std::vector<float>& out) {
    out.resize((size_t)4 * cout * cin);
    for (int ci = 0; ci < cin; ++ci)
        for (int co = 0; co < cout; ++co)
            for (int t = 0; t < 4; ++t)
                out[((size_t)t * cout + co) * cin + ci] = iohw[((size_t)ci * cout + co) * 4 + t];
}
void from_lib_convt(const float* lib, int cin, int cout, float* iohw) {
    for (int ci = 0; ci < cin; ++ci)
        for (int co = 0; co < cout; ++co)
            for (int t = 0; t < 4; ++t)
                iohw[((size_t)ci * cout + co) * 4 + t] = lib[((size_t)t * cout + co) * cin + ci];
}

}  // namespace rfi

namespace {

size_t flat_slot(rfi_model* m, size_t floats) {
    const size_t off = m->n_flat;
    m->n_flat = align4(m->n_flat + floats);
    return off;
}

void add_entry(rfi_model* m, const std::string& name, EntryKind kind, std::initializer_list<int64_t> dims, int layer,
               size_t off = 0) {
    Entry e;
    e.name = name;
    e.kind = kind;
    e.ndim = (int)dims.size();
    std::copy(dims.begin(), dims.end(), e.dims);
    e.layer = layer;
    e.off = off;
    if (is_parameter(kind)) m->n_params += e.numel();
    m->entry_index[name] = (int)m->entries.size();
    m->entries.push_back(e);
}

// floats of a parameter in the library layout
size_t lib_floats(const rfi_model* m, const Entry& e) {
    return e.kind == EntryKind::ConvWeight ? (size_t)e.dims[2] * e.dims[3] * e.dims[0] * m->convs[e.layer].cin_p : (size_t)e.numel();
}
void to_lib(const rfi_model* m, const Entry& e, const float* src, std::vector<float>& out) {
    if (e.kind == EntryKind::ConvWeight) to_lib_conv(src, (int)e.dims[0], (int)e.dims[1], (int)e.dims[2], out, m->convs[e.layer].cin_p);
    else if (e.kind == EntryKind::ConvTWeight) to_lib_convt(src, (int)e.dims[0], (int)e.dims[1], out);
    else out.assign(src, src + e.numel());
}
void from_lib(const rfi_model* m, const Entry& e, const float* lib, float* out) {
    if (e.kind == EntryKind::ConvWeight) from_lib_conv(lib, (int)e.dims[0], (int)e.dims[1], (int)e.dims[2], out, m->convs[e.layer].cin_p);
    else if (e.kind == EntryKind::ConvTWeight) from_lib_convt(lib, (int)e.dims[0], (int)e.dims[1], out);
    else std::memcpy(out, lib, (size_t)e.numel() * sizeof(float));
}

// the per-channel state a buffer entry lives in (null: not a per-channel entry)
float* chan_slot(const rfi_model* m, const Entry& e) {
    switch (e.kind) {
        case EntryKind::RunningMean: return m->convs[e.layer].running_mean();
        case EntryKind::RunningVar: return m->convs[e.layer].running_var();
        case EntryKind::FrozenBnWeight: return m->convs[e.layer].frozen_weight();
        case EntryKind::FrozenBnBias: return m->convs[e.layer].frozen_bias();
        default: return nullptr;
    }
}

void check_bytes(const Entry& e, size_t bytes) {
    RFI_REQUIRE(bytes == (size_t)e.numel() * sizeof(float),
                "size mismatch for " + e.name + ": expected " + std::to_string(e.numel() * 4) + " bytes, got " +
                    std::to_string(bytes));
}

void upload(rfi_model* m, float* dst, const float* src, size_t n) {
    RFI_CHECK_HIP(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyHostToDevice, m->ctx->stream));
    RFI_CHECK_HIP(hipStreamSynchronize(m->ctx->stream));
}
void download(rfi_model* m, float* dst, const float* src, size_t n) {
    RFI_CHECK_HIP(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToHost, m->ctx->stream));
    RFI_CHECK_HIP(hipStreamSynchronize(m->ctx->stream));
}

}  // namespace

// ------------------------------------------------------------------------------------ registry
int rfi_model::add_conv(ConvBN c) {
    const int ci = (int)convs.size();
    const size_t wn = (size_t)c.R * c.R * c.cin_p * c.cout;
    const bool train_bn = c.has_bn && !c.frozen_bn;
    c.w_off = flat_slot(this, wn);
    c.b_off = flat_slot(this, c.cout);           // (also without a bias: the slot stays 0)
    if (train_bn) {
        c.g_off = flat_slot(this, c.cout);
        c.be_off = flat_slot(this, c.cout);
    }
    c.chan_off = chan_floats;
    chan_floats += align4((size_t)8 * c.cout);
    c.wd_off = wd_floats;
    wd_floats += align4(wn);

    const int64_t co = c.cout;
    if (c.R == 1) {
        RFI_REQUIRE(c.cin_p == c.cin, "1x1 conv " + c.conv_name + ": padded input channels");
        add_entry(this, c.conv_name + ".weight", EntryKind::LinearWeight, {co, c.cin, 1, 1}, ci, c.w_off);
    } else {
        add_entry(this, c.conv_name + ".weight", EntryKind::ConvWeight, {co, c.cin, c.R, c.R}, ci, c.w_off);
    }
    if (c.has_bias) add_entry(this, c.conv_name + ".bias", EntryKind::Bias, {co}, ci, c.b_off);
    if (c.has_bn) {
        const std::string& bn = c.bn_name;
        if (train_bn) {
            add_entry(this, bn + ".weight", EntryKind::BnWeight, {co}, ci, c.g_off);
            add_entry(this, bn + ".bias", EntryKind::BnBias, {co}, ci, c.be_off);
        } else {
            add_entry(this, bn + ".weight", EntryKind::FrozenBnWeight, {co}, ci);
            add_entry(this, bn + ".bias", EntryKind::FrozenBnBias, {co}, ci);
        }
        add_entry(this, bn + ".running_mean", EntryKind::RunningMean, {co}, ci);
        add_entry(this, bn + ".running_var", EntryKind::RunningVar, {co}, ci);
        if (train_bn) add_entry(this, bn + ".num_batches_tracked", EntryKind::NumBatchesTracked, {}, ci);
    }
    convs.push_back(std::move(c));
    return ci;
}

void rfi_model::add_up(const std::string& name, int cin, int cout) {
    UpConv u;
    u.name = name;
    u.cin = cin;
    u.cout = cout;
    const size_t wn = (size_t)4 * cin * cout;
    u.w_off = flat_slot(this, wn);
    u.b_off = flat_slot(this, cout);
    u.wd_off = wd_floats;
    wd_floats += align4(wn);
    add_entry(this, name + ".weight", EntryKind::ConvTWeight, {cin, cout, 2, 2}, -1, u.w_off);
    add_entry(this, name + ".bias", EntryKind::Bias, {cout}, -1, u.b_off);
    ups.push_back(u);
}

void rfi_model::add_head(const std::string& name, int cin) {
    head_w_off = flat_slot(this, (size_t)out_ch * cin);
    head_b_off = flat_slot(this, out_ch);
    add_entry(this, name + ".weight", EntryKind::LinearWeight, {out_ch, cin, 1, 1}, -1, head_w_off);
    add_entry(this, name + ".bias", EntryKind::Bias, {out_ch}, -1, head_b_off);
}

// device state of the registered table: the flat buffers (zeroed), the per-channel state and dgrad-layout pools, the loss
// scalars; then the running statistics of a fresh model
void rfi_model::alloc_state() {
    ctx->activate();
    const size_t bytes = n_flat * sizeof(float);
    params = static_cast<float*>(ctx->alloc(bytes));
    grads = static_cast<float*>(ctx->alloc(bytes));
    adam_m = static_cast<float*>(ctx->alloc(bytes));
    adam_v = static_cast<float*>(ctx->alloc(bytes));
    chan_pool = static_cast<float*>(ctx->alloc(chan_floats * sizeof(float)));
    wd_pool = static_cast<float*>(ctx->alloc(wd_floats * sizeof(float)));
    d_sums = static_cast<double*>(ctx->alloc(kSumsDoubles * sizeof(double)));
    d_scalars = static_cast<float*>(ctx->alloc(8 * sizeof(float)));
    for (float* p : {params, grads, adam_m, adam_v}) RFI_CHECK_HIP(hipMemsetAsync(p, 0, bytes, ctx->stream));
    RFI_CHECK_HIP(hipMemsetAsync(chan_pool, 0, chan_floats * sizeof(float), ctx->stream));
    RFI_CHECK_HIP(hipMemsetAsync(d_sums, 0, kSumsDoubles * sizeof(double), ctx->stream));
    RFI_CHECK_HIP(hipMemsetAsync(d_scalars, 0, 8 * sizeof(float), ctx->stream));
    for (auto& c : convs) {
        c.chan = chan_pool + c.chan_off;
        c.wd = wd_pool + c.wd_off;
    }
    for (auto& u : ups) u.wd = wd_pool + u.wd_off;
    reset_channel_state();
}

void rfi_model::reset_channel_state() {
    for (auto& c : convs) {
        std::vector<float> ch((size_t)8 * c.cout, 0.0f);
        for (int i = 0; i < c.cout; ++i) ch[c.cout + i] = 1.0f;                          // running_var = 1
        if (!c.has_bn)
            for (int i = 0; i < c.cout; ++i) ch[(size_t)4 * c.cout + i] = 1.0f;          // scale = 1, shift = 0
        RFI_CHECK_HIP(hipMemcpyAsync(c.chan, ch.data(), ch.size() * sizeof(float), hipMemcpyHostToDevice,
                                     ctx->stream));
        RFI_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        c.nbt = 0;
    }
}

// ------------------------------------------------------------------------------------ entry access
const Entry& rfi_model::entry(const char* name) const {
    RFI_REQUIRE(name, "null entry name");
    auto it = entry_index.find(name);
    RFI_REQUIRE(it != entry_index.end(), std::string("unexpected key in state_dict: ") + name);
    return entries[it->second];
}

void rfi_model::init_params(uint64_t seed) {
    std::mt19937_64 rng(seed);
    std::vector<float> flat(n_flat, 0.0f);
    auto uni = [&](float bound) {
        return (float)((std::generate_canonical<double, 53>(rng) * 2.0 - 1.0) * bound);
    };
    float last_bound = 0;                        // a bias draws from the bound of the weight before it
    for (const Entry& e : entries) {
        float* v = flat.data() + e.off;
        switch (e.kind) {
            case EntryKind::ConvWeight:
            case EntryKind::ConvTWeight:
            case EntryKind::LinearWeight: {
                // kaiming_uniform(a=sqrt(5)) == U(+-1/sqrt(fan_in)), fan_in = dims[1]*kh*kw
                const double fan_in = (double)e.dims[1] * e.dims[2] * e.dims[3];
                last_bound = (float)(1.0 / std::sqrt(fan_in));
                if (e.kind == EntryKind::ConvWeight) {       // [tap][cout][cin_p], padded channels stay 0
                    const int cin_p = convs[e.layer].cin_p, cin = (int)e.dims[1];
                    for (int64_t r = 0; r < e.dims[2] * e.dims[3] * e.dims[0]; ++r)
                        for (int ci = 0; ci < cin; ++ci) v[r * cin_p + ci] = uni(last_bound);
                } else {
                    for (int64_t i = 0; i < e.numel(); ++i) v[i] = uni(last_bound);   // layout-agnostic iid
                }
                break;
            }
            case EntryKind::Bias:
                for (int64_t i = 0; i < e.numel(); ++i) v[i] = uni(last_bound);
                break;
            case EntryKind::BnWeight:
                std::fill(v, v + e.numel(), 1.0f);
                break;
            default:                             // BatchNorm bias 0; buffers: reset_channel_state
                break;
        }
    }
    upload(this, params, flat.data(), n_flat);
    reset_channel_state();
    RFI_CHECK_HIP(hipMemsetAsync(adam_m, 0, n_flat * sizeof(float), ctx->stream));
    RFI_CHECK_HIP(hipMemsetAsync(adam_v, 0, n_flat * sizeof(float), ctx->stream));
    adam_step = 0;
    weights_changed();
}

void rfi_model::load_entry(const Entry& e, const void* host, size_t bytes) {
    if (e.kind == EntryKind::NumBatchesTracked) {
        RFI_REQUIRE(bytes == sizeof(int64_t), "size mismatch for " + e.name);
        convs[e.layer].nbt = *static_cast<const int64_t*>(host);
        return;
    }
    check_bytes(e, bytes);
    const float* src = static_cast<const float*>(host);
    if (float* dst = chan_slot(this, e)) {
        upload(this, dst, src, (size_t)convs[e.layer].cout);
        frozen_changed();
        return;
    }
    std::vector<float> tmp;
    to_lib(this, e, src, tmp);
    upload(this, params + e.off, tmp.data(), tmp.size());
    weights_changed();
}

void rfi_model::store_entry(const Entry& e, void* host, size_t bytes) {
    if (e.kind == EntryKind::NumBatchesTracked) {
        RFI_REQUIRE(bytes == sizeof(int64_t), "size mismatch for " + e.name);
        *static_cast<int64_t*>(host) = convs[e.layer].nbt;
        return;
    }
    if (const float* src = chan_slot(this, e)) {
        RFI_REQUIRE(bytes == (size_t)e.numel() * sizeof(float), "size mismatch for " + e.name);
        download(this, static_cast<float*>(host), src, (size_t)convs[e.layer].cout);
        return;
    }
    store_flat(params, e, host, bytes);
}

void rfi_model::store_flat(const float* flat, const Entry& e, void* host, size_t bytes) {
    check_bytes(e, bytes);
    if (!is_parameter(e.kind)) throw Error("entry " + e.name + " is not a parameter");
    std::vector<float> tmp(lib_floats(this, e));
    download(this, tmp.data(), flat + e.off, tmp.size());
    from_lib(this, e, tmp.data(), static_cast<float*>(host));
}

void rfi_model::load_adam(const Entry& e, const void* host_m, const void* host_v, size_t bytes) {
    RFI_REQUIRE(bytes == (size_t)e.numel() * sizeof(float), "size mismatch for " + e.name);
    if (!is_parameter(e.kind)) throw Error("entry " + e.name + " is not a parameter");
    std::vector<float> tmp;
    for (auto [src, dst] : {std::pair(host_m, adam_m), std::pair(host_v, adam_v)}) {
        if (!src) continue;
        to_lib(this, e, static_cast<const float*>(src), tmp);
        upload(this, dst + e.off, tmp.data(), tmp.size());
    }
}
