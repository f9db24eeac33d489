// extern "C" surface of librfi_hip.so (declared in include/rfi_hip.h).
#include <dlfcn.h>

#include <algorithm>
#include <cmath>

#include "launch_common.hpp"
#include "model.hpp"
#include "tiling.hpp"

using namespace rfi;

// ------------------------------------------------------------------------------------ errors
namespace rfi {
static thread_local std::string g_last_error;
void set_last_error(const std::string& msg) { g_last_error = msg; }
}  // namespace rfi

// ------------------------------------------------------------------------------------ ctx
void rfi_ctx::activate() const { RFI_CHECK_HIP(hipSetDevice(device)); }

void* rfi_ctx::alloc(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0) bytes = 16;
    RFI_CHECK_HIP(hipMalloc(&p, bytes));
    allocs[p] = bytes;
    return p;
}
void rfi_ctx::release(void* p) {
    if (!p) return;
    auto it = allocs.find(p);
    RFI_REQUIRE(it != allocs.end(), "rfi_free: pointer was not allocated by this context");
    allocs.erase(it);
    RFI_CHECK_HIP(hipFree(p));
}
void* rfi_ctx::upload_table(const void* host, size_t bytes) {
    void* d = alloc(bytes);
    if (bytes) RFI_CHECK_HIP(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, stream));
    RFI_CHECK_HIP(hipStreamSynchronize(stream));
    return d;
}
void* rfi_ctx::get_scratch(size_t bytes) {
    if (bytes > scratch_bytes) {
        if (scratch) {
            RFI_CHECK_HIP(hipStreamSynchronize(stream));
            release(scratch);
        }
        scratch = alloc(bytes);
        scratch_bytes = bytes;
    }
    return scratch;
}
hipEvent_t rfi_ctx::get_event() {
    if (!event_pool.empty()) {
        hipEvent_t e = event_pool.back();
        event_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    RFI_CHECK_HIP(hipEventCreate(&e));
    return e;
}
void rfi_ctx::drain_profile() {
    for (auto& pe : pending) {
        RFI_CHECK_HIP(hipEventSynchronize(pe.b));
        float ms = 0;
        RFI_CHECK_HIP(hipEventElapsedTime(&ms, pe.a, pe.b));
        fam[pe.family].ms += ms;
        launches.push_back({pe.family, (double)ms, pe.flops, pe.bytes, pe.label});
        event_pool.push_back(pe.a);
        event_pool.push_back(pe.b);
    }
    pending.clear();
}

static const char* kFamilyNames[FAM_COUNT] = {"conv_igemm_mfma", "wgrad_igemm_mfma", "conv_direct_valu",
                                              "batchnorm", "elementwise", "slab_reduce", "optimizer",
                                              "preprocess", "metrics", "comm"};

namespace {

// build the model `make` returns; if that throws, the model is deleted without the destructor's frees (everything it
// allocated is tracked by ctx)
template <class Make>
int create_model(const char* fn, rfi_ctx* ctx, rfi_model** out, Make make) {
    return guarded([&] {
        RFI_REQUIRE(ctx && out, std::string(fn) + ": null argument");
        rfi_model* m = make();
        m->ctx = ctx;
        try {
            m->build();
        } catch (...) {
            m->ctx = nullptr;
            delete m;
            throw;
        }
        *out = m;
    });
}

// the plain U-Net (models/unet.py), or null
UNetModel* plain_unet(rfi_model* m) {
    auto* u = dynamic_cast<UNetModel*>(m);
    return u && !u->resnet_encoder ? u : nullptr;
}

// launches on another stream for the life of the scope (profiled launches read ctx->stream)
struct OnStream {
    rfi_ctx* c; hipStream_t old;
    OnStream(rfi_ctx* ctx, hipStream_t s) : c(ctx), old(ctx->stream) { c->stream = s; }
    ~OnStream() { c->stream = old; }
};

}  // namespace

extern "C" {

int rfi_abi_version(void) { return RFI_HIP_ABI_VERSION; }
const char* rfi_last_error(void) { return g_last_error.c_str(); }

int rfi_device_count(int* count) {
    return guarded([&] {
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess) n = 0;
        *count = n;
    });
}

int rfi_ctx_create(int device_id, rfi_ctx** out) {
    return guarded([&] {
        RFI_REQUIRE(out, "rfi_ctx_create: null out pointer");
        int n = 0;
        RFI_CHECK_HIP(hipGetDeviceCount(&n));
        RFI_REQUIRE(device_id >= 0 && device_id < n, "rfi_ctx_create: no such GPU (device " +
                                                         std::to_string(device_id) + " of " + std::to_string(n) + ")");
        auto* c = new rfi_ctx();
        c->device = device_id;
        c->activate();
        RFI_CHECK_HIP(hipGetDeviceProperties(&c->prop, device_id));
        // the main stream carries the dependent chain: highest priority; the side stream fills in
        int pr_least = 0, pr_greatest = 0;
        RFI_CHECK_HIP(hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest));
        RFI_CHECK_HIP(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, pr_greatest));
        c->main_stream = c->stream;
        RFI_CHECK_HIP(hipStreamCreateWithPriority(&c->side_stream, hipStreamNonBlocking, pr_least));
        RFI_CHECK_HIP(hipStreamCreateWithPriority(&c->comm_stream, hipStreamNonBlocking, pr_least));
        RFI_CHECK_HIP(hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming));
        c->side_done.resize(4);
        for (auto& e : c->side_done) RFI_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        if (const char* e = getenv("RFI_NO_OVERLAP")) c->overlap = !(e[0] == '1');
        RFI_CHECK_HIP(hipEventCreate(&c->t0));
        RFI_CHECK_HIP(hipEventCreate(&c->t1));
        RFI_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&c->pinned), 4096, hipHostMallocDefault));
        c->zero_page = c->alloc(4096);
        RFI_CHECK_HIP(hipMemsetAsync(c->zero_page, 0, 4096, c->stream));
        RFI_CHECK_HIP(hipStreamSynchronize(c->stream));
        *out = c;
    });
}

int rfi_ctx_destroy(rfi_ctx* ctx) {
    return guarded([&] {
        if (!ctx) return;
        ctx->activate();
        hipStreamSynchronize(ctx->stream);
        for (auto& pe : ctx->pending) { hipEventDestroy(pe.a); hipEventDestroy(pe.b); }
        for (auto e : ctx->event_pool) hipEventDestroy(e);
        for (auto& kv : ctx->allocs) hipFree(kv.first);
        if (ctx->pinned) hipHostFree(ctx->pinned);
        if (ctx->readback_ev) (void)hipEventDestroy(ctx->readback_ev);
        hipEventDestroy(ctx->t0);
        hipEventDestroy(ctx->t1);
        hipStreamSynchronize(ctx->side_stream);
        hipEventDestroy(ctx->fork_ev);
        for (auto e : ctx->fork_ring) hipEventDestroy(e);
        for (auto e : ctx->side_done) hipEventDestroy(e);
        hipStreamSynchronize(ctx->comm_stream);
        for (auto e : ctx->bucket_ev) hipEventDestroy(e);
        hipStreamDestroy(ctx->comm_stream);
        hipStreamDestroy(ctx->side_stream);
        hipStreamDestroy(ctx->main_stream);
        delete ctx;
    });
}

int rfi_ctx_set_overlap(rfi_ctx* ctx, int enabled) {
    return guarded([&] {
        ctx->activate();
        RFI_CHECK_HIP(hipStreamSynchronize(ctx->main_stream));
        RFI_CHECK_HIP(hipStreamSynchronize(ctx->side_stream));
        ctx->overlap = enabled != 0;
    });
}
int rfi_ctx_synchronize(rfi_ctx* ctx) {
    return guarded([&] {
        ctx->activate();
        RFI_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        if (ctx->side_stream) RFI_CHECK_HIP(hipStreamSynchronize(ctx->side_stream));
        if (ctx->comm_stream) RFI_CHECK_HIP(hipStreamSynchronize(ctx->comm_stream));
    });
}
int rfi_ctx_stream(rfi_ctx* ctx, void** s) {
    return guarded([&] { *s = reinterpret_cast<void*>(ctx->stream); });
}
int rfi_ctx_device_name(rfi_ctx* ctx, char* buf, size_t buflen) {
    return guarded([&] {
        std::string s = std::string(ctx->prop.name) + " " + ctx->prop.gcnArchName + " CUs=" +
                        std::to_string(ctx->prop.multiProcessorCount);
        std::snprintf(buf, buflen, "%s", s.c_str());
    });
}

int rfi_ctx_allocations(rfi_ctx* ctx, int64_t* count, uint64_t* bytes) {
    return guarded([&] {
        RFI_REQUIRE(ctx && count && bytes, "rfi_ctx_allocations: null argument");
        uint64_t b = 0;
        for (const auto& kv : ctx->allocs) b += kv.second;
        *count = (int64_t)ctx->allocs.size();
        *bytes = b;
    });
}

int rfi_malloc(rfi_ctx* ctx, size_t bytes, void** dptr) {
    return guarded([&] {
        ctx->activate();
        *dptr = ctx->alloc(bytes);
    });
}
int rfi_free(rfi_ctx* ctx, void* dptr) {
    return guarded([&] {
        ctx->activate();
        RFI_CHECK_HIP(hipStreamSynchronize(ctx->stream));
        ctx->release(dptr);
    });
}
int rfi_memcpy(rfi_ctx* ctx, void* dst, int dst_mem, const void* src, int src_mem, size_t bytes) {
    return guarded([&] {
        ctx->activate();
        hipMemcpyKind k = (dst_mem == RFI_DEVICE)
                              ? (src_mem == RFI_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice)
                              : (src_mem == RFI_DEVICE ? hipMemcpyDeviceToHost : hipMemcpyHostToHost);
        RFI_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, k, ctx->stream));
        RFI_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    });
}
int rfi_memset(rfi_ctx* ctx, void* dptr, int value, size_t bytes) {
    return guarded([&] {
        ctx->activate();
        RFI_CHECK_HIP(hipMemsetAsync(dptr, value, bytes, ctx->stream));
    });
}

int rfi_timer_start(rfi_ctx* ctx) {
    return guarded([&] {
        ctx->activate();
        RFI_CHECK_HIP(hipEventRecord(ctx->t0, ctx->stream));
    });
}
int rfi_timer_stop(rfi_ctx* ctx, float* elapsed_ms) {
    return guarded([&] {
        ctx->activate();
        RFI_CHECK_HIP(hipEventRecord(ctx->t1, ctx->stream));
        RFI_CHECK_HIP(hipEventSynchronize(ctx->t1));
        RFI_CHECK_HIP(hipEventElapsedTime(elapsed_ms, ctx->t0, ctx->t1));
    });
}

int rfi_profile_enable(rfi_ctx* ctx, int on) {
    return guarded([&] {
        ctx->activate();
        if (!on) ctx->drain_profile();
        ctx->profiling = on != 0;
    });
}
int rfi_profile_reset(rfi_ctx* ctx) {
    return guarded([&] {
        ctx->activate();
        ctx->drain_profile();
        for (auto& f : ctx->fam) f = FamilyStat();
        ctx->launches.clear();
    });
}
int rfi_profile_dump(rfi_ctx* ctx, const char* csv_path) {
    return guarded([&] {
        ctx->activate();
        ctx->drain_profile();
        FILE* f = std::fopen(csv_path, "w");
        RFI_REQUIRE(f, std::string("cannot open ") + csv_path);
        std::fprintf(f, "index,family,label,ms,gflop,tflops,mbytes,gbs\n");
        int i = 0;
        for (auto& l : ctx->launches)
            std::fprintf(f, "%d,%s,%s,%.6f,%.4f,%.3f,%.3f,%.1f\n", i++, kFamilyNames[l.family], l.label.c_str(), l.ms,
                         l.flops * 1e-9, l.ms > 0 ? l.flops / (l.ms * 1e-3) * 1e-12 : 0.0, l.bytes * 1e-6,
                         l.ms > 0 ? l.bytes / (l.ms * 1e-3) * 1e-9 : 0.0);
        std::fclose(f);
    });
}
int rfi_profile_family_count(void) { return FAM_COUNT; }
const char* rfi_profile_family_name(int family) {
    return (family >= 0 && family < FAM_COUNT) ? kFamilyNames[family] : "";
}
int rfi_profile_get(rfi_ctx* ctx, int family, int64_t* launches, double* total_ms, double* flops,
                    double* bytes) {
    return guarded([&] {
        RFI_REQUIRE(family >= 0 && family < FAM_COUNT, "rfi_profile_get: bad family");
        ctx->activate();
        ctx->drain_profile();
        const FamilyStat& f = ctx->fam[family];
        if (launches) *launches = f.launches;
        if (total_ms) *total_ms = f.ms;
        if (flops) *flops = f.flops;
        if (bytes) *bytes = f.bytes;
    });
}

// ------------------------------------------------------------------------------------ model
int rfi_unet_create(rfi_ctx* ctx, int in_channels, int out_channels, int init_features, int depth,
                    rfi_model** out) {
    return create_model("rfi_unet_create", ctx, out,
                        [&] { return new UNetModel(in_channels, out_channels, init_features, depth, false); });
}
int rfi_cnn3_create(rfi_ctx* ctx, int in_channels, int out_channels, int width, rfi_model** out) {
    return create_model("rfi_cnn3_create", ctx, out, [&] { return new Cnn3Model(in_channels, out_channels, width); });
}
int rfi_unet_resnet_create(rfi_ctx* ctx, int in_channels, int out_channels, int init_features, rfi_model** out) {
    return create_model("rfi_unet_resnet_create", ctx, out,
                        [&] { return new UNetModel(in_channels, out_channels, init_features, 4, true); });
}
int rfi_mask_head_create(rfi_ctx* ctx, int in_channels, int conv_layers, int out_channels, rfi_model** out) {
    return create_model("rfi_mask_head_create", ctx, out,
                        [&] { return new ConvHeadModel(in_channels, conv_layers, out_channels, true); });
}
int rfi_box_head_create(rfi_ctx* ctx, int in_features, int hidden, int fc_layers, int num_outputs, rfi_model** out) {
    return create_model("rfi_box_head_create", ctx, out,
                        [&] { return new BoxHeadModel(in_features, hidden, fc_layers, num_outputs); });
}
int rfi_resnet50_fpn_create(rfi_ctx* ctx, int in_channels, int base_width, int fpn_channels, rfi_model** out) {
    return create_model("rfi_resnet50_fpn_create", ctx, out,
                        [&] { return new BackboneModel(in_channels, base_width, fpn_channels); });
}
int rfi_rpn_head_create(rfi_ctx* ctx, int in_channels, int conv_layers, int anchors_per_pixel, rfi_model** out) {
    return create_model("rfi_rpn_head_create", ctx, out, [&] {
        RFI_REQUIRE(anchors_per_pixel > 0 && anchors_per_pixel % 4 == 0, "RPNHead: anchors per pixel must be a positive multiple of 4");
        return new ConvHeadModel(in_channels, conv_layers, 5 * anchors_per_pixel, false);
    });
}
int rfi_model_input_grad(rfi_model* m, float* dx, int dx_mem) {
    return guarded([&] {
        RFI_REQUIRE(m->gx >= 0, "input_grad: only the mask head computes the gradient w.r.t. its input");
        RFI_REQUIRE(m->pN > 0 && dx, "input_grad: no backward pass has run");
        m->ctx->activate();
        const size_t cnt = (size_t)m->pN * m->pH * m->pW * m->in_ch;
        if (dx_mem == RFI_DEVICE) launch_copy_d2d(m->ctx, dx, m->buf(m->gx), cnt * sizeof(float));
        else RFI_CHECK_HIP(hipMemcpyAsync(dx, m->buf(m->gx), cnt * sizeof(float), hipMemcpyDeviceToHost, m->ctx->stream));
        if (dx_mem != RFI_DEVICE || getenv("RFI_SYNC_ALWAYS")) RFI_CHECK_HIP(hipStreamSynchronize(m->ctx->stream));   // (sync_if_host below)
    });
}
int rfi_model_destroy(rfi_model* m) {
    return guarded([&] {
        if (!m) return;
        m->ctx->activate();
        RFI_CHECK_HIP(hipStreamSynchronize(m->ctx->stream));
        delete m;
    });
}

int rfi_model_init(rfi_model* m, uint64_t seed) {
    return guarded([&] {
        m->ctx->activate();
        m->init_params(seed);
    });
}

int rfi_model_entry_count(rfi_model* m, int* n) {
    return guarded([&] { *n = (int)m->entries.size(); });
}
int rfi_model_entry_info(rfi_model* m, int index, const char** name, int* ndim, int64_t dims[4],
                         int* is_int64, int* is_parameter) {
    return guarded([&] {
        RFI_REQUIRE(index >= 0 && index < (int)m->entries.size(), "entry index out of range");
        const Entry& e = m->entries[index];
        if (name) *name = e.name.c_str();
        if (ndim) *ndim = e.ndim;
        if (dims)
            for (int i = 0; i < 4; ++i) dims[i] = i < e.ndim ? e.dims[i] : 1;
        if (is_int64) *is_int64 = e.kind == EntryKind::NumBatchesTracked;
        if (is_parameter) *is_parameter = rfi::is_parameter(e.kind);
    });
}
int rfi_model_param_count(rfi_model* m, int64_t* n) {
    return guarded([&] { *n = m->n_params; });
}

int rfi_model_load_entry(rfi_model* m, const char* name, const void* host, size_t bytes) {
    return guarded([&] {
        m->ctx->activate();
        m->load_entry(m->entry(name), host, bytes);
    });
}
int rfi_model_store_entry(rfi_model* m, const char* name, void* host, size_t bytes) {
    return guarded([&] {
        m->ctx->activate();
        m->store_entry(m->entry(name), host, bytes);
    });
}
int rfi_model_store_grad(rfi_model* m, const char* name, void* host, size_t bytes) {
    return guarded([&] {
        m->ctx->activate();
        m->join_pending_side();
        m->store_flat(m->grads, m->entry(name), host, bytes);
    });
}
int rfi_model_store_adam(rfi_model* m, const char* name, void* host_m, void* host_v, size_t bytes,
                         int64_t* step) {
    return guarded([&] {
        m->ctx->activate();
        const Entry& e = m->entry(name);
        if (host_m) m->store_flat(m->adam_m, e, host_m, bytes);
        if (host_v) m->store_flat(m->adam_v, e, host_v, bytes);
        if (step) *step = m->adam_step;
    });
}
int rfi_model_load_adam(rfi_model* m, const char* name, const void* host_m, const void* host_v,
                        size_t bytes) {
    return guarded([&] {
        m->ctx->activate();
        m->load_adam(m->entry(name), host_m, host_v, bytes);
    });
}
int rfi_model_set_adam_step(rfi_model* m, int64_t step) {
    return guarded([&] {
        RFI_REQUIRE(step >= 0, "Adam step must be >= 0");
        m->adam_step = step;
    });
}

int rfi_model_set_training(rfi_model* m, int training) {
    return guarded([&] { m->training = training != 0; });
}
int rfi_model_set_activation(rfi_model* m, float negative_slope) {
    return guarded([&] {
        UNetModel* u = plain_unet(m);
        RFI_REQUIRE(u, "set_activation: U-Net models only");
        RFI_REQUIRE(negative_slope >= 0.0f && negative_slope < 1.0f, "set_activation: negative_slope must be in [0, 1)");
        u->act_slope = negative_slope;
    });
}
int rfi_model_set_compute_dtype(rfi_model* m, int dtype) {
    return guarded([&] {
        RFI_REQUIRE(dtype >= 0 && dtype <= 4,
                    "set_compute_dtype: 0 native float32 MFMA, 1 bfloat16 (bf16 activations in HBM, plane kernels), "
                    "2 float32 by 3 x bfloat16 splitting in registers (default), 3 the same arithmetic on pre-split "
                    "plane tensors, 4 bfloat16 operands rounded in registers (float32 storage)");
        m->set_compute_dtype(dtype);
    });
}
int rfi_model_set_loss(rfi_model* m, int kind, float alpha, float gamma) {
    return guarded([&] {
        RFI_REQUIRE(kind >= 0 && kind <= 2,
                    "set_loss: 0 (BCE-with-logits + dice), 1 (sigmoid focal loss) or 2 (BCE-with-logits + per-class dice)");
        RFI_REQUIRE(kind != 1 || (gamma >= 0.0f && alpha <= 1.0f), "set_loss: focal needs gamma >= 0 and alpha <= 1");
        RFI_REQUIRE(kind != 2 || m->label_mode == RFI_LABELS_CLASS_BITS,
                    "set_loss: the per-class dice term needs class-bit labels (rfi_model_set_label_mode first)");
        RFI_REQUIRE(kind != 1 || !m->weights_on,
                    "set_loss: the focal loss takes no positive weights (it has alpha); clear them with rfi_model_set_pos_weight(m, NULL, 0) first");
        m->loss_kind = kind;
        m->focal_alpha = alpha;
        m->focal_gamma = gamma;
    });
}
namespace {
void require_masked_scope(rfi_model* m, const char* what) {
    RFI_REQUIRE(plain_unet(m) && !m->head_sigmoid && m->dense_head,
                std::string(what) + ": the ignore bit and positive weights are for UNet, UNetBigger and UNetDifferentActivation (not the "
                                    "sigmoid-head, ResNet-encoder, SimpleCNN or detector models)");
}
}  // namespace
int rfi_model_set_ignore(rfi_model* m, int enabled) {
    return guarded([&] {
        if (enabled) {
            require_masked_scope(m, "set_ignore");
            RFI_REQUIRE(m->label_mode != RFI_LABELS_CLASS_BITS || m->out_ch <= 7,
                        "set_ignore: bit 7 of a class-bit label is the target of channel 7; the ignore bit needs out_channels <= 7");
        }
        m->ignore_on = enabled != 0;
    });
}
int rfi_model_set_pos_weight(rfi_model* m, const float* weights_host, int k) {
    return guarded([&] {
        if (!weights_host || k == 0) {
            m->weights_on = false;
            for (float& w : m->pos_weight) w = 1.0f;
            return;
        }
        require_masked_scope(m, "set_pos_weight");
        RFI_REQUIRE(k == m->out_ch, "set_pos_weight: " + std::to_string(k) + " weights for " + std::to_string(m->out_ch) + " output channels");
        RFI_REQUIRE(k <= 8, "set_pos_weight: at most 8 output channels");
        for (int c = 0; c < k; ++c)
            RFI_REQUIRE(std::isfinite(weights_host[c]) && weights_host[c] >= 0.0f, "set_pos_weight: every weight must be finite and >= 0");
        RFI_REQUIRE(m->loss_kind != 1, "set_pos_weight: the focal loss takes no positive weights (it has alpha)");
        for (int c = 0; c < 8; ++c) m->pos_weight[c] = c < k ? weights_host[c] : 1.0f;
        m->weights_on = true;
    });
}
int rfi_model_set_label_mode(rfi_model* m, int mode) {
    return guarded([&] {
        RFI_REQUIRE(mode == RFI_LABELS_MAP || mode == RFI_LABELS_CLASS_BITS, "set_label_mode: RFI_LABELS_MAP or RFI_LABELS_CLASS_BITS");
        if (mode == RFI_LABELS_CLASS_BITS) {
            RFI_REQUIRE(plain_unet(m) && !m->head_sigmoid,
                        "set_label_mode: class-bit labels are for UNet, UNetBigger and UNetDifferentActivation (not the sigmoid-head, "
                        "ResNet-encoder or SimpleCNN models)");
            RFI_REQUIRE(m->out_ch >= 1 && m->out_ch <= 8, "set_label_mode: class-bit labels need 1 <= out_channels <= 8");
            RFI_REQUIRE(!m->ignore_on || m->out_ch <= 7,
                        "set_label_mode: the ignore bit (rfi_model_set_ignore) is bit 7; class-bit labels then need out_channels <= 7");
        } else if (m->loss_kind == 2) {
            m->loss_kind = 0;         // (the per-class dice term of one class is the reference's loss)
        }
        m->label_mode = mode;
    });
}
int rfi_model_set_head_sigmoid(rfi_model* m, int enabled) {
    return guarded([&] {
        RFI_REQUIRE(plain_unet(m), "set_head_sigmoid: U-Net models only");
        RFI_REQUIRE(!enabled || m->label_mode == RFI_LABELS_MAP, "set_head_sigmoid: not with class-bit labels");
        RFI_REQUIRE(!enabled || !m->masked_loss(), "set_head_sigmoid: not with the ignore bit or positive weights");
        m->head_sigmoid = enabled != 0;
    });
}

namespace {

// a copy on the model's stream: between two device buffers as a kernel (launch_copy_d2d), else hipMemcpyAsync
void copy_on_stream(rfi_ctx* ctx, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (kind == hipMemcpyDeviceToDevice) launch_copy_d2d(ctx, dst, src, bytes);
    else RFI_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, kind, ctx->stream));
}
const float* stage_input(rfi_model* m, const float* x, int x_mem, int n, int h, int w, bool nchw) {
    const size_t cnt = (size_t)n * h * w * m->in_ch;
    const float* dev = x;
    if (x_mem == RFI_HOST) {
        float* st = m->buf(nchw ? m->x_stage2 : m->x_stage);
        RFI_CHECK_HIP(hipMemcpyAsync(st, x, cnt * sizeof(float), hipMemcpyHostToDevice, m->ctx->stream));
        dev = st;
    }
    if (nchw) {
        launch_nchw_to_nhwc(m->ctx, dev, n, m->in_ch, h, w, m->buf(m->x_stage));
        dev = m->buf(m->x_stage);
    }
    return dev;
}
const uint8_t* stage_labels(rfi_model* m, const uint8_t* y, int y_mem, int n, int h, int w) {
    if (y_mem == RFI_DEVICE) return y;
    uint8_t* st = reinterpret_cast<uint8_t*>(m->buf(m->lab_stage));
    const size_t bytes = (size_t)n * h * w * m->out_scale * m->out_scale;
    // (the ResNet-50-FPN backbone prepares no label staging)
    RFI_REQUIRE(m->dense_head, "labels: this model takes no label map (its loss lives outside the model)");
    RFI_CHECK_HIP(hipMemcpyAsync(st, y, bytes, hipMemcpyHostToDevice, m->ctx->stream));
    return st;
}
// Entry points whose every tensor argument is a DEVICE pointer return when their work is enqueued (the caller's next
// call that hands data to the host -- rfi_memcpy, a loss scalar -- synchronises the stream); with a host pointer they
// return when the data is there.  RFI_SYNC_ALWAYS=1: synchronise always (round 2's behaviour).
void sync_if_host(rfi_model* m, int mem_a, int mem_b = RFI_DEVICE) {
    static const bool always = getenv("RFI_SYNC_ALWAYS") != nullptr;
    if (always || mem_a != RFI_DEVICE || mem_b != RFI_DEVICE) RFI_CHECK_HIP(hipStreamSynchronize(m->ctx->stream));
}
void emit_logits(rfi_model* m, float* out, int out_mem, int n, int h, int w, bool nchw) {
    h *= m->out_scale; w *= m->out_scale;         // (the mask head's output map is twice its input map)
    const size_t cnt = (size_t)n * h * w * m->out_ch;
    const float* src = m->buf(m->head_sigmoid ? m->probs : m->logits);   // the model's OUTPUT
    if (nchw && m->out_ch > 1) {
        launch_nhwc_to_nchw(m->ctx, src, n, m->out_ch, h, w, m->buf(m->out_stage));
        src = m->buf(m->out_stage);
    }
    copy_on_stream(m->ctx, out, src, cnt * sizeof(float), out_mem == RFI_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost);
    sync_if_host(m, out_mem);
}
float read_scalar(rfi_model* m, const float* dev) {
    RFI_CHECK_HIP(hipMemcpyAsync(m->ctx->pinned, dev, sizeof(float), hipMemcpyDeviceToHost, m->ctx->stream));
    RFI_CHECK_HIP(hipStreamSynchronize(m->ctx->stream));
    return m->ctx->pinned[0];
}
void check_hyper(const rfi_hyper* hp) {
    RFI_REQUIRE(hp, "null hyper-parameters");
    RFI_REQUIRE(hp->lr >= 0 && hp->eps >= 0 && hp->weight_decay >= 0, "Adam: lr, eps, weight_decay must be >= 0");
    RFI_REQUIRE(hp->beta1 >= 0 && hp->beta1 < 1 && hp->beta2 >= 0 && hp->beta2 < 1, "Adam: betas must be in [0,1)");
}


// The optimiser half of a full training step, shared by rfi_train_step and rfi_train_step_async: when the
// context holds a communicator of more than one rank the flat gradient buffer is summed over the ranks
// (RCCL, on this context's stream) and clip + Adam see the MEAN gradient (grad_scale = 1 / world).
void backward_with_exchange(rfi_model* m, const float* x, const uint8_t* y, int n, int h, int w) {
    struct Flag { rfi_model* m; ~Flag() { m->exchange_in_backward = false; } } flag{m};
    m->exchange_in_backward = true;               // the buckets leave as the backward pass finishes them
    m->backward(x, y, n, h, w);
}
void exchange_and_apply(rfi_model* m, const rfi_hyper& hp) {
    if (m->ctx->exchange_active()) {
        // the buckets were all-reduced on the communication stream while the backward pass ran (rfi_model::
        // bucket_ready); exchange_join makes the main stream wait for the last of them
        m->exchange_join();
        m->apply(hp, 1.0f / (float)m->ctx->exchange_world());
    } else {
        m->apply(hp, 1.0f);
    }
}

}  // namespace

int rfi_model_forward_nhwc(rfi_model* m, const float* x, int x_mem, int n, int h, int w, float* logits,
                           int logits_mem) {
    return guarded([&] {
        m->ctx->activate();
        m->prepare(n, h, w);
        const float* xd = stage_input(m, x, x_mem, n, h, w, false);
        m->forward(xd, n, h, w, m->training);
        emit_logits(m, logits, logits_mem, n, h, w, false);
    });
}
int rfi_model_forward_nchw(rfi_model* m, const float* x, int x_mem, int n, int h, int w, float* logits,
                           int logits_mem) {
    return guarded([&] {
        m->ctx->activate();
        m->prepare(n, h, w);
        const float* xd = stage_input(m, x, x_mem, n, h, w, true);
        m->forward(xd, n, h, w, m->training);
        emit_logits(m, logits, logits_mem, n, h, w, true);
    });
}

int rfi_train_forward_backward(rfi_model* m, const float* x, int x_mem, const uint8_t* labels,
                               int labels_mem, int n, int h, int w, float* loss_out) {
    return guarded([&] {
        m->ctx->activate();
        m->prepare(n, h, w);
        const float* xd = stage_input(m, x, x_mem, n, h, w, false);
        const uint8_t* yd = stage_labels(m, labels, labels_mem, n, h, w);
        m->forward(xd, n, h, w, true);
        m->loss_forward(yd, n, h, w);
        m->backward(xd, yd, n, h, w);
        if (loss_out) *loss_out = m->last_loss = read_scalar(m, m->d_scalars);
    });
}
int rfi_train_apply(rfi_model* m, const rfi_hyper* hp, float grad_scale, float* grad_norm_out) {
    return guarded([&] {
        check_hyper(hp);
        m->ctx->activate();
        RFI_REQUIRE(m->pN > 0, "rfi_train_apply: no gradients (call rfi_train_forward_backward first)");
        m->apply(*hp, grad_scale);
        if (grad_norm_out) *grad_norm_out = m->last_norm = read_scalar(m, m->d_scalars + 1);
    });
}
int rfi_train_step(rfi_model* m, const float* x, int x_mem, const uint8_t* labels, int labels_mem,
                   int n, int h, int w, const rfi_hyper* hp, float* loss_out) {
    return guarded([&] {
        check_hyper(hp);
        m->ctx->activate();
        m->prepare(n, h, w);
        const float* xd = stage_input(m, x, x_mem, n, h, w, false);
        const uint8_t* yd = stage_labels(m, labels, labels_mem, n, h, w);
        m->forward(xd, n, h, w, true);
        m->loss_forward(yd, n, h, w);
        backward_with_exchange(m, xd, yd, n, h, w);
        exchange_and_apply(m, *hp);
        RFI_CHECK_HIP(hipMemcpyAsync(m->ctx->pinned, m->d_scalars, 2 * sizeof(float), hipMemcpyDeviceToHost,
                                     m->ctx->stream));
        RFI_CHECK_HIP(hipStreamSynchronize(m->ctx->stream));
        m->last_loss = m->ctx->pinned[0];
        m->last_norm = m->ctx->pinned[1];
        if (loss_out) *loss_out = m->last_loss;
    });
}
int rfi_train_step_async(rfi_model* m, const float* x_dev, const uint8_t* labels_dev, int n, int h,
                         int w, const rfi_hyper* hp) {
    return guarded([&] {
        check_hyper(hp);
        m->ctx->activate();
        m->prepare(n, h, w);
        m->forward(x_dev, n, h, w, true);
        m->loss_forward(labels_dev, n, h, w);
        backward_with_exchange(m, x_dev, labels_dev, n, h, w);
        exchange_and_apply(m, *hp);
    });
}
int rfi_model_backward_dlogits(rfi_model* m, const float* x, int x_mem, const float* dlogits, int dlogits_mem, int n, int h,
                               int w) {
    return guarded([&] {
        RFI_REQUIRE(m->gx >= 0, "backward_dlogits: mask / RPN / box heads only");
        RFI_REQUIRE(m->pN == n && m->pH == h && m->pW == w, "backward_dlogits: run the forward pass on this input first");
        m->ctx->activate();
        const float* xd = stage_input(m, x, x_mem, n, h, w, false);
        const size_t cnt = (size_t)n * h * w * m->out_scale * m->out_scale * m->out_ch;
        copy_on_stream(m->ctx, m->buf(m->dlogits), dlogits, cnt * sizeof(float),
                       dlogits_mem == RFI_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
        struct Flag { rfi_model* m; ~Flag() { m->ext_dlogits = false; } } flag{m};
        m->ext_dlogits = true;
        m->backward(xd, nullptr, n, h, w);
        sync_if_host(m, x_mem, dlogits_mem);
    });
}
int rfi_backbone_forward(rfi_model* m, const float* x, int x_mem, int n, int h, int w, float* const feats[5], int feats_mem) {
    return guarded([&] {
        auto* b = dynamic_cast<BackboneModel*>(m);
        RFI_REQUIRE(b && feats, "backbone_forward: ResNet-50-FPN models only");
        m->ctx->activate();
        m->prepare(n, h, w);
        const float* xd = stage_input(m, x, x_mem, n, h, w, false);
        m->forward(xd, n, h, w, false);
        for (int i = 0; i < 5; ++i) {
            if (!feats[i]) continue;
            const int lvl = i + 2;
            const size_t cnt = (size_t)n * (h >> lvl) * (w >> lvl) * m->out_ch;
            copy_on_stream(m->ctx, feats[i], m->buf(i < 4 ? b->fP[i] : b->fP6), cnt * sizeof(float),
                           feats_mem == RFI_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost);
        }
        sync_if_host(m, x_mem, feats_mem);
    });
}
int rfi_backbone_backward(rfi_model* m, const float* x, int x_mem, int n, int h, int w, const float* const dfeats[5], int dfeats_mem) {
    return guarded([&] {
        auto* b = dynamic_cast<BackboneModel*>(m);
        RFI_REQUIRE(b && dfeats, "backbone_backward: ResNet-50-FPN models only");
        RFI_REQUIRE(m->pN == n && m->pH == h && m->pW == w, "backbone_backward: run the forward pass on this input first");
        m->ctx->activate();
        const float* xd = stage_input(m, x, x_mem, n, h, w, false);
        for (int i = 0; i < 5; ++i) {
            const int lvl = i + 2;
            const size_t cnt = (size_t)n * (h >> lvl) * (w >> lvl) * m->out_ch;
            float* dst = m->buf(i < 4 ? b->fdP[i] : b->fdP6);
            if (dfeats[i])
                copy_on_stream(m->ctx, dst, dfeats[i], cnt * sizeof(float),
                               dfeats_mem == RFI_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
            else
                RFI_CHECK_HIP(hipMemsetAsync(dst, 0, cnt * sizeof(float), m->ctx->stream));
        }
        m->backward(xd, nullptr, n, h, w);
        sync_if_host(m, x_mem, dfeats_mem);
    });
}
int rfi_model_last_loss(rfi_model* m, float* loss_out, float* grad_norm_out) {
    return guarded([&] {
        m->ctx->activate();
        RFI_CHECK_HIP(hipMemcpyAsync(m->ctx->pinned, m->d_scalars, 2 * sizeof(float), hipMemcpyDeviceToHost,
                                     m->ctx->stream));
        RFI_CHECK_HIP(hipStreamSynchronize(m->ctx->stream));
        if (loss_out) *loss_out = m->ctx->pinned[0];
        if (grad_norm_out) *grad_norm_out = m->ctx->pinned[1];
    });
}
int rfi_model_loss(rfi_model* m, const float* x, int x_mem, const uint8_t* labels, int labels_mem, int n,
                   int h, int w, float* loss_out) {
    return guarded([&] {
        m->ctx->activate();
        m->prepare(n, h, w);
        const float* xd = stage_input(m, x, x_mem, n, h, w, false);
        const uint8_t* yd = stage_labels(m, labels, labels_mem, n, h, w);
        m->forward(xd, n, h, w, m->training);
        m->loss_forward(yd, n, h, w);
        if (loss_out) *loss_out = read_scalar(m, m->d_scalars);
    });
}

int rfi_model_eval_batch(rfi_model* m, const float* x, int x_mem, const uint8_t* labels, int labels_mem, int n,
                         int h, int w, float threshold, int64_t* tp, int64_t* fp, int64_t* fn) {
    return guarded([&] {
        RFI_REQUIRE(m->out_ch == 1, "eval_batch: defined for out_channels == 1");
        RFI_REQUIRE(m->label_mode == RFI_LABELS_MAP, "eval_batch: class-bit labels are counted by rfi_model_eval_batch_classes");
        m->ctx->activate();
        m->prepare(n, h, w);
        const float* xd = stage_input(m, x, x_mem, n, h, w, false);
        const uint8_t* yd = stage_labels(m, labels, labels_mem, n, h, w);
        m->forward(xd, n, h, w, m->training);
        const int64_t cnt = (int64_t)n * h * w * m->out_scale * m->out_scale;
        if (m->ignore_on) {           // the counts over the pixels whose label has bit 7 clear
            CallScope sc(m->ctx);
            auto* ws = sc.temp<unsigned long long>(class_confusion_ws_words(1));
            unsigned long long h3[3];
            launch_masked_confusion(m->ctx, m->buf(m->logits), yd, cnt, 1, threshold, true, true, ws, sc.out(h3, RFI_HOST, 3));
            sc.finish();
            *tp = (int64_t)h3[0]; *fp = (int64_t)h3[1]; *fn = (int64_t)h3[2];
            return;
        }
        uint8_t* mask = reinterpret_cast<uint8_t*>(m->buf(m->out_stage));      // cnt bytes fit (cnt floats)
        // evaluate_model.py:44-47 thresholds sigmoid(model output), whatever the model returns
        launch_threshold(m->ctx, m->buf(m->head_sigmoid ? m->probs : m->logits), cnt, threshold, mask);
        auto* d3 = reinterpret_cast<unsigned long long*>(m->d_sums + 5);      // 3 spare 64-bit words
        launch_confusion(m->ctx, mask, RFI_U8, yd, RFI_U8, cnt, d3);
        unsigned long long h3[3];
        RFI_CHECK_HIP(hipMemcpyAsync(h3, d3, sizeof(h3), hipMemcpyDeviceToHost, m->ctx->stream));
        RFI_CHECK_HIP(hipStreamSynchronize(m->ctx->stream));
        *tp = (int64_t)h3[0]; *fp = (int64_t)h3[1]; *fn = (int64_t)h3[2];
    });
}

int rfi_model_eval_batch_classes(rfi_model* m, const float* x, int x_mem, const uint8_t* labels, int labels_mem, int n, int h,
                                 int w, float threshold, int64_t* counts) {
    return guarded([&] {
        RFI_REQUIRE(m->label_mode == RFI_LABELS_CLASS_BITS, "eval_batch_classes: the model's labels are not class bits");
        RFI_REQUIRE(counts, "eval_batch_classes: null argument");
        m->ctx->activate();
        m->prepare(n, h, w);
        const float* xd = stage_input(m, x, x_mem, n, h, w, false);
        const uint8_t* yd = stage_labels(m, labels, labels_mem, n, h, w);
        m->forward(xd, n, h, w, m->training);
        const int K = m->out_ch;
        CallScope sc(m->ctx);
        auto* ws = sc.temp<unsigned long long>(class_confusion_ws_words(K));
        static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counts are copied as they are");
        auto* out = reinterpret_cast<unsigned long long*>(sc.out(counts, RFI_HOST, (size_t)K * 3));
        if (m->ignore_on) launch_masked_confusion(m->ctx, m->buf(m->logits), yd, (int64_t)n * h * w, K, threshold, false, true, ws, out);
        else launch_class_confusion(m->ctx, m->buf(m->logits), yd, (int64_t)n * h * w, K, threshold, ws, out);
        sc.finish();
    });
}

int rfi_model_eval_sweep(rfi_model* m, const float* x, int x_mem, const uint8_t* labels, int labels_mem, int n, int h,
                         int w, const float* thresholds_host, int n_thresholds, int64_t* counts_host) {
    return guarded([&] {
        RFI_REQUIRE(m->out_ch == 1 && m->label_mode == RFI_LABELS_MAP, "eval_sweep: defined for out_channels == 1 and label maps");
        RFI_REQUIRE(!m->ignore_on,
                    "eval_sweep: not while the ignore bit is on (the sweep pools every pixel); sweep the valid pixels with "
                    "rfi_threshold_sweep on prob[valid], truth[valid]");
        RFI_REQUIRE(thresholds_host && counts_host, "eval_sweep: null argument");
        check_sweep_thresholds(thresholds_host, n_thresholds);
        m->ctx->activate();
        m->prepare(n, h, w);
        const float* xd = stage_input(m, x, x_mem, n, h, w, false);
        const uint8_t* yd = stage_labels(m, labels, labels_mem, n, h, w);
        m->forward(xd, n, h, w, m->training);
        const int64_t cnt = (int64_t)n * h * w * m->out_scale * m->out_scale;
        std::vector<unsigned long long> hist(2 * ((size_t)n_thresholds + 1));
        CallScope sc(m->ctx);
        const float* dthr = sc.in(thresholds_host, RFI_HOST, (size_t)n_thresholds);
        // what eval_batch thresholds: sigmoid of the model's output, whatever the model returns (evaluate_model.py:44-47)
        launch_threshold_sweep(m->ctx, m->buf(m->head_sigmoid ? m->probs : m->logits), RFI_VALUES_LOGITS, yd, RFI_U8, 1, cnt,
                               dthr, n_thresholds, sc.out(hist.data(), RFI_HOST, hist.size()));
        sc.finish();
        threshold_sweep_counts(hist.data(), 1, n_thresholds, counts_host);
    });
}

int rfi_model_grad_accumulate(rfi_model* m, int phase) {
    return guarded([&] {
        RFI_REQUIRE(phase >= 0 && phase <= 2, "grad_accumulate: phase 0 (begin), 1 (add the current gradients), 2 (end: sum -> gradients)");
        m->ctx->activate();
        m->join_pending_side();
        const size_t bytes = m->n_flat * sizeof(float);
        if (!m->grad_acc) m->grad_acc = static_cast<float*>(m->ctx->alloc(bytes));
        if (phase == 0) RFI_CHECK_HIP(hipMemsetAsync(m->grad_acc, 0, bytes, m->ctx->stream));
        else if (phase == 1) launch_add_inplace(m->ctx, m->grad_acc, m->grads, (int64_t)m->n_flat);
        else launch_copy_d2d(m->ctx, m->grads, m->grad_acc, bytes);
    });
}
int rfi_model_grad_buffer(rfi_model* m, float** dptr, int64_t* n_floats) {
    return guarded([&] {
        m->ctx->activate();
        m->join_pending_side();                   // (the caller is about to read or reduce the gradients)
        *dptr = m->grads;
        *n_floats = (int64_t)m->n_flat;
    });
}
int rfi_model_param_buffer(rfi_model* m, float** dptr, int64_t* n_floats) {
    return guarded([&] {
        *dptr = m->params;
        *n_floats = (int64_t)m->n_flat;
    });
}

int rfi_model_debug_tensor(rfi_model* m, const char* name, float* host, size_t host_floats,
                           int64_t* n_floats) {
    return guarded([&] {
        m->ctx->activate();
        RFI_REQUIRE(name && m->pN > 0, "debug_tensor: no prepared shape");
        std::string s(name);
        const bool pad = s.size() > 4 && s.compare(s.size() - 4, 4, ":pad") == 0;      // "<name>:pad": the padding lanes of a plane tensor
        std::string core = pad ? s.substr(0, s.size() - 4) : s, base = core;
        int idx = -1;
        auto dot = core.find('.');
        if (dot != std::string::npos) {
            base = core.substr(0, dot);
            idx = std::stoi(core.substr(dot + 1));
        }
        const float* src = nullptr;
        size_t n = 0;
        CallScope sc(m->ctx);                     // (float32 copies of bfloat16 tensors live until the copy to the host is done)
        const size_t M1 = (size_t)m->pN * m->pH * m->pW * m->out_scale * m->out_scale;     // pixels of the OUTPUT map
        RFI_REQUIRE(!pad || (base != "logits" && base != "dlogits" && base != "chan"), "debug_tensor: this tensor has no padding lanes");
        if (base == "logits") { src = m->buf(m->logits); n = M1 * m->out_ch; }
        else if (base == "dlogits") { src = m->buf(m->dlogits); n = M1 * m->out_ch; }
        else if (base == "chan") {
            RFI_REQUIRE(idx >= 0 && idx < (int)m->convs.size(), "debug_tensor: conv index out of range");
            src = m->convs[idx].chan;
            n = (size_t)8 * m->convs[idx].cout;
        } else {
            m->debug_tensor(s, base, idx, host != nullptr, sc, src, n);     // (the U-Net's tensors)
        }
        if (n_floats) *n_floats = (int64_t)n;
        if (host && n) {
            RFI_REQUIRE(host_floats >= n, "debug_tensor: host buffer too small");
            RFI_CHECK_HIP(hipMemcpyAsync(host, src, n * sizeof(float), hipMemcpyDeviceToHost, m->ctx->stream));
            RFI_CHECK_HIP(hipStreamSynchronize(m->ctx->stream));
        }
    });
}

int rfi_model_algorithmic_flops(rfi_model* m, int n, int h, int w, double* fwd, double* step) {
    return guarded([&] {
        double f = 0, st = 0;
        m->algorithmic_flops(n, h, w, f, st);
        if (fwd) *fwd = f;
        if (step) *step = st;
    });
}

// ------------------------------------------------------------------------------------ RCCL
struct Id128 { char bytes[128]; };   // ncclUniqueId is passed BY VALUE to ncclCommInitRank
namespace {

struct NcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, Id128, int) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
NcclApi g_nccl;

void load_nccl() {
    if (g_nccl.lib) return;
    const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
    for (const char* nm : names) {
        g_nccl.lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
        if (g_nccl.lib) break;
    }
    RFI_REQUIRE(g_nccl.lib, std::string("cannot dlopen librccl.so: ") + dlerror());
    auto sym = [&](const char* s) {
        void* p = dlsym(g_nccl.lib, s);
        RFI_REQUIRE(p, std::string("librccl.so lacks symbol ") + s);
        return p;
    };
    g_nccl.GetUniqueId = reinterpret_cast<decltype(g_nccl.GetUniqueId)>(sym("ncclGetUniqueId"));
    g_nccl.CommInitRank = reinterpret_cast<decltype(g_nccl.CommInitRank)>(sym("ncclCommInitRank"));
    g_nccl.AllReduce = reinterpret_cast<decltype(g_nccl.AllReduce)>(sym("ncclAllReduce"));
    g_nccl.CommDestroy = reinterpret_cast<decltype(g_nccl.CommDestroy)>(sym("ncclCommDestroy"));
    g_nccl.GetErrorString = reinterpret_cast<decltype(g_nccl.GetErrorString)>(sym("ncclGetErrorString"));
}
void nccl_check(int rc, const char* what) {
    if (rc != 0) throw Error(std::string(what) + " failed: " + g_nccl.GetErrorString(rc));
}
}  // namespace

int rfi_comm_unique_id(void* id_buf128) {
    return guarded([&] {
        load_nccl();
        nccl_check(g_nccl.GetUniqueId(id_buf128), "ncclGetUniqueId");
    });
}
int rfi_comm_init(rfi_ctx* ctx, const void* id_buf128, int rank, int world_size) {
    return guarded([&] {
        RFI_REQUIRE(world_size >= 1 && rank >= 0 && rank < world_size, "rfi_comm_init: bad rank/world");
        load_nccl();
        ctx->activate();
        Id128 id;
        std::memcpy(id.bytes, id_buf128, 128);
        void* comm = nullptr;
        nccl_check(g_nccl.CommInitRank(&comm, world_size, id, rank), "ncclCommInitRank");
        ctx->nccl_comm = comm;
        ctx->rank = rank;
        ctx->world = world_size;
    });
}
int rfi_comm_destroy(rfi_ctx* ctx) {
    return guarded([&] {
        if (ctx->nccl_comm) {
            ctx->activate();
            (void)hipStreamSynchronize(ctx->stream);
            if (ctx->main_stream) (void)hipStreamSynchronize(ctx->main_stream);
            if (ctx->side_stream) (void)hipStreamSynchronize(ctx->side_stream);      // (weight gradients feed the buckets)
            if (ctx->comm_stream) (void)hipStreamSynchronize(ctx->comm_stream);
            nccl_check(g_nccl.CommDestroy(ctx->nccl_comm), "ncclCommDestroy");
            ctx->nccl_comm = nullptr;
            ctx->world = 1;
        }
    });
}
namespace {
void comm_allreduce_sum(rfi_ctx* ctx, float* dptr, int64_t count) {
    RFI_REQUIRE(ctx->nccl_comm, "rfi_comm_allreduce: communicator not initialised");
    ctx->activate();
    ProfScope ps(ctx, FAM_COMM, 0, (double)count * 4);
    // ncclFloat32 = 7, ncclSum = 0
    nccl_check(g_nccl.AllReduce(dptr, dptr, (size_t)count, 7, 0, ctx->nccl_comm, ctx->stream), "ncclAllReduce");
}
}  // namespace
int rfi_comm_allreduce_sum_f32(rfi_ctx* ctx, float* dptr, int64_t count) {
    return guarded([&] { comm_allreduce_sum(ctx, dptr, count); });
}
int rfi_comm_emulate(rfi_ctx* ctx, int world) {
    return guarded([&] {
        RFI_REQUIRE(world == 0 || world >= 2, "rfi_comm_emulate: world must be 0 (off) or >= 2");
        RFI_REQUIRE(!(ctx->nccl_comm && ctx->world > 1), "rfi_comm_emulate: a real communicator is active");
        ctx->activate();
        RFI_CHECK_HIP(hipStreamSynchronize(ctx->main_stream));
        ctx->comm_emulate = world;
    });
}
}  // extern "C"
namespace rfi {
// one bucket of the gradient exchange, on the context's communication stream (the caller orders it by events)
void comm_bucket_allreduce(rfi_ctx* ctx, float* dptr, int64_t count) {
    OnStream on(ctx, ctx->comm_stream);
    if (ctx->comm_emulate > 1) {
        launch_scale_inplace(ctx, dptr, count, (float)ctx->comm_emulate);
        return;
    }
    load_nccl();
    ProfScope ps(ctx, FAM_COMM, 0, (double)count * 4);
    nccl_check(g_nccl.AllReduce(dptr, dptr, (size_t)count, 7, 0, ctx->nccl_comm, ctx->comm_stream), "ncclAllReduce");
}
}  // namespace rfi
extern "C" {
int rfi_model_allreduce_grads(rfi_model* m) {
    {
        const int rc = guarded([&] { m->ctx->activate(); m->join_pending_side(); });
        if (rc) return rc;
    }
    if (m->ctx->comm_emulate > 1)          // rfi_comm_emulate: the explicit exchange of the split API is emulated like the buckets
        return guarded([&] {
            m->ctx->activate();
            launch_scale_inplace(m->ctx, m->grads, (int64_t)m->n_flat, (float)m->ctx->comm_emulate);
        });
    return rfi_comm_allreduce_sum_f32(m->ctx, m->grads, (int64_t)m->n_flat);
}

// ------------------------------------------------------------------------------------ preprocessing / metrics
int rfi_preprocess_patches(rfi_ctx* ctx, const void* patches, int patches_mem, int dtype, int n,
                           int ps_h, int ps_w, float* out_nhwc, int out_mem) {
    return guarded([&] {
        RFI_REQUIRE(n >= 0 && ps_h > 0 && ps_w > 0, "preprocess: bad shape");
        if (n == 0) return;
        ctx->activate();
        const size_t px = (size_t)n * ps_h * ps_w;
        CallScope sc(ctx);                  // (holds nothing with device pointers only: the call stays asynchronous)
        const void* din = sc.in(patches, patches_mem, px * dtype_bytes(dtype));
        float* dout = sc.out(out_nhwc, out_mem, px * 3);
        void* mm = ctx->get_scratch((size_t)n * 4 * sizeof(unsigned long long));
        launch_preprocess(ctx, din, dtype, n, ps_h, ps_w, static_cast<float*>(mm), dout);
        sc.finish();
    });
}

namespace {
void check_table(const rfi_patch_src* t, int n, int n_planes, int c, int tt, int ps, const char* who = "preprocess_gather") {
    const std::string w(who);
    RFI_REQUIRE(n_planes > 0 && c > 0 && tt > 0 && ps > 0, w + ": bad shape");
    RFI_REQUIRE((int64_t)n_planes * c * tt < ((int64_t)1 << 40), w + ": waterfall too large");
    for (int i = 0; i < n; ++i) {
        const rfi_patch_src& e = t[i];
        RFI_REQUIRE(e.plane >= 0 && e.plane < n_planes && e.view >= 0 && e.view <= 3 && e.row0 >= 0 && e.col0 >= 0,
                    w + ": bad table entry " + std::to_string(i));
    }
}
}  // namespace

int rfi_patch_any_flag(rfi_ctx* ctx, const uint8_t* flags, int flags_mem, int n_planes, int c, int t,
                       const rfi_patch_src* table_host, int n, int ps, uint8_t* any_out_host) {
    return guarded([&] {
        RFI_REQUIRE(n >= 0 && flags && (n == 0 || (table_host && any_out_host)), "patch_any_flag: null argument");
        if (n == 0) return;
        check_table(table_host, n, n_planes, c, t, ps);
        ctx->activate();
        std::vector<unsigned> h((size_t)n);
        CallScope sc(ctx);
        const uint8_t* fl = sc.in(flags, flags_mem, (size_t)n_planes * c * t);
        const rfi_patch_src* tb = sc.in(table_host, RFI_HOST, (size_t)n);
        launch_patch_any_flag(ctx, fl, tb, c, t, n, ps, sc.out(h.data(), RFI_HOST, (size_t)n));
        sc.finish();
        for (int i = 0; i < n; ++i) any_out_host[i] = h[(size_t)i] ? 1 : 0;
    });
}

int rfi_preprocess_gather(rfi_ctx* ctx, const void* planes, int planes_mem, int dtype, int n_planes, int c,
                          int t, const uint8_t* flags, int flags_mem, const rfi_patch_src* table_host, int n,
                          int ps, float* out_nhwc, int out_mem, uint8_t* out_labels, int labels_mem) {
    return guarded([&] {
        RFI_REQUIRE(n >= 0 && planes && (n == 0 || (table_host && out_nhwc)), "preprocess_gather: null argument");
        RFI_REQUIRE(dtype >= RFI_C128 && dtype <= RFI_F32, "preprocess_gather: unknown dtype");
        RFI_REQUIRE(!out_labels || flags, "preprocess_gather: labels requested without flags");
        if (n == 0) return;
        check_table(table_host, n, n_planes, c, t, ps);
        ctx->activate();
        const size_t px = (size_t)n * ps * ps, plane_px = (size_t)n_planes * c * t;
        CallScope sc(ctx);
        const void* pl = sc.in(planes, planes_mem, plane_px * dtype_bytes(dtype));
        const uint8_t* fl = sc.in(flags, flags_mem, plane_px);
        const rfi_patch_src* tb = sc.in(table_host, RFI_HOST, (size_t)n);
        float* dout = sc.out(out_nhwc, out_mem, px * 3);
        uint8_t* dlab = sc.out(out_labels, labels_mem, px);
        void* mm = ctx->get_scratch((size_t)n * 4 * sizeof(unsigned long long));
        launch_preprocess(ctx, pl, dtype, n, ps, ps, static_cast<float*>(mm), dout, tb, c, t);
        if (out_labels) launch_gather_labels(ctx, fl, tb, c, t, n, ps, dlab);
        sc.finish();
    });
}

int rfi_norm_gather(rfi_ctx* ctx, const void* planes, int planes_mem, int dtype, int n_samples, int c, int t,
                    const rfi_patch_src* table_host, int n, int ps, double centre, double scale,
                    const double (*params_host)[2], float* out_nhwc, int out_mem) {
    return guarded([&] {
        RFI_REQUIRE(ctx && n >= 0 && planes && (n == 0 || (table_host && out_nhwc)), "norm_gather: null argument");
        RFI_REQUIRE(dtype == RFI_C128 || dtype == RFI_C64, "norm_gather: planes must be complex128 or complex64");
        if (n == 0) return;
        check_table(table_host, n, n_samples, c, t, ps, "norm_gather");
        RFI_REQUIRE((int64_t)n_samples * 4 * c * t < ((int64_t)1 << 40), "norm_gather: waterfall too large");
        ctx->activate();
        CallScope sc(ctx);
        const void* pl = sc.in(planes, planes_mem, (size_t)n_samples * 4 * c * t * dtype_bytes(dtype));
        const rfi_patch_src* tb = sc.in(table_host, RFI_HOST, (size_t)n);
        const double* pr = sc.in(params_host ? params_host[0] : nullptr, RFI_HOST, (size_t)n_samples * 2);
        float* dout = sc.out(out_nhwc, out_mem, (size_t)n * ps * ps * 8);
        launch_pol_gather(ctx, pl, dtype, c, t, tb, n, ps, centre, scale, pr, dout);
        sc.finish();
    });
}

int rfi_valid_gather(rfi_ctx* ctx, const void* planes, int planes_mem, int dtype, int n_samples, int c, int t,
                     const rfi_patch_src* table_host, int n, int ps, double centre, double scale,
                     const double (*params_host)[2], const uint8_t* flags, int flags_mem, int flags_form, float fill,
                     float* out_nhwc, int out_mem) {
    return guarded([&] {
        RFI_REQUIRE(ctx && n >= 0 && planes && (n == 0 || (table_host && out_nhwc)), "valid_gather: null argument");
        RFI_REQUIRE(dtype == RFI_C128 || dtype == RFI_C64, "valid_gather: planes must be complex128 or complex64");
        RFI_REQUIRE(flags_form == RFI_VALID_FLAGS_POL || flags_form == RFI_VALID_FLAGS_BASELINE, "valid_gather: bad flags form");
        if (n == 0) return;
        check_table(table_host, n, n_samples, c, t, ps, "valid_gather");
        RFI_REQUIRE((int64_t)n_samples * 4 * c * t < ((int64_t)1 << 40), "valid_gather: waterfall too large");
        ctx->activate();
        const size_t px = (size_t)n_samples * c * t;
        const bool per_baseline = flags_form == RFI_VALID_FLAGS_BASELINE;
        CallScope sc(ctx);
        const void* pl = sc.in(planes, planes_mem, px * 4 * dtype_bytes(dtype));
        const uint8_t* fl = sc.in(flags, flags_mem, px * (per_baseline ? 1 : 4));
        const rfi_patch_src* tb = sc.in(table_host, RFI_HOST, (size_t)n);
        const double* pr = sc.in(params_host ? params_host[0] : nullptr, RFI_HOST, (size_t)n_samples * 2);
        float* dout = sc.out(out_nhwc, out_mem, (size_t)n * ps * ps * 8);
        launch_pol_gather_valid(ctx, pl, dtype, c, t, tb, n, ps, centre, scale, pr, fl, per_baseline, fill, dout);
        sc.finish();
    });
}

int rfi_label_gather(rfi_ctx* ctx, const uint8_t* labels, int labels_mem, int n_samples, int c, int t, const uint8_t* invalid,
                     int invalid_mem, int invalid_form, int rule, const rfi_patch_src* table_host, int n_tiles, int ps,
                     int pad_value, uint8_t* out, int out_mem) {
    return guarded([&] {
        RFI_REQUIRE(ctx && n_tiles >= 0 && labels && (n_tiles == 0 || (table_host && out)), "label_gather: null argument");
        RFI_REQUIRE(invalid_form == RFI_VALID_FLAGS_POL || invalid_form == RFI_VALID_FLAGS_BASELINE, "label_gather: bad invalid form");
        RFI_REQUIRE(rule == RFI_LABEL_INVALID_ANY || rule == RFI_LABEL_INVALID_ALL, "label_gather: rule must be any (0) or all (1)");
        RFI_REQUIRE(pad_value >= 0 && pad_value <= 255, "label_gather: pad_value must be a byte");
        if (n_tiles == 0) return;
        check_table(table_host, n_tiles, n_samples, c, t, ps, "label_gather");
        RFI_REQUIRE((int64_t)n_samples * 4 * c * t < ((int64_t)1 << 40), "label_gather: waterfall too large");
        ctx->activate();
        const size_t px = (size_t)n_samples * c * t;
        const bool per_baseline = invalid_form == RFI_VALID_FLAGS_BASELINE;
        CallScope sc(ctx);
        const uint8_t* lb = sc.in(labels, labels_mem, px);
        const uint8_t* iv = sc.in(invalid, invalid_mem, px * (per_baseline ? 1 : 4));
        const rfi_patch_src* tb = sc.in(table_host, RFI_HOST, (size_t)n_tiles);
        uint8_t* dout = sc.out(out, out_mem, (size_t)n_tiles * ps * ps);
        launch_label_gather(ctx, lb, c, t, iv, per_baseline, rule == RFI_LABEL_INVALID_ALL, tb, n_tiles, ps, pad_value, dout);
        sc.finish();
    });
}

namespace {
// med / mad of every patch of w (n x per doubles) over its non-NaN values -> d_med, d_mad
void median_and_mad(rfi_ctx* ctx, const double* w, int n, int per, bool finite_only, double* d_med, double* d_mad,
                    int* d_cnt, bool f32 = false) {
    launch_patch_median(ctx, w, n, per, false, nullptr, finite_only, d_med, d_cnt, f32);
    launch_patch_median(ctx, w, n, per, true, d_med, finite_only, d_mad, nullptr, f32);
}
}  // namespace

int rfi_preprocess_real(rfi_ctx* ctx, const void* patches, int patches_mem, int dtype, int n, int ps_h, int ps_w,
                        int stretch, int normalize_before, int normalize_after, double flag_sigma, float* out_nhwc,
                        int out_mem, uint8_t* flags_out, int flags_mem) {
    return guarded([&] {
        RFI_REQUIRE(dtype == RFI_F64 || dtype == RFI_F32, "preprocess_real: input must be float64 or float32");
        // float32 input: NumPy keeps it in float32 arithmetic (preprocessor.py:608-706 on a float32 array); here the values
        // ride in doubles and every result is rounded to float32 (order_stats.hip)
        const bool f32 = dtype == RFI_F32;
        RFI_REQUIRE(stretch >= 0 && stretch <= 2, "preprocess_real: stretch must be 0 (none), 1 (SQRT) or 2 (LOG10)");
        RFI_REQUIRE(n >= 0 && ps_h > 0 && ps_w > 0 && (n == 0 || (patches && out_nhwc)), "preprocess_real: bad argument");
        if (n == 0) return;
        ctx->activate();
        const int per = ps_h * ps_w;
        const size_t px = (size_t)n * per;
        CallScope sc(ctx);
        const void* in = sc.in(patches, patches_mem, px * dtype_bytes(dtype));
        double* w = sc.temp<double>(px);
        double* stat = static_cast<double*>(sc.temp<void>((size_t)n * 2 * sizeof(double) + (size_t)n * sizeof(int)));
        double *d_med = stat, *d_mad = stat + n;
        int* d_cnt = reinterpret_cast<int*>(stat + 2 * (size_t)n);
        launch_to_abs_f64(ctx, in, dtype, (int64_t)px, w);            // real dtypes: widening copy
        auto normalise = [&] {
            launch_patch_median(ctx, w, n, per, false, nullptr, false, d_med, nullptr, f32);
            launch_scale_by_median(ctx, w, n, per, d_med, f32);
        };
        if (normalize_before) normalise();
        if (stretch) {
            launch_stretch(ctx, w, (int64_t)px, stretch, f32);
            median_and_mad(ctx, w, n, per, true, d_med, d_mad, d_cnt, f32);
            launch_replace_inf(ctx, w, n, per, d_mad, d_cnt);
        }
        if (normalize_after) normalise();
        float* dout = sc.out(out_nhwc, out_mem, px * 3);
        uint8_t* dfl = sc.out(flags_out, flags_mem, px);
        if (flags_out) {
            median_and_mad(ctx, w, n, per, false, d_med, d_mad, nullptr, f32);
            launch_mad_flags(ctx, w, n, per, d_med, d_mad, flag_sigma, dfl, f32);
        }
        void* mm = ctx->get_scratch((size_t)n * 4 * sizeof(unsigned long long));
        if (f32) {                                  // the channel kernels' float32 form on the float32 values
            float* w32 = sc.temp<float>(px);
            launch_narrow_f32(ctx, w, (int64_t)px, w32);
            launch_preprocess(ctx, w32, RFI_F32, n, ps_h, ps_w, static_cast<float*>(mm), dout);
        } else {
            launch_preprocess(ctx, w, RFI_F64, n, ps_h, ps_w, static_cast<float*>(mm), dout);
        }
        sc.finish();
    });
}

int rfi_mad_flags(rfi_ctx* ctx, const void* patches, int patches_mem, int dtype, int n, int ps_h, int ps_w,
                  double flag_sigma, uint8_t* flags_out, int flags_mem) {
    return guarded([&] {
        RFI_REQUIRE(dtype >= RFI_C128 && dtype <= RFI_F32, "mad_flags: unknown dtype");
        RFI_REQUIRE(n >= 0 && ps_h > 0 && ps_w > 0 && (n == 0 || (patches && flags_out)), "mad_flags: bad argument");
        if (n == 0) return;
        ctx->activate();
        const int per = ps_h * ps_w;
        const size_t px = (size_t)n * per;
        CallScope sc(ctx);
        const void* in = sc.in(patches, patches_mem, px * dtype_bytes(dtype));
        double* w = sc.temp<double>(px);
        double* stat = sc.temp<double>((size_t)n * 2);
        uint8_t* dfl = sc.out(flags_out, flags_mem, px);
        // complex64 / float32 input: NumPy keeps |z| and every step after it in float32 (rfi_preprocess_real's rule)
        const bool f32 = dtype == RFI_C64 || dtype == RFI_F32;
        launch_to_abs_f64(ctx, in, dtype, (int64_t)px, w);
        median_and_mad(ctx, w, n, per, false, stat, stat + n, nullptr, f32);
        launch_mad_flags(ctx, w, n, per, stat, stat + n, flag_sigma, dfl, f32);
        sc.finish();
    });
}

int rfi_generate_waterfalls(rfi_ctx* ctx, uint64_t seed, int n_samples, int n_pol, int c, int t, double noise_mjy,
                            int bandpass, int bandpass_order, double pol_corr, const rfi_event* events_host,
                            const int32_t* event_offsets_host, int out_dtype, void* planes_out, int planes_mem,
                            uint8_t* flags_out, int flags_mem) {
    return guarded([&] {
        RFI_REQUIRE(n_samples >= 0 && n_pol > 0 && c > 0 && t > 0, "generate_waterfalls: bad shape");
        RFI_REQUIRE(out_dtype == RFI_C128 || out_dtype == RFI_C64, "generate_waterfalls: output must be complex128/64");
        RFI_REQUIRE(planes_out && flags_out && event_offsets_host, "generate_waterfalls: null argument");
        if (n_samples == 0) return;
        const int n_events = event_offsets_host[n_samples];
        RFI_REQUIRE(event_offsets_host[0] == 0 && n_events >= 0 && (n_events == 0 || events_host),
                    "generate_waterfalls: bad event table");
        for (int s = 0; s < n_samples; ++s)
            RFI_REQUIRE(event_offsets_host[s] <= event_offsets_host[s + 1], "generate_waterfalls: offsets must ascend");
        ctx->activate();
        const size_t px = (size_t)n_samples * n_pol * c * t;
        CallScope sc(ctx);
        const rfi_event* ev = sc.in(events_host, RFI_HOST, (size_t)std::max(n_events, 1));
        const int32_t* of = sc.in(event_offsets_host, RFI_HOST, (size_t)(n_samples + 1));
        void* dpl = sc.out(planes_out, planes_mem, px * dtype_bytes(out_dtype));
        uint8_t* dfl = sc.out(flags_out, flags_mem, px);
        launch_synth(ctx, seed, n_samples, n_pol, c, t, noise_mjy, bandpass, bandpass_order, pol_corr, n_events ? ev : nullptr,
                     of, out_dtype, dpl, dfl);
        sc.finish();
    });
}

int rfi_confusion_counts(rfi_ctx* ctx, const void* pred, int pred_dtype, int pred_mem, const void* truth,
                         int truth_dtype, int truth_mem, int64_t count, int64_t* tp, int64_t* fp,
                         int64_t* fn) {
    return guarded([&] {
        RFI_REQUIRE(count >= 0, "confusion: negative count");
        RFI_REQUIRE((pred_dtype == RFI_U8 || pred_dtype == RFI_FLOAT32) &&
                        (truth_dtype == RFI_U8 || truth_dtype == RFI_FLOAT32), "confusion: dtype must be u8 or f32");
        ctx->activate();
        unsigned long long h3[3];
        CallScope sc(ctx);
        const void* dp = sc.in(pred, pred_mem, (size_t)count * (pred_dtype ? 4 : 1));
        const void* dt = sc.in(truth, truth_mem, (size_t)count * (truth_dtype ? 4 : 1));
        launch_confusion(ctx, dp, pred_dtype, dt, truth_dtype, count, sc.out(h3, RFI_HOST, 3));
        sc.finish();
        *tp = (int64_t)h3[0]; *fp = (int64_t)h3[1]; *fn = (int64_t)h3[2];
    });
}
int rfi_flag_statistics(rfi_ctx* ctx, const void* data, int data_mem, int dtype, int64_t count, const void* flags,
                        int flags_mem, int flags_dtype, int want, rfi_flag_stats* all_out, rfi_flag_stats* clean_out) {
    return guarded([&] {
        RFI_REQUIRE(ctx, "flag_statistics: null context");
        RFI_REQUIRE(dtype >= RFI_C128 && dtype <= RFI_F32, "flag_statistics: dtype must be complex128, complex64, float64 or float32");
        RFI_REQUIRE(count >= 0 && (count == 0 || data), "flag_statistics: bad data");
        RFI_REQUIRE(!flags || flags_dtype == RFI_U8, "flag_statistics: flags must be uint8 (non-zero == flagged)");
        RFI_REQUIRE(data_mem == RFI_HOST || data_mem == RFI_DEVICE, "flag_statistics: bad data memory kind");
        RFI_REQUIRE(!flags || flags_mem == RFI_HOST || flags_mem == RFI_DEVICE, "flag_statistics: bad flags memory kind");
        RFI_REQUIRE((want & ~(RFI_FS_ALL | RFI_FS_CLEAN | RFI_FS_MEDIANS)) == 0 && (want & (RFI_FS_ALL | RFI_FS_CLEAN)),
                    "flag_statistics: want must select the all and/or the unflagged view");
        RFI_REQUIRE((!(want & RFI_FS_ALL) || all_out) && (!(want & RFI_FS_CLEAN) || clean_out), "flag_statistics: null output");
        const double qnan = std::nan("");
        rfi_flag_stats res[2];
        for (auto& r : res) r = rfi_flag_stats{0, 0, qnan, qnan, qnan, qnan, qnan};
        if (count > 0) {
            ctx->activate();
            const size_t esz = dtype_bytes(dtype);
            const bool cplx = dtype == RFI_C128 || dtype == RFI_C64;
            // without flags the unflagged view IS the all view: compute it once
            const int views = flags ? (want & (RFI_FS_ALL | RFI_FS_CLEAN)) : RFI_FS_ALL;
            CallScope sc(ctx);
            const void* in = sc.in(data, data_mem, (size_t)count * esz);
            const void* fl = sc.in(flags, flags_mem, flags ? (size_t)count : 0);
            // workspace and |z| buffer in the context's scratch (kept between calls: no allocation per call)
            const size_t wsb = (flag_stats_ws_bytes() + 255) / 256 * 256;
            char* ws = static_cast<char*>(ctx->get_scratch(wsb + (cplx ? (size_t)count * (esz / 2) : 0)));
            void* mag = cplx ? ws + wsb : nullptr;
            auto* dout = reinterpret_cast<rfi_flag_stats*>(ws + flag_stats_ws_bytes() - sizeof(res));
            launch_flag_stats(ctx, in, dtype, count, static_cast<const uint8_t*>(fl), views, (want & RFI_FS_MEDIANS) != 0, ws,
                              mag, dout);
            RFI_CHECK_HIP(hipMemcpyAsync(res, dout, sizeof(res), hipMemcpyDeviceToHost, ctx->stream));
            RFI_CHECK_HIP(hipStreamSynchronize(ctx->stream));     // (the result lies in the scratch: also with device inputs)
            if (!flags) res[1] = res[0];
        }
        if (want & RFI_FS_ALL) *all_out = res[0];
        if (want & RFI_FS_CLEAN) *clean_out = res[1];
    });
}
int rfi_simulate_rfi(rfi_ctx* ctx, uint64_t seed, uint64_t first_sample, int n_samples, const rfi_sim_params* params,
                     const double* power_range_dev, int out_layout, void* out_dev, uint8_t* mask_dev,
                     rfi_sim_event* events_dev, double* baseline_frac_dev) {
    return guarded([&] {
        RFI_REQUIRE(ctx && params, "simulate_rfi: null argument");
        const rfi_sim_params& p = *params;
        const int64_t T = p.time_bins, F = p.freq_bins;
        RFI_REQUIRE(p.clean ? (T >= 1 && F >= 1) : (T >= 4 && F >= 52),
                    "simulate_rfi: needs time_bins >= 4 and freq_bins >= 52 (the reference's randint bounds)");
        RFI_REQUIRE(T * F < ((int64_t)1 << 32), "simulate_rfi: time_bins * freq_bins must stay below 2^32");
        RFI_REQUIRE(n_samples >= 0, "simulate_rfi: negative sample count");
        RFI_REQUIRE(first_sample + (uint64_t)n_samples <= ((uint64_t)1 << 32), "simulate_rfi: sample counter past 2^32");
        RFI_REQUIRE(n_samples * T * ((F + 255) / 256) < ((int64_t)1 << 31), "simulate_rfi: batch too large for one launch");
        RFI_REQUIRE(p.n_power >= 1 && p.n_power <= 1024, "simulate_rfi: power_range must have 1..1024 entries");
        RFI_REQUIRE(out_layout >= RFI_SIM_C128 && out_layout <= RFI_SIM_NHWC, "simulate_rfi: bad out_layout");
        RFI_REQUIRE(out_dev && mask_dev && power_range_dev && (p.clean || events_dev), "simulate_rfi: null buffer");
        if (n_samples == 0) return;
        ctx->activate();
        launch_rfi_sim(ctx, seed, (unsigned)first_sample, n_samples, p, power_range_dev, out_layout, out_dev, mask_dev,
                       events_dev, baseline_frac_dev);
    });
}
namespace {
// the size limits rfi_simulate_rfi puts on a batch with events, for the entry points that recompute from its event table
void require_sim_events_batch(const char* who, const rfi_sim_params& p, uint64_t first_sample, int n_samples) {
    const std::string w(who);
    const int64_t T = p.time_bins, F = p.freq_bins;
    RFI_REQUIRE(!p.clean, w + ": a clean batch has no events");
    RFI_REQUIRE(T >= 4 && F >= 52, w + ": needs time_bins >= 4 and freq_bins >= 52 (the reference's randint bounds)");
    RFI_REQUIRE(T * F < ((int64_t)1 << 32), w + ": time_bins * freq_bins must stay below 2^32");
    RFI_REQUIRE(n_samples >= 0, w + ": negative sample count");
    RFI_REQUIRE(first_sample + (uint64_t)n_samples <= ((uint64_t)1 << 32), w + ": sample counter past 2^32");
    RFI_REQUIRE(n_samples * T * ((F + 255) / 256) < ((int64_t)1 << 31), w + ": batch too large for one launch");
    RFI_REQUIRE(p.n_power >= 1 && p.n_power <= 1024, w + ": power_range must have 1..1024 entries");
}
}  // namespace
int rfi_sim_event_table(rfi_ctx* ctx, uint64_t seed, uint64_t first_sample, int n_samples, const rfi_sim_params* params,
                        const double* power_range_dev, const rfi_sim_event* events_dev, int32_t* area, int32_t* box) {
    return guarded([&] {
        RFI_REQUIRE(ctx && params, "sim_event_table: null argument");
        require_sim_events_batch("sim_event_table", *params, first_sample, n_samples);
        RFI_REQUIRE(power_range_dev && events_dev && area && box, "sim_event_table: null buffer");
        if (n_samples == 0) return;
        ctx->activate();
        launch_rfi_sim_event_table(ctx, seed, (unsigned)first_sample, n_samples, *params, power_range_dev, events_dev, area, box);
    });
}
int rfi_sim_instances(rfi_ctx* ctx, uint64_t seed, uint64_t first_sample, int n_samples, const rfi_sim_params* params,
                      const double* power_range_dev, const rfi_sim_event* events_dev, const int32_t* component, const int32_t* count,
                      const int32_t* base, int max_instances, int class_mode, int32_t* labels, uint8_t* masks) {
    return guarded([&] {
        RFI_REQUIRE(ctx && params, "sim_instances: null argument");
        require_sim_events_batch("sim_instances", *params, first_sample, n_samples);
        RFI_REQUIRE(max_instances >= 1 && max_instances <= 256, "sim_instances: max_instances must be in 1 .. 256");
        RFI_REQUIRE(class_mode == RFI_SIM_CLASS_SINGLE || class_mode == RFI_SIM_CLASS_FAMILY, "sim_instances: bad class_mode");
        RFI_REQUIRE(power_range_dev && events_dev && component && count && base && labels, "sim_instances: null buffer");
        if (n_samples == 0) return;
        ctx->activate();
        launch_rfi_sim_instances(ctx, seed, (unsigned)first_sample, n_samples, *params, power_range_dev, events_dev, component, count,
                                 base, max_instances, class_mode, labels, masks);
    });
}
int rfi_sim_family_bits(rfi_ctx* ctx, uint64_t seed, uint64_t first_sample, int n_samples, const rfi_sim_params* params,
                        const double* power_range_dev, const rfi_sim_event* events_dev, uint8_t* bits) {
    return guarded([&] {
        RFI_REQUIRE(ctx && params, "sim_family_bits: null argument");
        require_sim_events_batch("sim_family_bits", *params, first_sample, n_samples);
        RFI_REQUIRE(power_range_dev && events_dev && bits, "sim_family_bits: null buffer");
        if (n_samples == 0) return;
        ctx->activate();
        launch_rfi_sim_family_bits(ctx, seed, (unsigned)first_sample, n_samples, *params, power_range_dev, events_dev, bits);
    });
}
int rfi_sim_inject(rfi_ctx* ctx, uint64_t seed, uint64_t first_sample, int n_samples, const rfi_sim_params* params,
                   const double* power_range_dev, int layout, int rows, int cross_hand, const void* data_dev,
                   const uint8_t* flags_dev, int flag_pols, const double* sigma_dev, void* out_dev, uint8_t* mask_dev,
                   rfi_sim_event* events_dev, double* baseline_frac_dev) {
    return guarded([&] {
        RFI_REQUIRE(ctx && params, "sim_inject: null argument");
        require_sim_events_batch("sim_inject", *params, first_sample, n_samples);
        RFI_REQUIRE(layout == RFI_SIM_C128 || layout == RFI_SIM_C64, "sim_inject: the planes are complex128 or complex64");
        RFI_REQUIRE(rows == RFI_INJECT_ROWS_TIME || rows == RFI_INJECT_ROWS_CHANNEL, "sim_inject: bad rows");
        RFI_REQUIRE(cross_hand == RFI_INJECT_CROSS_INJECTED || cross_hand == RFI_INJECT_CROSS_REFERENCE, "sim_inject: bad cross_hand");
        RFI_REQUIRE(!flags_dev || flag_pols == 1 || flag_pols == 4, "sim_inject: flag_pols must be 1 or 4");
        RFI_REQUIRE(rfi_sim_inject_blocks(n_samples, params->time_bins, params->freq_bins, params->gibbs_ringing, rows) < ((int64_t)1 << 31),
                    "sim_inject: batch too large for one launch");
        RFI_REQUIRE(power_range_dev && data_dev && sigma_dev && out_dev && mask_dev && events_dev, "sim_inject: null buffer");
        if (n_samples == 0) return;
        ctx->activate();
        launch_rfi_sim_inject(ctx, seed, (unsigned)first_sample, n_samples, *params, power_range_dev, layout, rows, cross_hand, data_dev,
                              flags_dev, flag_pols, sigma_dev, out_dev, mask_dev, events_dev, baseline_frac_dev);
    });
}
int rfi_sim_transpose_planes(rfi_ctx* ctx, const uint8_t* src_dev, int64_t n, int rows, int cols, uint8_t* dst_dev) {
    return guarded([&] {
        RFI_REQUIRE(ctx, "sim_transpose_planes: null argument");
        RFI_REQUIRE(n >= 0 && rows >= 1 && cols >= 1, "sim_transpose_planes: bad sizes");
        RFI_REQUIRE(src_dev && dst_dev && src_dev != dst_dev, "sim_transpose_planes: null buffer, or dst is src");
        if (n == 0) return;
        ctx->activate();
        launch_rfi_sim_transpose_bytes(ctx, src_dev, n, rows, cols, dst_dev);
    });
}
namespace {
void norm_bracket(int64_t count, double q, int64_t* ranks, double* frac) {
    const double v = q * (double)(count - 1), f = std::floor(v);
    ranks[0] = (int64_t)f;
    ranks[1] = std::min(ranks[0] + 1, count - 1);
    if (frac) *frac = v - f;
}
}  // namespace
int rfi_norm_bracket(int64_t count, double q, int64_t* ranks, double* frac) {
    return guarded([&] {
        RFI_REQUIRE(count >= 1 && q >= 0.0 && q <= 1.0 && ranks, "norm_bracket: needs count >= 1, 0 <= q <= 1 and ranks");
        norm_bracket(count, q, ranks, frac);
    });
}
int rfi_norm_statistics(rfi_ctx* ctx, const void* const* chunks, const int64_t* counts, int n_chunks, int dtype,
                        int64_t segment, int quantiles, rfi_norm_stats* out, int n_out) {
    return guarded([&] {
        RFI_REQUIRE(ctx && chunks && counts && out, "norm_statistics: null argument");
        RFI_REQUIRE(dtype == RFI_F64 || dtype == RFI_F32, "norm_statistics: dtype must be float64 or float32 (pass complex data as its real scalars)");
        RFI_REQUIRE(n_chunks >= 1 && n_chunks <= 65536, "norm_statistics: needs 1 to 65536 chunks");
        RFI_REQUIRE(segment >= 0, "norm_statistics: negative segment");
        RFI_REQUIRE(segment == 0 || n_chunks == 1, "norm_statistics: the per-sample mode takes one chunk");
        const size_t esz = dtype == RFI_F32 ? 4 : 8;
        std::vector<norm_chunk> table((size_t)n_chunks + 1);
        int64_t total = 0;
        for (int i = 0; i < n_chunks; ++i) {
            RFI_REQUIRE(counts[i] >= 0 && (counts[i] == 0 || chunks[i]), "norm_statistics: bad chunk");
            RFI_REQUIRE(reinterpret_cast<uintptr_t>(chunks[i]) % esz == 0, "norm_statistics: misaligned chunk");
            table[i] = norm_chunk{chunks[i], total};
            total += counts[i];
        }
        table[n_chunks] = norm_chunk{nullptr, total};
        RFI_REQUIRE(total >= 1, "norm_statistics: no data");
        const int64_t seg = segment ? segment : total;
        RFI_REQUIRE(total % seg == 0, "norm_statistics: the chunk is not a whole number of segments");
        const int64_t pops = total / seg;
        RFI_REQUIRE(pops <= 4096, "norm_statistics: at most 4096 populations per call");
        RFI_REQUIRE(n_out == pops, "norm_statistics: n_out must be the number of populations");
        int64_t ranks[6];
        norm_bracket(seg, 0.5, ranks + 0, nullptr);
        norm_bracket(seg, 0.25, ranks + 2, nullptr);
        norm_bracket(seg, 0.75, ranks + 4, nullptr);
        ctx->activate();
        CallScope sc(ctx);
        const norm_chunk* tb = sc.in(table.data(), RFI_HOST, table.size());
        void* ws = sc.temp<void>(norm_stats_ws_bytes((int)pops, seg));
        rfi_norm_stats* dout = sc.out(out, RFI_HOST, (size_t)pops);
        launch_norm_stats(ctx, tb, n_chunks, dtype == RFI_F32, seg, (int)pops, quantiles != 0, ranks, ws, dout);
        sc.finish();
    });
}
int rfi_norm_apply(rfi_ctx* ctx, const void* src_dev, int dtype, int src_layout, int n, int64_t pixels, double centre,
                   double scale, const double* params_dev, float* dst_dev, int dst_layout) {
    return guarded([&] {
        RFI_REQUIRE(ctx, "norm_apply: null context");
        RFI_REQUIRE(dtype >= RFI_C128 && dtype <= RFI_F32, "norm_apply: dtype must be complex128, complex64, float64 or float32");
        RFI_REQUIRE(src_layout == RFI_NORM_NCHW || src_layout == RFI_NORM_NHWC, "norm_apply: bad source layout");
        RFI_REQUIRE(dst_layout == RFI_NORM_NCHW || dst_layout == RFI_NORM_NHWC, "norm_apply: bad destination layout");
        const bool cplx = dtype == RFI_C128 || dtype == RFI_C64;
        RFI_REQUIRE(!cplx || src_layout == RFI_NORM_NCHW, "norm_apply: complex input is (n, 4, T, F)");
        RFI_REQUIRE(n >= 0 && pixels >= 1 && (double)n * (double)pixels < 549755813888.0, "norm_apply: bad sizes");
        if (n == 0) return;
        RFI_REQUIRE(src_dev && dst_dev, "norm_apply: null buffer");
        RFI_REQUIRE(reinterpret_cast<uintptr_t>(src_dev) % 16 == 0 && reinterpret_cast<uintptr_t>(dst_dev) % 16 == 0,
                    "norm_apply: buffers must be 16-byte aligned");
        const size_t sbytes = (size_t)n * (size_t)pixels * 8 * (dtype == RFI_C64 || dtype == RFI_F32 ? 4 : 8);
        const size_t dbytes = (size_t)n * (size_t)pixels * 8 * 4;
        const char *s0 = static_cast<const char*>(src_dev), *d0 = reinterpret_cast<const char*>(dst_dev);
        const bool same = s0 == d0 && dtype == RFI_F32 && src_layout == dst_layout;
        RFI_REQUIRE(same || s0 + sbytes <= d0 || d0 + dbytes <= s0,
                    "norm_apply: source and destination overlap (in place needs the same dtype and layout)");
        ctx->activate();
        launch_norm_apply(ctx, src_dev, dtype, src_layout == RFI_NORM_NHWC, n, pixels, centre, scale, params_dev, dst_dev,
                          dst_layout == RFI_NORM_NHWC);
    });
}
// ---- validity-aware 8-channel input (include/rfi_hip.h): the three entry points above with an invalid map
namespace {
// the argument checks rfi_norm_apply makes on a source, for `who`
void check_valid_source(const char* who, rfi_ctx* ctx, int dtype, int src_layout, int n, int64_t pixels) {
    const std::string w(who);
    RFI_REQUIRE(ctx, w + ": null context");
    RFI_REQUIRE(dtype >= RFI_C128 && dtype <= RFI_F32, w + ": dtype must be complex128, complex64, float64 or float32");
    RFI_REQUIRE(src_layout == RFI_NORM_NCHW || src_layout == RFI_NORM_NHWC, w + ": bad source layout");
    const bool cplx = dtype == RFI_C128 || dtype == RFI_C64;
    RFI_REQUIRE(!cplx || src_layout == RFI_NORM_NCHW, w + ": complex input is (n, 4, T, F)");
    RFI_REQUIRE(n >= 0 && pixels >= 1 && (double)n * (double)pixels < 549755813888.0, w + ": bad sizes");
}
}  // namespace
int rfi_valid_map(rfi_ctx* ctx, const void* src_dev, int dtype, int src_layout, int n, int64_t pixels, const uint8_t* flags_dev,
                  int flags_form, uint8_t* map_dev, int64_t* counts, int counts_mem) {
    return guarded([&] {
        check_valid_source("valid_map", ctx, dtype, src_layout, n, pixels);
        RFI_REQUIRE(flags_form == RFI_VALID_FLAGS_POL || flags_form == RFI_VALID_FLAGS_BASELINE, "valid_map: bad flags form");
        if (n == 0) return;
        RFI_REQUIRE(src_dev && map_dev, "valid_map: null buffer");
        RFI_REQUIRE(reinterpret_cast<uintptr_t>(src_dev) % 16 == 0, "valid_map: the source must be 16-byte aligned");
        RFI_REQUIRE(cdiv(pixels, 256) <= 0x7fffffff, "valid_map: sample too large for one launch");
        ctx->activate();
        CallScope sc(ctx);
        int64_t* dc = counts ? sc.out(counts, counts_mem, (size_t)n) : sc.temp<int64_t>((size_t)n);
        launch_valid_map(ctx, src_dev, dtype, src_layout == RFI_NORM_NHWC, flags_dev, flags_form == RFI_VALID_FLAGS_BASELINE, n, pixels,
                         map_dev, dc);
        sc.finish();
    });
}
int rfi_valid_statistics(rfi_ctx* ctx, const void* const* chunks, const int64_t* counts, const uint8_t* const* maps,
                         const int* forms, const int64_t* pixels, int n_chunks, int dtype, int64_t segment, int quantiles,
                         rfi_norm_stats* out, int n_out) {
    return guarded([&] {
        RFI_REQUIRE(ctx && chunks && counts && maps && forms && pixels && out, "valid_statistics: null argument");
        RFI_REQUIRE(dtype == RFI_F64 || dtype == RFI_F32, "valid_statistics: dtype must be float64 or float32 (pass complex data as its real scalars)");
        RFI_REQUIRE(n_chunks >= 1 && n_chunks <= 65536, "valid_statistics: needs 1 to 65536 chunks");
        RFI_REQUIRE(segment >= 0, "valid_statistics: negative segment");
        RFI_REQUIRE(segment == 0 || n_chunks == 1, "valid_statistics: the per-sample mode takes one chunk");
        const size_t esz = dtype == RFI_F32 ? 4 : 8;
        std::vector<norm_chunk> table((size_t)n_chunks + 1);
        std::vector<valid_chunk> vtable((size_t)n_chunks);
        int64_t total = 0;
        for (int i = 0; i < n_chunks; ++i) {
            RFI_REQUIRE(counts[i] >= 0 && (counts[i] == 0 || (chunks[i] && maps[i])), "valid_statistics: bad chunk");
            RFI_REQUIRE(reinterpret_cast<uintptr_t>(chunks[i]) % esz == 0, "valid_statistics: misaligned chunk");
            RFI_REQUIRE(forms[i] == RFI_VALID_SRC_COMPLEX || forms[i] == RFI_VALID_SRC_PLANAR || forms[i] == RFI_VALID_SRC_NHWC,
                        "valid_statistics: bad source form");
            RFI_REQUIRE(pixels[i] >= 1 && counts[i] % (8 * pixels[i]) == 0,
                        "valid_statistics: a chunk must be whole samples of 8 x pixels scalars");
            table[i] = norm_chunk{chunks[i], total};
            vtable[i] = valid_chunk{maps[i], pixels[i], forms[i], 0};
            total += counts[i];
        }
        table[n_chunks] = norm_chunk{nullptr, total};
        RFI_REQUIRE(total >= 1, "valid_statistics: no data");
        const int64_t seg = segment ? segment : total;
        RFI_REQUIRE(total % seg == 0, "valid_statistics: the chunk is not a whole number of segments");
        const int64_t pops = total / seg;
        RFI_REQUIRE(pops <= 4096, "valid_statistics: at most 4096 populations per call");
        RFI_REQUIRE(n_out == pops, "valid_statistics: n_out must be the number of populations");
        ctx->activate();
        CallScope sc(ctx);
        const norm_chunk* tb = sc.in(table.data(), RFI_HOST, table.size());
        const valid_chunk* vb = sc.in(vtable.data(), RFI_HOST, vtable.size());
        void* ws = sc.temp<void>(valid_stats_ws_bytes((int)pops, seg));
        rfi_norm_stats* dout = sc.out(out, RFI_HOST, (size_t)pops);
        launch_valid_stats(ctx, tb, vb, n_chunks, dtype == RFI_F32, seg, (int)pops, quantiles != 0, ws, dout);
        sc.finish();
    });
}
int rfi_valid_apply(rfi_ctx* ctx, const void* src_dev, int dtype, int src_layout, int n, int64_t pixels, double centre,
                    double scale, const double* params_dev, const uint8_t* map_dev, float fill, float* dst_dev, int dst_layout) {
    return guarded([&] {
        check_valid_source("valid_apply", ctx, dtype, src_layout, n, pixels);
        RFI_REQUIRE(dst_layout == RFI_NORM_NCHW || dst_layout == RFI_NORM_NHWC, "valid_apply: bad destination layout");
        if (n == 0) return;
        RFI_REQUIRE(src_dev && dst_dev && map_dev, "valid_apply: null buffer");
        RFI_REQUIRE(reinterpret_cast<uintptr_t>(src_dev) % 16 == 0 && reinterpret_cast<uintptr_t>(dst_dev) % 16 == 0,
                    "valid_apply: buffers must be 16-byte aligned");
        const size_t sbytes = (size_t)n * (size_t)pixels * 8 * (dtype == RFI_C64 || dtype == RFI_F32 ? 4 : 8);
        const size_t dbytes = (size_t)n * (size_t)pixels * 8 * 4, mbytes = (size_t)n * (size_t)pixels * 4;
        const char *s0 = static_cast<const char*>(src_dev), *d0 = reinterpret_cast<const char*>(dst_dev);
        const char* m0 = reinterpret_cast<const char*>(map_dev);
        const bool same = s0 == d0 && dtype == RFI_F32 && src_layout == dst_layout;
        RFI_REQUIRE(same || s0 + sbytes <= d0 || d0 + dbytes <= s0,
                    "valid_apply: source and destination overlap (in place needs the same dtype and layout)");
        RFI_REQUIRE(m0 + mbytes <= d0 || d0 + dbytes <= m0, "valid_apply: the invalid map overlaps the destination");
        ctx->activate();
        launch_valid_apply(ctx, src_dev, dtype, src_layout == RFI_NORM_NHWC, map_dev, fill, n, pixels, centre, scale, params_dev,
                           dst_dev, dst_layout == RFI_NORM_NHWC);
    });
}
int rfi_threshold_logits(rfi_ctx* ctx, const float* logits_dev, int64_t count, float threshold,
                         uint8_t* mask_dev) {
    return guarded([&] {
        ctx->activate();
        launch_threshold(ctx, logits_dev, count, threshold, mask_dev);
    });
}

// ------------------------------------------------------------------------------------ whole-observation prediction
namespace {
// workspace of rfi_model_predict_flags that grows with the chunk (patch outputs, staged planes and outputs, the table)
constexpr size_t kPredictBudget = size_t(1) << 30;

// a temporary HIP stream / events
struct TmpStream {
    hipStream_t s = nullptr;
    TmpStream() { RFI_CHECK_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    ~TmpStream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
};
struct TmpEvents {
    std::vector<hipEvent_t> e;
    explicit TmpEvents(int n) : e((size_t)n, nullptr) {
        for (auto& x : e) RFI_CHECK_HIP(hipEventCreateWithFlags(&x, hipEventDisableTiming));
    }
    ~TmpEvents() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};
}  // namespace

int rfi_tiling_count(int c, int t, const rfi_tiling* tiling, int64_t* patches_per_plane) {
    return guarded([&] {
        RFI_REQUIRE(tiling && patches_per_plane, "tiling_count: null argument");
        RFI_REQUIRE(c > 0 && t > 0, "tiling_count: empty plane");
        check_tiling(*tiling);
        *patches_per_plane = tiling_patches_per_plane(c, t, *tiling);
    });
}

int rfi_tiling_table(int c, int t, const rfi_tiling* tiling, int n_units, rfi_patch_src* table_host, int64_t capacity) {
    return guarded([&] {
        RFI_REQUIRE(tiling && (table_host || capacity <= 0), "tiling_table: null argument");
        RFI_REQUIRE(c >= 0 && t >= 0 && n_units >= 0, "tiling_table: negative shape or unit count");
        check_tiling(*tiling);
        const TileGrid g = make_tile_grid(c, t, *tiling);
        RFI_REQUIRE(capacity >= (int64_t)n_units * g.ppp,
                    "tiling_table: the table has " + std::to_string((int64_t)n_units * g.ppp) + " entries, capacity is " +
                        std::to_string(capacity));
        const std::vector<rfi_patch_src> table = tile_table(g, n_units);
        std::copy(table.begin(), table.end(), table_host);
    });
}

int rfi_stitch_patches(rfi_ctx* ctx, const float* values, int values_mem, int kind, int n_planes, int c, int t,
                       const rfi_tiling* tiling, int combine, float threshold, uint8_t* flags, int flags_mem,
                       float* prob, int prob_mem) {
    return rfi_stitch_patches_classes(ctx, values, values_mem, kind, n_planes, 1, c, t, tiling, combine, threshold, flags, flags_mem,
                                      prob, prob_mem);
}
int rfi_stitch_patches_classes(rfi_ctx* ctx, const float* values, int values_mem, int kind, int n_planes, int n_classes, int c,
                               int t, const rfi_tiling* tiling, int combine, float threshold, uint8_t* flags, int flags_mem,
                               float* prob, int prob_mem) {
    return guarded([&] {
        RFI_REQUIRE(ctx && values && flags && tiling, "stitch_patches: null argument");
        RFI_REQUIRE(n_planes >= 0 && n_classes > 0 && c > 0 && t > 0, "stitch_patches: bad shape");
        check_tiling(*tiling);
        if (n_planes == 0) return;
        ctx->activate();
        const int64_t ppp = tiling_patches_per_plane(c, t, *tiling);
        const size_t px = (size_t)n_planes * n_classes * c * t;
        CallScope sc(ctx);
        const float* v = sc.in(values, values_mem, (size_t)n_planes * ppp * tiling->ps * tiling->ps * n_classes);
        uint8_t* df = sc.out(flags, flags_mem, px);
        float* dp = sc.out(prob, prob_mem, px);
        launch_stitch(ctx, v, kind, n_planes, c, t, *tiling, combine, threshold, df, dp, n_classes);
        sc.finish();
        RFI_CHECK_HIP(hipStreamSynchronize(ctx->stream));     // (with device pointers only too)
    });
}

// Chunks of k whole planes.  Per chunk: gather + channel extraction of `nb` patches at a time into one image batch,
// eval forward of that batch (always nb samples: one prepared shape; the slots past the chunk's last patch hold zeros or
// the previous batch's images and their outputs are dropped -- eval mode is independent per sample), its output copied
// into the chunk's patch-output buffer, then one stitch.  Host input is uploaded on a second stream into two alternating
// slots, the next chunk's upload next to the current chunk's compute; host outputs are staged the same way and copied
// back on that stream while the next chunk computes.
//
// One driver serves both entry points.  Its unit is what one stitched C x T plane of flags comes from: a complex plane
// (rfi_model_predict_flags) or a sample of 4 of them (rfi_model_predict_flags_pol); a PredictGather says how a batch of
// patches becomes an image batch.
namespace {
struct PredictGather {
    const char* who;           // the entry point, for messages
    const char* unit;          // "plane" or "sample"
    int in_ch;                 // channels of the image batch
    int pols;                  // complex planes per unit
    int max_out = 1;           // output channels a model may have: each is stitched into a plane of its own
    // optional second input streamed next to the planes (prior flags; aux_unit bytes per unit) and optional second
    // output written after the stitch (merged_unit bytes per unit); both null for the entry points without them
    const uint8_t* aux = nullptr;
    int aux_mem = RFI_HOST;
    size_t aux_unit = 0;
    uint8_t* merged = nullptr;
    int merged_mem = RFI_HOST;
    size_t merged_unit = 0;
    // private device workspace for image batches of nb patches out of n_units units, filled once by setup()
    virtual size_t ws_bytes(int nb, int n_units) const = 0;
    virtual void setup(rfi_ctx*, void*, int) {}
    // patches tb[0 .. nv) of the chunk at `pl`, whose first unit is unit `first` of the call -> img (nv, ps, ps, in_ch)
    virtual void run(rfi_ctx* ctx, const void* pl, int dtype, int first, int c, int t, const rfi_patch_src* tb, int nv, int ps,
                     void* ws, float* img) const = 0;
    // the chunk's part of `aux` on the device, before the chunk's first run()
    virtual void bind(const uint8_t*) {}
    // after the stitch of a chunk of np units at `pl`: its stitched flags -> its part of `merged`, both on the device
    virtual void merge(rfi_ctx*, const void*, int, int, int, int, const uint8_t*, uint8_t*) const {}
    virtual ~PredictGather() = default;
};

struct ChannelGather final : PredictGather {        // amplitude gradient, log-amplitude, phase (rfi_preprocess_gather's kernels)
    ChannelGather() { who = "predict_flags"; unit = "plane"; in_ch = 3; pols = 1; }
    size_t ws_bytes(int nb, int) const override { return (size_t)nb * 4 * sizeof(unsigned long long); }     // min/max words
    void run(rfi_ctx* ctx, const void* pl, int dtype, int, int c, int t, const rfi_patch_src* tb, int nv, int ps, void* ws,
             float* img) const override {
        launch_preprocess(ctx, pl, dtype, nv, ps, ps, static_cast<float*>(ws), img, tb, c, t);
    }
};

struct PolGather final : PredictGather {            // the four polarisations, normalised (rfi_norm_gather's kernel)
    double centre, scale;
    const double* params_host;                      // one pair per unit, or null
    PolGather(double ce, double sc, const double* ph) : centre(ce), scale(sc), params_host(ph) {
        who = "predict_flags_pol"; unit = "sample"; in_ch = 8; pols = 4; max_out = 8;
    }
    size_t ws_bytes(int, int n_units) const override { return params_host ? (size_t)n_units * 2 * sizeof(double) : 0; }
    void setup(rfi_ctx* ctx, void* ws, int n_units) override {
        if (params_host)
            RFI_CHECK_HIP(hipMemcpyAsync(ws, params_host, (size_t)n_units * 2 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    void run(rfi_ctx* ctx, const void* pl, int dtype, int first, int c, int t, const rfi_patch_src* tb, int nv, int ps, void* ws,
             float* img) const override {
        launch_pol_gather(ctx, pl, dtype, c, t, tb, nv, ps, centre, scale,
                          params_host ? static_cast<const double*>(ws) + 2 * (size_t)first : nullptr, img);
    }
};

struct ValidGather final : PredictGather {          // PolGather with prior flags and non-finite values (rfi_valid_gather's kernel)
    double centre, scale;
    const double* params_host;
    bool per_baseline;
    float fill;
    const uint8_t* cur = nullptr;                   // the current chunk's prior flags on the device
    ValidGather(double ce, double sc, const double* ph, bool pb, float fi) : centre(ce), scale(sc), params_host(ph), per_baseline(pb), fill(fi) {
        who = "predict_flags_valid"; unit = "sample"; in_ch = 8; pols = 4; max_out = 8;
    }
    size_t ws_bytes(int, int n_units) const override { return params_host ? (size_t)n_units * 2 * sizeof(double) : 0; }
    void setup(rfi_ctx* ctx, void* ws, int n_units) override {
        if (params_host)
            RFI_CHECK_HIP(hipMemcpyAsync(ws, params_host, (size_t)n_units * 2 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    void bind(const uint8_t* chunk_flags) override { cur = chunk_flags; }
    void run(rfi_ctx* ctx, const void* pl, int dtype, int first, int c, int t, const rfi_patch_src* tb, int nv, int ps, void* ws,
             float* img) const override {
        launch_pol_gather_valid(ctx, pl, dtype, c, t, tb, nv, ps, centre, scale,
                                params_host ? static_cast<const double*>(ws) + 2 * (size_t)first : nullptr, cur, per_baseline, fill, img);
    }
    void merge(rfi_ctx* ctx, const void* pl, int dtype, int np, int c, int t, const uint8_t* stitched, uint8_t* out) const override {
        launch_valid_merge(ctx, pl, dtype, np, (int64_t)c * t, cur, per_baseline, stitched, out);
    }
};

void predict_flags_driver(rfi_model* m, PredictGather& g, const void* planes, int planes_mem, int dtype, int n_planes, int c,
                          int t, const rfi_tiling* tiling, int batch, int combine, float threshold, uint8_t* flags,
                          int flags_mem, float* prob, int prob_mem) {
    const std::string who(g.who);
    RFI_REQUIRE(m && planes && flags && tiling, who + ": null argument");
    RFI_REQUIRE(dtype == RFI_C128 || dtype == RFI_C64,
                who + ": planes must be complex128 or complex64 (real input: Preprocessor + rfi_stitch_patches)");
    RFI_REQUIRE(n_planes >= 0 && c > 0 && t > 0 && batch > 0, who + ": bad shape or batch");
    // (several output channels: those of a model with class-bit labels, each a class of its own)
    const bool by_class = g.max_out > 1 && m->label_mode == RFI_LABELS_CLASS_BITS;
    RFI_REQUIRE(m->in_ch == g.in_ch && m->out_ch >= 1 && m->out_ch <= (by_class ? g.max_out : 1) && m->out_scale == 1,
                who + ": needs a model with " + std::to_string(g.in_ch) + " input channels, 1 output channel" +
                    (g.max_out > 1 ? " (class-bit labels: up to " + std::to_string(g.max_out) + ")" : std::string()) +
                    " and an output map the size of its input");
    RFI_REQUIRE(combine == RFI_COMBINE_MEAN || combine == RFI_COMBINE_MAX, who + ": combine must be mean (0) or max (1)");
    check_tiling(*tiling);
    if (n_planes == 0) return;
    rfi_ctx* ctx = m->ctx;
    ctx->activate();
    const int ps = tiling->ps;
    const int64_t ppp = tiling_patches_per_plane(c, t, *tiling);
    const size_t esz = dtype_bytes(dtype);
    // plane_px: pixels of a stitched plane; plane_bytes: the input behind it
    // K output channels: patch outputs are channel-last and every unit has K stitched planes (K = 1: the plane itself)
    const size_t K = (size_t)m->out_ch;
    const size_t plane_px = (size_t)c * t, plane_bytes = plane_px * esz * g.pols, patch_px = (size_t)ps * ps, out_px = plane_px * K;
    const bool host_in = planes_mem == RFI_HOST, host_fl = flags_mem == RFI_HOST, host_pr = prob && prob_mem == RFI_HOST;
    const bool host_ax = g.aux && g.aux_mem == RFI_HOST, host_mg = g.merged && g.merged_mem == RFI_HOST;
    const bool host_out = host_fl || host_pr || host_mg;
    RFI_REQUIRE(!g.merged || K == 1, who + ": merged flags need a model with 1 output channel");
    const size_t out_px_bytes = (host_fl ? 1 : 0) + (host_pr ? 4 : 0);
    const size_t per_plane = (size_t)ppp * (patch_px * K * sizeof(float) + sizeof(rfi_patch_src)) +
                             (host_in ? 2 * plane_bytes : 0) + 2 * out_px * out_px_bytes +
                             (host_ax ? 2 * g.aux_unit : 0) + (host_mg ? 2 * g.merged_unit : 0);
    RFI_REQUIRE(per_plane <= kPredictBudget,
                who + ": one " + (g.pols > 1 ? std::to_string(g.pols) + " x " : std::string()) + std::to_string(c) + " x " +
                    std::to_string(t) + " " + g.unit + " needs " +
                    std::to_string(per_plane >> 20) + " MiB of workspace at this tiling (" + std::to_string(ppp) +
                    " patches of " + std::to_string(ps) + "^2), over the budget of " +
                    std::to_string(kPredictBudget >> 20) + " MiB; " + g.unit + "s are not split: use a larger stride, fewer views "
                    "or smaller planes");
    // planes per chunk: at least ~4 batches of patches, no more than the budget holds; among up to 4x that, the one
    // whose last batch wastes the smallest share of slots
    const int kmax = (int)std::min<size_t>((size_t)n_planes, kPredictBudget / per_plane);
    const int k0 = (int)std::min<int64_t>(kmax, std::max<int64_t>(1, cdiv(4 * (int64_t)batch, ppp)));
    int k = k0;
    double best = 2.0;
    for (int kk = k0; kk <= std::min(kmax, 4 * k0); ++kk) {
        const int64_t np = (int64_t)kk * ppp, nbk = std::min<int64_t>(batch, np);
        const double waste = (double)(cdiv(np, nbk) * nbk - np) / (double)np;
        if (waste < best - 1e-12) { best = waste; k = kk; }
    }
    const int64_t chunk_patches = (int64_t)k * ppp;
    const int nb = (int)std::min<int64_t>(batch, chunk_patches);
    const int nchunks = (int)cdiv(n_planes, k);
    const int kind = m->head_sigmoid ? RFI_VALUES_PROBS : RFI_VALUES_LOGITS;

    // the chunk's patch table (plane indices local to the chunk; the same for every chunk, a prefix for the last)
    const std::vector<rfi_patch_src> table = tile_table(make_tile_grid(c, t, *tiling), k);

    // one grow-only scratch region: [table | the gather's own | images | patch outputs | 2 plane slots | 2 output slots |
    // 2 slots of the second input | 2 slots of the second output]
    const size_t b_table = al(table.size() * sizeof(rfi_patch_src)), b_gws = al(g.ws_bytes(nb, n_planes));
    const size_t b_img = al((size_t)nb * patch_px * g.in_ch * sizeof(float)), b_out = al((size_t)chunk_patches * patch_px * K * sizeof(float));
    const size_t b_in = host_in ? al((size_t)k * plane_bytes) : 0;
    const size_t b_fl = host_fl ? al((size_t)k * out_px) : 0, b_pr = host_pr ? al((size_t)k * out_px * sizeof(float)) : 0;
    const size_t b_ax = host_ax ? al((size_t)k * g.aux_unit) : 0, b_mg = host_mg ? al((size_t)k * g.merged_unit) : 0;
    char* base = static_cast<char*>(ctx->get_scratch(b_table + b_gws + b_img + b_out + 2 * (b_in + b_fl + b_pr + b_ax + b_mg)));
    auto* d_table = reinterpret_cast<rfi_patch_src*>(base);
    void* d_gws = base + b_table;
    float* d_img = reinterpret_cast<float*>(base + b_table + b_gws);
    float* d_out = reinterpret_cast<float*>(base + b_table + b_gws + b_img);
    char* slots = base + b_table + b_gws + b_img + b_out;
    auto in_slot = [&](int s) { return slots + s * b_in; };
    auto fl_slot = [&](int s) { return reinterpret_cast<uint8_t*>(slots + 2 * b_in + s * b_fl); };
    auto pr_slot = [&](int s) { return reinterpret_cast<float*>(slots + 2 * (b_in + b_fl) + s * b_pr); };
    auto ax_slot = [&](int s) { return reinterpret_cast<uint8_t*>(slots + 2 * (b_in + b_fl + b_pr) + s * b_ax); };
    auto mg_slot = [&](int s) { return reinterpret_cast<uint8_t*>(slots + 2 * (b_in + b_fl + b_pr + b_ax) + s * b_mg); };
    RFI_CHECK_HIP(hipMemcpyAsync(d_table, table.data(), table.size() * sizeof(rfi_patch_src), hipMemcpyHostToDevice,
                                 ctx->stream));
    RFI_CHECK_HIP(hipMemsetAsync(d_img, 0, b_img, ctx->stream));
    g.setup(ctx, d_gws, n_planes);

    TmpStream cs;
    TmpEvents ev(8);          // [0,1] upload done, [2,3] slot read by the gathers, [4,5] outputs ready, [6,7] outputs copied
    Drain drain{ctx, cs.s};   // every exit (an exception included) leaves both streams idle
    const char* src = static_cast<const char*>(planes);
    auto planes_in = [&](int ci) { return std::min(k, n_planes - ci * k); };
    auto upload = [&](int ci) {
        const int s = ci & 1;
        if (ci >= 2) RFI_CHECK_HIP(hipStreamWaitEvent(cs.s, ev.e[2 + s], 0));
        OnStream on(ctx, cs.s);
        ProfScope pf(ctx, FAM_PREPROCESS, 0, (double)planes_in(ci) * ((host_in ? plane_bytes : 0) + (host_ax ? g.aux_unit : 0)), "predict_upload");
        if (host_in)
            RFI_CHECK_HIP(hipMemcpyAsync(in_slot(s), src + (size_t)ci * k * plane_bytes, (size_t)planes_in(ci) * plane_bytes,
                                         hipMemcpyHostToDevice, cs.s));
        if (host_ax)
            RFI_CHECK_HIP(hipMemcpyAsync(ax_slot(s), g.aux + (size_t)ci * k * g.aux_unit, (size_t)planes_in(ci) * g.aux_unit,
                                         hipMemcpyHostToDevice, cs.s));
        RFI_CHECK_HIP(hipEventRecord(ev.e[s], cs.s));
    };
    auto download = [&](int ci) {
        const int s = ci & 1;
        const size_t px = (size_t)planes_in(ci) * out_px, off = (size_t)ci * k * out_px;
        RFI_CHECK_HIP(hipStreamWaitEvent(cs.s, ev.e[4 + s], 0));
        OnStream on(ctx, cs.s);
        ProfScope pf(ctx, FAM_PREPROCESS, 0, (double)px * out_px_bytes + (host_mg ? (double)planes_in(ci) * g.merged_unit : 0.0), "predict_download");
        if (host_fl) RFI_CHECK_HIP(hipMemcpyAsync(flags + off, fl_slot(s), px, hipMemcpyDeviceToHost, cs.s));
        if (host_pr) RFI_CHECK_HIP(hipMemcpyAsync(prob + off, pr_slot(s), px * sizeof(float), hipMemcpyDeviceToHost, cs.s));
        if (host_mg)
            RFI_CHECK_HIP(hipMemcpyAsync(g.merged + (size_t)ci * k * g.merged_unit, mg_slot(s), (size_t)planes_in(ci) * g.merged_unit,
                                         hipMemcpyDeviceToHost, cs.s));
        RFI_CHECK_HIP(hipEventRecord(ev.e[6 + s], cs.s));
    };
    auto compute = [&](int ci) {
        const int s = ci & 1, np = planes_in(ci);
        const int64_t npatch = (int64_t)np * ppp;
        const void* pl = host_in ? static_cast<const void*>(in_slot(s)) : static_cast<const void*>(src + (size_t)ci * k * plane_bytes);
        if (host_in || host_ax) RFI_CHECK_HIP(hipStreamWaitEvent(ctx->stream, ev.e[s], 0));
        if (host_out && ci >= 2) RFI_CHECK_HIP(hipStreamWaitEvent(ctx->stream, ev.e[6 + s], 0));
        if (g.aux) g.bind(host_ax ? ax_slot(s) : g.aux + (size_t)ci * k * g.aux_unit);
        for (int64_t p0 = 0; p0 < npatch; p0 += nb) {
            const int nv = (int)std::min<int64_t>(nb, npatch - p0);
            g.run(ctx, pl, dtype, ci * k, c, t, d_table + p0, nv, ps, d_gws, d_img);
            if (p0 + nb >= npatch && !g.merged) RFI_CHECK_HIP(hipEventRecord(ev.e[2 + s], ctx->stream));
            m->forward(d_img, nb, ps, ps, false);
            launch_copy_d2d(ctx, d_out + p0 * patch_px * K, m->buf(m->head_sigmoid ? m->probs : m->logits),
                            (size_t)nv * patch_px * K * sizeof(float));
        }
        const size_t off = (size_t)ci * k * out_px;
        launch_stitch(ctx, d_out, kind, np, c, t, *tiling, combine, threshold, host_fl ? fl_slot(s) : flags + off,
                      prob ? (host_pr ? pr_slot(s) : prob + off) : nullptr, (int)K);
        if (g.merged) {                       // (the merge reads the chunk's planes and prior flags once more: the slot is free after it)
            g.merge(ctx, pl, dtype, np, c, t, host_fl ? fl_slot(s) : flags + off,
                    host_mg ? mg_slot(s) : g.merged + (size_t)ci * k * g.merged_unit);
            RFI_CHECK_HIP(hipEventRecord(ev.e[2 + s], ctx->stream));
        }
        RFI_CHECK_HIP(hipEventRecord(ev.e[4 + s], ctx->stream));
    };
    if (host_in || host_ax) upload(0);
    for (int ci = 0; ci < nchunks; ++ci) {
        compute(ci);
        if (ci > 0 && host_out) download(ci - 1);
        if ((host_in || host_ax) && ci + 1 < nchunks) upload(ci + 1);
    }
    if (host_out) download(nchunks - 1);
    RFI_CHECK_HIP(hipStreamSynchronize(cs.s));
    RFI_CHECK_HIP(hipStreamSynchronize(ctx->stream));
}
}  // namespace

int rfi_model_predict_flags(rfi_model* m, const void* planes, int planes_mem, int dtype, int n_planes, int c, int t,
                            const rfi_tiling* tiling, int batch, int combine, float threshold, uint8_t* flags,
                            int flags_mem, float* prob, int prob_mem) {
    return guarded([&] {
        ChannelGather g;
        predict_flags_driver(m, g, planes, planes_mem, dtype, n_planes, c, t, tiling, batch, combine, threshold, flags, flags_mem,
                             prob, prob_mem);
    });
}

int rfi_model_predict_flags_pol(rfi_model* m, const void* planes, int planes_mem, int dtype, int n_samples, int c, int t,
                                const rfi_tiling* tiling, int batch, int combine, float threshold, double centre,
                                double scale, const double (*params_host)[2], uint8_t* flags, int flags_mem, float* prob,
                                int prob_mem) {
    return guarded([&] {
        PolGather g(centre, scale, params_host ? params_host[0] : nullptr);
        predict_flags_driver(m, g, planes, planes_mem, dtype, n_samples, c, t, tiling, batch, combine, threshold, flags, flags_mem,
                             prob, prob_mem);
    });
}

int rfi_model_predict_flags_valid(rfi_model* m, const void* planes, int planes_mem, int dtype, int n_samples, int c, int t,
                                  const rfi_tiling* tiling, int batch, int combine, float threshold, double centre,
                                  double scale, const double (*params_host)[2], const uint8_t* prior, int prior_mem,
                                  int prior_form, float fill, uint8_t* flags, int flags_mem, float* prob, int prob_mem,
                                  uint8_t* merged, int merged_mem) {
    return guarded([&] {
        RFI_REQUIRE(prior_form == RFI_VALID_FLAGS_POL || prior_form == RFI_VALID_FLAGS_BASELINE, "predict_flags_valid: bad flags form");
        const bool per_baseline = prior_form == RFI_VALID_FLAGS_BASELINE;
        ValidGather g(centre, scale, params_host ? params_host[0] : nullptr, per_baseline, fill);
        const size_t px = c > 0 && t > 0 ? (size_t)c * t : 0;
        g.aux = prior; g.aux_mem = prior_mem; g.aux_unit = px * (per_baseline ? 1 : 4);
        g.merged = merged; g.merged_mem = merged_mem; g.merged_unit = px * 4;
        predict_flags_driver(m, g, planes, planes_mem, dtype, n_samples, c, t, tiling, batch, combine, threshold, flags, flags_mem,
                             prob, prob_mem);
    });
}

}  // extern "C"
