// The networks of the library (one class per network) on top of the HIP kernels (host orchestration).
#pragma once
#include "derived.hpp"

namespace rfi {

struct DevBuf {
    rfi_ctx* ctx = nullptr;
    float* p = nullptr;
    size_t n = 0;
    void ensure(rfi_ctx* c, size_t floats);
    void free();
};

// a plane tensor (planes.hpp) owned by a model: [pixels][chunks][P][16] bf16 + a zeroed 64-byte tail
struct PlaneBuf {
    rfi_ctx* ctx = nullptr;
    bf16_t* p = nullptr;
    size_t elems = 0;                 // allocated (the largest shape so far)
    size_t used = 0;                  // of the shape in use: the kernels expect 64 zero bytes behind them
    int64_t pstride = 0;
    int nchunks = 0;
    void ensure(rfi_ctx* c, int64_t pixels, int C, int P);
    void free();
    YRef ref() const { return YRef(p, pstride); }                       // as a bfloat16 [pixel][pstride] tensor (P = 1)
    PlaneSeg seg() const { return PlaneSeg{p, pstride, nchunks}; }      // as a K-segment of a contraction
};

// One tensor of the U-Net's plane data flow (model_planes.cpp): a raw conv output or a gradient tensor that the mode stores
// either as float32 (bufs[f32]) or as bfloat16 (pl[b16]).  UNetModel::prepare_planes decides `half`, nobody else; the passes
// ask UNetModel::flow() for the storage in use
struct FlowTensor {
    int f32 = -1, b16 = -1;
    bool half = false;
};

// a tensor resolved to its storage, which is what the launches take: a float32 pointer, or a bfloat16 one with its pixel
// stride (neither: no tensor)
struct FlowRef {
    float* f = nullptr;
    bf16_t* h = nullptr;
    int64_t pstride = 0;
    FlowRef() = default;
    FlowRef(float* p) : f(p) {}
    FlowRef(const PlaneBuf& b) : h(b.p), pstride(b.pstride) {}
    FlowRef(bf16_t* p, int64_t ps) : h(p), pstride(ps) {}      // (a dense view of a scratch tensor)
    explicit operator bool() const { return f || h; }
    YRef ref() const { return h ? YRef(h, pstride) : YRef(f); }
};

// Conv3x3(pad 1)+bias -> BatchNorm2d -> ReLU
struct ConvBN {
    std::string conv_name, bn_name;     // e.g. "encoder1.conv.conv.0", "encoder1.conv.conv.1"
    int cin = 0, cout = 0;
    int cin_p = 0;                      // cin rounded up to a multiple of 4 (library layout; zero padded)
    size_t w_off = 0, b_off = 0, g_off = 0, be_off = 0;   // offsets into the flat param/grad buffers
    size_t dbias_rec_off = 0;           // this layer's region of UNetModel::dbias_pool (floats)
    int ema_repeats = 1;
    int level = 1;                      // resolution level of the OUTPUT: H >> (level - 1)
    int R = 3, stride = 1;              // ResNet-style encoder: 3x3 stride 1 / 2, or the 1x1 stride-2 projection (R = 1)
    bool has_bias = true;               // false: Conv2d(bias=False) in front of a BatchNorm (the bias slot stays 0, no state_dict entry)
    float* ws2d = nullptr;              // stride 2: filters of the 2x2 form on the space-to-depth input [4][cout][4 cin]
    float* wds2d = nullptr;             // ... and their dgrad layout [4'][4 cin][cout]
    float* ws2d3 = nullptr;             // ... and the 3 x bf16 records of both (a launch without them splits a temporary copy
    float* wds2d3 = nullptr;            // and drains the stream to free it: six stalls per step)
    bool has_bn = true;                 // false: Conv+bias -> ReLU (SimpleCNN); scale=1, shift=0 stay fixed
    bool frozen_bn = false;             // (with has_bn) BatchNorm frozen to its buffers (the backbone): no trainable affine
    size_t chan_off = 0, wd_off = 0;    // this layer's regions of chan_pool / wd_pool (floats)
    int64_t nbt = 0;                    // num_batches_tracked (host side)
    // device per-channel state: [running_mean | running_var | mean | invstd | scale | shift | c1 | c2]
    float* chan = nullptr;
    float* running_mean() const { return chan; }
    float* running_var() const { return chan + cout; }
    float* mean() const { return chan + 2 * cout; }
    float* invstd() const { return chan + 3 * cout; }
    float* scale() const { return chan + 4 * cout; }
    float* shift() const { return chan + 5 * cout; }
    float* c1() const { return chan + 6 * cout; }
    float* c2() const { return chan + 7 * cout; }
    // a frozen BatchNorm computes no batch statistics: its weight and bias live in the mean / invstd slots
    float* frozen_weight() const { return mean(); }
    float* frozen_bias() const { return invstd(); }
    float* wd = nullptr;                // dgrad-layout copy of the weight [9][cin_p][cout]
    float* w3 = nullptr;                // 3 x bf16 records of the forward layout (launch_weights_to_x3)
    float* wd3 = nullptr;               // ... and of the dgrad layout
    bf16_t* wBf = nullptr;              // plane kernels: filters in MFMA B-operand order, forward ...
    bf16_t* wBd = nullptr;              // ... and input-gradient direction (planes.hpp)
    bf16_t* ws3f = nullptr;             // wave-specialised float32 kernel (conv_ws.hip): B-operand order with three planes, one K
    bf16_t* ws3d = nullptr;             // segment; forward and input-gradient direction (3x3 stride-1 layers, channels % 16 == 0)
};

// ConvTranspose2d(k2,s2)+bias
struct UpConv {
    std::string name;                   // "decoder4.up"
    int cin = 0, cout = 0;
    size_t w_off = 0, b_off = 0;        // forward layout [4][cout][cin]
    size_t dbias_rec_off = 0;           // this layer's region of UNetModel::dbias_pool (floats)
    size_t wd_off = 0;                  // ... and of wd_pool
    float* wd = nullptr;                // dgrad layout [4][cin][cout]
    float* w3 = nullptr;                // 3 x bf16 records of both layouts
    float* wd3 = nullptr;
    bf16_t* wBf = nullptr;              // plane kernels (bfloat16 flow): the four taps as ONE 1x1 contraction with 4 cout channels ...
    bf16_t* wBd = nullptr;              // ... and the 2x2 stride-2 contraction of the input gradient
};

// what a state_dict entry is, which decides where it lives and in what layout
enum class EntryKind {
    ConvWeight,      // OIHW <-> the flat buffers' [tap][cout][cin_p] (padded channels stay 0)
    ConvTWeight,     // IOHW <-> [tap][cout][cin]
    LinearWeight,    // the head's and the 1x1 convs' [cout][cin][1][1]: the library's [1 tap][cout][cin] as is
    Bias, BnWeight, BnBias,                                  // flat vectors
    RunningMean, RunningVar, FrozenBnWeight, FrozenBnBias,   // per-channel state of convs[layer]
    NumBatchesTracked,                                       // host int64 of convs[layer]
};
// parameters live in the flat buffers (trained, counted by num_parameters); the other kinds are buffers
inline bool is_parameter(EntryKind k) { return k <= EntryKind::BnBias; }

struct Entry {
    std::string name;
    EntryKind kind = EntryKind::Bias;
    int ndim = 0;
    int64_t dims[4] = {0, 0, 0, 0};
    int layer = -1;      // index into convs (ConvWeight, per-channel and host entries)
    size_t off = 0;      // parameters: offset into the flat buffers
    int64_t numel() const {
        int64_t n = 1;
        for (int i = 0; i < ndim; ++i) n *= dims[i];
        return n;
    }
};

inline size_t align4(size_t v) { return (v + 3) & ~size_t(3); }

struct Shape { int N, H, W; };

// BatchNorm-apply + activation of layer c as a load transform for its consumers (slope 0 = ReLU; a layer without
// BatchNorm keeps scale 1, shift 0)
inline InXform act_of(const ConvBN& c, float slope = 0.0f) { return act_xform(c.scale(), c.shift(), slope); }

// reference layout <-> library layout of a conv / transposed-conv weight (model_params.cpp); cin_p >= cin: library rows
// are zero-padded to cin_p input channels
void to_lib_conv(const float* oihw, int cout, int cin, int R, std::vector<float>& out, int cin_p = -1);
void from_lib_conv(const float* lib, int cout, int cin, int R, float* oihw, int cin_p = -1);
void to_lib_convt(const float* iohw, int cin, int cout, std::vector<float>& out);     // ConvTranspose2d weight [cin][cout][2][2]
void from_lib_convt(const float* lib, int cin, int cout, float* iohw);

}  // namespace rfi

// What every network shares: shape, compute mode, loss, the parameter table with its flat buffers and derived filter
// copies, the buffers of the prepared shape, the side-stream / bucketed-exchange machinery and the optimiser step.  One
// derived class per network (below) builds its layers and runs its passes through the virtual hooks.
struct rfi_model {
    rfi_ctx* ctx = nullptr;
    int in_ch = 0, out_ch = 0, feat = 0, depth = 0;
    int out_scale = 1;                // output map / input map in each direction (the mask head's transposed conv: 2)
    bool training = true;
    // the arithmetic of the conv / wgrad MFMAs (float32 storage + accumulate): native float32, bf16-rounded operands, or
    // float32 operands as three bf16 pieces (DEFAULT: float32-level accuracy)
    enum class Arith { F32, BF16, X3 };
    Arith arith = Arith::X3;
    bool use_w3() const { return arith == Arith::X3; }   // who reads the pre-split filter records
    // plane data flow (model_planes.cpp; set by the U-Net family only): 0 off (round-1 kernels on float32 tensors), 1 bf16
    // activations (the bfloat16 compute mode), 3 float32 as three bf16 pieces
    int planesP = 0;
    // 0: BCE-with-logits + dice (the reference's, train_model.py:120-128); 1: focal; 2: BCE + the mean of the per-class dice
    // terms (class-bit labels; with one class it is kind 0)
    int loss_kind = 0;
    // what a label byte means (rfi_model_set_label_mode): RFI_LABELS_MAP non-zero == RFI, one output channel; RFI_LABELS_CLASS_BITS
    // bit k is the target of output channel k (the plain U-Net without the sigmoid head)
    int label_mode = 0;
    float focal_alpha = 0.25f, focal_gamma = 2.0f;
    // rfi_model_set_ignore / rfi_model_set_pos_weight: bit 7 of a label byte takes the pixel out of the loss and the counts;
    // pos_weight[k] multiplies the positive BCE term of channel k.  Either one routes the loss through the masked kernels
    bool ignore_on = false, weights_on = false;
    float pos_weight[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    bool masked_loss() const { return ignore_on || weights_on; }
    bool head_sigmoid = false;        // UNetOverfit: forward returns sigmoid(logits); the loss sees that too
    // a per-pixel head of out_ch channels with the loss inside the model.  False (the backbone: out_ch is the FPN width): no
    // logits, no label map, no loss workspace
    bool dense_head = true;

    std::vector<rfi::ConvBN> convs;   // the network's conv-like layers in forward order
    std::vector<rfi::UpConv> ups;     // its transposed convs
    size_t head_w_off = 0, head_b_off = 0;
    std::vector<rfi::Entry> entries;
    std::unordered_map<std::string, int> entry_index;

    size_t n_flat = 0;                // floats in each flat buffer (padded)
    int64_t n_params = 0;             // true scalar parameter count
    float *params = nullptr, *grads = nullptr, *adam_m = nullptr, *adam_v = nullptr;
    float* grad_acc = nullptr;        // rfi_model_grad_accumulate: sum of the gradients of several backward passes
    float* chan_pool = nullptr;
    float* wd_pool = nullptr;
    float* w3_pool = nullptr;         // pre-split (3 x bf16) filter records, rebuilt with the dgrad layouts
    rfi::bf16_t* ws_pool = nullptr;   // B-operand-order filters of the wave-specialised conv kernel (ConvBN::ws3f / ws3d) ...
    rfi::BatchTable ws;               // ... and the table of their batched rebuild (refresh_ws_weights)
    std::unordered_map<const float*, const rfi::bf16_t*> ws_by_w;    // float32 filter pointer (ConvArgs::w) -> the same filters for conv_ws / gemm_ws
    int ws_P = 0;                     // planes of the copies in ws_pool: 3 (float32 by 3 x bf16), 1 (bf16 operands), 0 (none built)
    int ws_need() const { return planesP ? 0 : arith == Arith::X3 ? 3 : arith == Arith::BF16 ? 1 : 0; }
    // the copy of filter `w` for the wave-specialised kernels in the current arithmetic (null: none)
    void ws_set(rfi::ConvArgs& a) const {
        auto it = ws_by_w.find(a.w);
        const rfi::bf16_t* p = it == ws_by_w.end() || ws_P != ws_need() ? nullptr : it->second;
        a.wB3 = ws_P == 3 ? p : nullptr;
        a.wB1 = ws_P == 1 ? p : nullptr;
        if (a.wB3 && x3_skipped.count(a.w)) a.w3 = nullptr;   // (no pre-split records are kept for this layer)
    }
    // The one place that maps `arith` onto a launch: its filters w (with their pre-split records w3, read in the 3 x bf16
    // arithmetic only, and the wave-specialised copy) and the MFMA mode ...
    void set_filters(rfi::ConvArgs& a, const float* w, const float* w3) const {
        a.w = w;
        a.w3 = use_w3() ? w3 : nullptr;
        ws_set(a);                    // (after w and w3: it looks up w and may clear w3)
        a.bf16 = arith == Arith::BF16;
        a.bf16x3 = arith == Arith::X3;
    }
    // ... and a weight gradient's slab workspace and MFMA mode
    void set_wgrad(rfi::WgradArgs& wa) const {
        wa.slab = bufs[ws_slab].p;
        wa.slab_floats = bufs[ws_slab].n;
        wa.bf16 = arith == Arith::BF16;
        wa.bf16x3 = arith == Arith::X3;
    }
    // The two workspaces: prepare_shape declares what the passes need, prepare() sizes them (need + 16 floats; the needs are
    // grow-only, as the buffers).  ws_red: the partial sums of a reduction, `floats` of them.  ws_slab: the slabs of weight
    // gradient `wa` -- the descriptor the backward pass will launch, from the same builder, with null data pointers -- or of a
    // plane weight gradient (pwgrad_slab_floats)
    size_t red_need = 0, slab_need = 0;
    void need_red(size_t floats) { red_need = std::max(red_need, floats); }
    void need_slab(size_t floats) { slab_need = std::max(slab_need, floats); }
    void need_slab(const rfi::WgradArgs& wa) { need_slab(rfi::wgrad_slab_floats(wa, rfi::IMPL_AUTO)); }
    // set by the plain U-Net: it keeps no pre-split (3 x bf16) filter records for the layers the wave-specialised kernels
    // cover, since at its shapes they never decline.  The other models (detector backbone on 4 x 4 maps, heads) keep every
    // record up to date, so a declined shape runs the round-2 kernel on valid records instead of a temporary copy (an
    // allocation + a stream synchronisation per launch)
    bool x3_skips_ws_layers = false;
    int64_t adam_step = 0;

    // ---- derived filter copies (derived.hpp; model.cpp): `stale` says which lag behind their sources.  Everything at
    // construction; the events below set bits, sync_filters (with side_rebuild_wd) is the one place that clears them
    unsigned stale = rfi::WEIGHT_DERIVED | rfi::FROZEN;
    void weights_changed() { stale |= rfi::WEIGHT_DERIVED; }    // apply, init_params, load_entry of a parameter
    void frozen_changed() { stale |= rfi::FROZEN; }             // load_entry of a per-channel entry
    bool model_copies_every_pass = false;     // the backbone: its own copies are rebuilt by every forward pass
    // rebuilds every stale copy the compute mode reads, row by row of the table: forward() and backward() call it.  A caller
    // that needs the forward half only lets a model that allows it (wd_split_ok) leave INPUT_GRAD_HALF to the side stream
    void sync_filters(rfi::Half needed);
    rfi::BatchTable relayout;         // dgrad layouts: one descriptor per conv-like layer, built once
    int64_t relayout_tiles = 0;
    void rebuild_dgrad();
    void refresh_ws_weights(rfi::Half half);
    rfi::BatchTable x3;               // pre-split records: the list of the batched rebuild ...
    rfi::RecordKey x3_key;            // ... and what it was built for
    rfi::RecordKey record_key() const { return rfi::RecordKey{ws_P, pH * 65536 + pW}; }    // (what a list built now is for)
    bool x3_reads_wd = false;         // the list reads dgrad-layout filters (which forbids the split)
    std::unordered_set<const float*> x3_skipped;      // filters whose records are NOT kept up to date (ws_set clears ConvArgs::w3 for them)
    void rebuild_records();
    // U-Net family hooks: may INPUT_GRAD_HALF be rebuilt on the side stream, and the model's own derived filters
    virtual bool wd_split_ok() const { return false; }
    virtual void refresh_model_weights(rfi::Half half) {}
    void refresh_s2d_forms(rfi::ConvBN& c);           // 2 x 2 form of a stride-2 3x3 filter, its dgrad layout, the records of both
    // a split rebuild: the side stream rebuilds INPUT_GRAD_HALF while the main stream runs the forward pass (side_rebuild_wd,
    // behind the first conv); wd_pending: enqueued there and not yet waited for (wait_wd: backward(), or the next rebuild)
    hipEvent_t wd_ready = nullptr;
    bool wd_pending = false;
    void side_rebuild_wd();
    void wait_wd();

    // activations / workspaces for the prepared shape (pN == 0: nothing prepared)
    int pN = 0, pH = 0, pW = 0;
    void invalidate_shape() { pN = 0; }               // the next prepare() sizes everything again
    std::vector<rfi::DevBuf> bufs;
    // indices into bufs.  What the entry points stage through and the workspaces: the constructor creates them, prepare() sizes
    // them (probs, sigmoid(logits) when head_sigmoid: by the one model that can enable it)
    int logits = -1, dlogits = -1, probs = -1;
    int x_stage = -1, x_stage2 = -1, x_pad = -1, out_stage = -1, ws_red = -1, ws_slab = -1, lab_stage = -1;
    int gx = -1;                      // the gradient w.r.t. the input (the detector's heads own it; -1: the model computes none)
    bool ext_dlogits = false;         // backward from caller-provided dlogits (rfi_model_backward_dlogits)
    double* d_sums = nullptr;         // [0..3] loss sums, [4] grad sumsq, [5..7] eval_batch's counts, [8..39] class-bit loss sums (4 x 8), [40] the masked loss's valid element count
    static constexpr int kSumsDoubles = 48;
    double* class_sums() const { return d_sums + 8; }
    float* d_scalars = nullptr;       // [0] loss, [1] grad norm
    float last_loss = 0, last_norm = 0;

    rfi_model(int in, int out, int f, int d) : in_ch(in), out_ch(out), feat(f), depth(d) {
        make_bufs({&logits, &dlogits, &probs, &x_stage, &x_stage2, &x_pad, &out_stage, &ws_red, &ws_slab, &lab_stage});
    }
    virtual ~rfi_model();
    virtual void build() = 0;                          // layers, parameter table, device state, the slots of the network's own tensors
    // rejoins the streams; for a shape other than the prepared one: prepare_shape, then the shared buffers and workspaces
    void prepare(int n, int h, int w);
    // rejects a shape the network cannot run, sizes the network's own tensors and declares its workspace needs
    virtual void prepare_shape(int n, int h, int w) = 0;
    void forward(const float* x_dev, int n, int h, int w, bool train_mode);    // (prepare + derived filters, then forward_pass)
    virtual void forward_pass(const float* x_dev, int n, int h, int w, bool train_mode) = 0;
    void loss_forward(const uint8_t* labels_dev, int n, int h, int w);
    void loss_backward(const uint8_t* labels_dev, int64_t pixels);      // logits + the loss sums -> dlogits (U-Net family)
    void backward(const float* x_dev, const uint8_t* labels_dev, int n, int h, int w);    // (then backward_pass)
    virtual void backward_pass(const float* x_dev, const uint8_t* labels_dev, int n, int h, int w) = 0;
    void apply(const rfi_hyper& hp, float grad_scale);
    virtual void algorithmic_flops(int n, int h, int w, double& fwd, double& step) const = 0;   // 2*M*K*N per layer
    virtual void set_compute_dtype(int dtype);        // rfi_model_set_compute_dtype's codes
    // rfi_model_debug_tensor for names other than logits / dlogits / chan: `n` floats at `src` (`name` with its ":pad" suffix,
    // base and idx without; float32 copies of bfloat16 tensors are temporaries of the call: sc)
    virtual void debug_tensor(const std::string& name, const std::string& base, int idx, bool to_host, rfi::CallScope& sc, const float*& src,
                              size_t& n);

    // ---- the parameter table (model_params.cpp).  build() registers the layers in the order of the flat buffers, which
    // is also the state_dict's: each gets its align4'd flat slots, its regions of chan_pool / wd_pool and its entries
    size_t chan_floats = 0, wd_floats = 0;
    int add_conv(rfi::ConvBN c);      // (names, shape and flags set) slots w, b, and g, be for a trainable BatchNorm; -> convs index
    void add_up(const std::string& name, int cin, int cout);   // transposed conv: w, b
    void add_head(const std::string& name, int cin);           // the final 1x1 conv (out_ch outputs): w, b
    void alloc_state();               // (end of build()) flat buffers, pools and the layers' pointers into them, loss scalars
    void reset_channel_state();       // running stats 0/1, BN-less layers: scale 1, shift 0
    const rfi::Entry& entry(const char* name) const;
    void init_params(uint64_t seed);  // rfi_model_init
    void load_entry(const rfi::Entry& e, const void* host, size_t bytes);
    void store_entry(const rfi::Entry& e, void* host, size_t bytes);
    void store_flat(const float* flat, const rfi::Entry& e, void* host, size_t bytes);   // a parameter's slot of params / grads / adam_m / adam_v
    void load_adam(const rfi::Entry& e, const void* host_m, const void* host_v, size_t bytes);
    float* buf(int i) { return bufs[i].p; }
    int new_buf() { bufs.emplace_back(); return (int)bufs.size() - 1; }
    void make_bufs(std::initializer_list<int*> slots) { for (int* s : slots) *s = new_buf(); }     // build(): a network's own tensors
    // what the first conv reads: the input with its channels zero-padded to convs[0].cin_p.  network_input pads (forward
    // pass); padded_input is that view again for a backward pass, without a launch
    rfi::View network_input(const float* x_dev, int n, int h, int w);
    rfi::View padded_input(const float* x_dev) const {
        const int cp = convs[0].cin_p;
        return cp == in_ch ? rfi::View{x_dev, in_ch} : rfi::View{bufs[x_pad].p, cp};
    }

    // ---- launches on float32 tensors the networks share (model.cpp); algo_flops, stats and done stay the caller's
    // a stride-1 conv whose output grid is its input's (s): R x R taps, `pad`, filters w [tap][cout][cin], output [M][cout]
    rfi::ConvArgs conv_same(rfi::View x, rfi::InXform xf, rfi::Shape s, int R, int pad, int cin, int cout, const float* w,
                            const float* w3, const float* bias, float* y) const;
    // its weight gradient from dy ([M][cout]) into dw [tap][cout][cin]
    rfi::WgradArgs wgrad_same(rfi::View x, rfi::InXform xf_x, const float* dy, rfi::Shape s, int R, int pad, int cin, int cout,
                              float* dw) const;
    // BatchNorm of layer c behind the conv that wrote its M output pixels.  Train: the batch statistics from the `records` the conv
    // epilogue left in ws_red (none: a pass over the float32 output Y), finalize, running statistics; eval: the coefficients
    void bn_tail(rfi::ConvBN& c, const float* Y, int64_t M, bool train, int records);
    // conv_same into Y, then bn_tail
    void conv_bn(rfi::ConvBN& c, rfi::View in, rfi::InXform xf, rfi::Shape s, const float* w, const float* w3, int R, int pad,
                 int cin, float* Y, bool train, double flops);
    // ConvTranspose2d(k2, s2) over the input grid s: the forward launch but its output (y / y16: the caller's) ...
    rfi::ConvArgs convt_args(const rfi::UpConv& u, rfi::View x, rfi::InXform xf, rfi::Shape s) const;
    // ... its weight gradient from dup (the gradient w.r.t. its output) ...
    rfi::WgradArgs convt_wgrad_args(const rfi::UpConv& u, rfi::View dup, rfi::View x, rfi::InXform xf, rfi::Shape s) const;
    // ... and its backward pass from dup: that weight gradient on the side stream, then the input gradient into dx [M][u.cin].
    // (The bias gradient is the caller's.)
    void convt_backward(const rfi::UpConv& u, rfi::View dup, rfi::View x, rfi::InXform xf, rfi::Shape s, float* dx);

    // backward-pass overlap: wgrad launches go to the context's side stream (see model.cpp)
    int side_seq = 0;
    int side_bound = 2;               // main may run this many side launches ahead (0: no bound -- nothing the side work reads is rewritten before side_join)
    void side_begin();                // side stream waits for everything enqueued on the main stream so far
    hipEvent_t next_fork_event();     // a fresh event for launch_*(..., done) (null: overlap off)
    void side_begin_after(hipEvent_t producer_done);   // side stream waits for that producer kernel only (null: as side_begin)
    void side_end();                  // marks the side launch; bounds the main stream's run-ahead
    void side_join();                 // main stream waits for all side work
    // a head model inside a larger step (the detector's box / mask heads): nothing the caller does next needs this model's WEIGHT
    // gradients, so the pass ends without waiting for them; whoever touches the gradients, the buffers or the weights next
    // (apply, all-reduce, accumulate, store_grad, the next forward / backward pass) joins first
    hipEvent_t lazy_ev = nullptr;
    bool lazy_pending = false;
    void side_join_lazy();
    void join_pending_side();
    void wgrad_on_side(const rfi::WgradArgs& wa, hipEvent_t after, bool after_everything = false);
    // bucketed gradient exchange (common.hpp): grads[lo, hi) are final once everything enqueued so far on the main
    // and side streams has run -> all-reduce them on the communication stream; exchange_join: main waits for all
    bool exchange_in_backward = false;   // set by the full-step entry points only (the split API exchanges explicitly)
    void bucket_ready(size_t lo, size_t hi);
    size_t pend_lo = 0, pend_hi = 0;  // finished but not yet exchanged range (small buckets wait for their neighbours)
    void flush_bucket();
    void exchange_join();
};

namespace rfi {
// launches inside a SideScope go to the side stream (behind `after`, or behind everything enqueued on the main stream so
// far); end() marks the side launch.  Left without end() (a throw) the context's stream is put back
struct SideScope {
    rfi_model* m;
    bool ended = false;
    explicit SideScope(rfi_model* model, hipEvent_t after = nullptr) : m(model) { m->side_begin_after(after); }
    void end() { m->side_end(); ended = true; }
    ~SideScope() { if (!ended) m->ctx->stream = m->ctx->main_stream; }
};
}  // namespace rfi

// U-Net (models/unet.py; model.cpp) and, with resnet_encoder, the U-Net with a ResNet-18-style encoder (SURVEY 8a A10;
// model_resnet.cpp).  Both share the decoder, the head, the loss and the plane data flow (model_planes.cpp)
struct UNetModel : rfi_model {
    const bool resnet_encoder;
    UNetModel(int in, int out, int f, int d, bool resnet) : rfi_model(in, out, f, d), resnet_encoder(resnet) {
        x3_skips_ws_layers = !resnet;
    }
    ~UNetModel() override;
    void build() override;
    void prepare_shape(int n, int h, int w) override;
    void forward_pass(const float* x_dev, int n, int h, int w, bool train_mode) override;
    void backward_pass(const float* x_dev, const uint8_t* labels_dev, int n, int h, int w) override;
    void algorithmic_flops(int n, int h, int w, double& fwd, double& step) const override;
    void set_compute_dtype(int dtype) override;
    void debug_tensor(const std::string& name, const std::string& base, int idx, bool to_host, rfi::CallScope& sc, const float*& src,
                      size_t& n) override;
    bool wd_split_ok() const override;
    void refresh_model_weights(rfi::Half half) override;

    int i_bott = 0;                   // index of the bottleneck's first conv in `convs` (decoder convs follow it)
    float act_slope = 0.0f;           // 0: ReLU; > 0: LeakyReLU(negative_slope) (UNetDifferentActivation)
    // BN-apply + activation of layer c as a load transform for its consumers (slope 0 = ReLU)
    rfi::InXform bn_xf(const rfi::ConvBN& c) const { return rfi::act_of(c, act_slope); }
    // convs: enc1.c1, enc1.c2, ..., encD.c2, bott.c1, bott.c2, decD.c1, decD.c2, ..., dec1.c2; ups: decD.up ... dec1.up
    // Raw conv outputs and gradient tensors, by level.  The float32 path reads their float32 storage, buf(t); on a plane data
    // flow some are bfloat16 tensors instead: flow(t), below
    std::vector<rfi::FlowTensor> encY1, encY2, decY1, decY2, gA, gB, dconcat, dpool;
    rfi::FlowTensor bottY1, bottY2, gBottA, gBottB;
    std::vector<int> concat, pool;
    std::vector<int> gAe, gBe;        // float32 U-Net path: the encoder phase's gradient tensors (gA / gB are the decoder's)
    using rfi_model::buf;
    float* buf(const rfi::FlowTensor& t) { return bufs[t.f32].p; }
    // conv-bias gradients of the float32 U-Net path: bn_bwd_apply leaves its per-block partial sums in a per-layer region of
    // dbias_pool; ONE batched launch at the end of the backward pass finishes them all (single-GPU steps: with a gradient
    // exchange the buckets need every gradient of a layer when the layer is done)
    float* dbias_pool = nullptr;
    void* dbias_descs = nullptr;
    int dbias_n = 0, dbias_max_c = 0;
    bool dbias_deferred = false;
    size_t head_rec_off = 0;            // the head's region of dbias_pool (its dw / db partials)
    bool head_fin_deferred = false;

    // ---- ResNet-18-style encoder (model_resnet.cpp): stem + 4 stages of 2 BasicBlocks
    struct ResBlock {
        int c1 = -1, c2 = -1, cd = -1;            // convs indices: conv1, conv2, projection (-1: identity shortcut)
        int stride = 1, cin = 0, cout = 0, level = 1;
        int Y1 = -1, Y2 = -1, Yd = -1, xs = -1, A = -1;      // bufs indices: raw conv outputs, space-to-depth input, block output
    };
    std::vector<ResBlock> blocks;
    int rs_stemY = -1, rs_a0 = -1, rs_g0 = -1, rs_g1 = -1, rs_dX = -1, rs_dS = -1, rs_dW = -1, rs_dzd = -1;
    int rs_dz[2] = {-1, -1}, rs_dA1[2] = {-1, -1};    // by block parity: the side stream's weight gradients still read the last block's
    float* rs_ones = nullptr;         // [max C] ones / zeros: identity scale / shift for the pooling kernels
    float* rs_zeros = nullptr;
    float* rs_wpool = nullptr;        // derived filters of the stride-2 and 1x1 convs
    void build_resnet();
    void prepare_resnet(int n, int h, int w);
    void refresh_resnet_weights();
    rfi::View forward_resnet_encoder(rfi::View x, int n, int h, int w, bool train_mode);
    void backward_resnet_encoder(const float* x_dev, int n, int h, int w);

    // ---- plane data flow (model_planes.cpp; planesP in the base)
    std::vector<rfi::PlaneBuf> pl;
    std::vector<int> pA1e, pSkip, pPool, pUp, pA1d, pdYa, pdYb, pdYaE, pdYbE, pUpIn, upf;      // (upf: bufs indices)
    int pXin = -1, pA1b = -1, pdYbottA = -1, pdYbottB = -1;
    // bf16 data flow (P = 1): three gates of the width decide which tensors are bfloat16 (prepare_planes holds the table).
    // y16_flow (feat % 4 == 0): raw conv outputs that only elementwise kernels read -- both convs of every encoder, the first
    // of the bottleneck and of every decoder, the last decoder's second.  The tensors a transposed conv reads stay float32
    // tensors holding bf16-rounded values, so the arithmetic is uniform: every conv output of this mode is a bfloat16 value
    bool y16_flow = false;
    // g16_flow (level widths multiples of 16): the gradient tensors the input-gradient convs write (dA of every first conv, the
    // pooled gradients), and dA of the second convs where an elementwise kernel produces it (head, max-pool backward)
    bool g16_flow = false;
    // gA.<l> has two storages in one pass: the decoder phase and the encoder phase share the tensor (gA: the encoder's rule)
    std::vector<rfi::FlowTensor> gAdec;
    // the storage of t in use
    rfi::FlowRef flow(const rfi::FlowTensor& t) { return t.half ? rfi::FlowRef(pl[t.b16]) : rfi::FlowRef(buf(t)); }
    // ResNet-style encoder on the bf16 flow (feat % 16 == 0; model_planes.cpp): indices into pl.  Every block owns its
    // raw conv outputs, its activation planes and its dY planes (the side stream's weight gradients read them until side_join)
    struct ResPlanes {
        int Y1 = -1, Y2 = -1, Yd = -1, A1 = -1, A = -1, dY1 = -1, dY2 = -1, dYd = -1;
        rfi::bf16_t* wBcls[4] = {nullptr, nullptr, nullptr, nullptr};     // stride 2: input-gradient filters per parity class
        float* cls = nullptr;                                             // ... and their float32 table (launch_w_s2_classes)
    };
    std::vector<ResPlanes> rpb;
    int rpStemY = -1, rpA0 = -1, rpdY0 = -1, rp_dA1 = -1, rp_dX = -1;
    int rp_dz[2] = {-1, -1};
    float* rs_cls_pool = nullptr;
    bool resnet_planes() const { return resnet_encoder && planesP == 1; }
    void forward_resnet_planes(rfi::PlaneSeg& cur, int n, int h, int w, bool train_mode);
    void backward_resnet_planes(int n, int h, int w);
    // transposed convs on the plane kernels (bfloat16 flow, init_features % 32 == 0): the DoubleConv outputs they read are bfloat16
    // (bottY2, decY2[l]) and activated once into planes (pUpIn[l]: the forward operand AND the weight gradient's); the decoder's
    // first conv writes its input gradient [up | skip] as bfloat16 (dconcat[l]) and the transposed conv's input gradient is
    // bfloat16 too (gBottA, gA[l + 1]), with the BatchNorm-backward sums of the layer below in its epilogue
    bool convt_planes = false;
    // the skip half (channels C .. 2 C - 1) of the gradient decoder l's first conv sends into its [up | skip] input
    rfi::YRef skip_grad(int l, int C) {
        const rfi::FlowRef g = flow(dconcat[l]);
        return g.h ? rfi::YRef(g.h + C, g.pstride) : rfi::YRef(g.f + C, (int64_t)2 * C);
    }
    rfi::bf16_t* wb_pool = nullptr;
    rfi::BatchTable wb;               // (the forward-direction filter images first)
    void set_planes(int P);           // switches the data flow; frees plane tensors of another P
    void make_slots();                // (end of build()) the float32 tensors' slots, then make_plane_slots
    void make_plane_slots();          // every plane tensor's slot, for either flow: they depend on depth and blocks only
    void prepare_planes(int n, int h, int w);        // (prepare_shape, on a plane data flow)
    void refresh_plane_weights(rfi::Half half);      // InputGrad: + the parity-class tables
    void forward_planes(const float* x_dev, int n, int h, int w, bool train_mode);
    void backward_planes(const float* x_dev, const uint8_t* labels_dev, int n, int h, int w);
    // weight-gradient launches of the plane kernel: of conv layer c over the output grid s (in: its input in nseg K-segments,
    // dY: the gradient w.r.t. its raw output) and of transposed conv u over its input grid s (dUp: the gradient w.r.t. its
    // output, in: its activated input).  prepare_planes declares ws_slab's need from the same descriptors with null operands
    rfi::PWgradArgs pwgrad_args(const rfi::ConvBN& c, const rfi::PlaneSeg* in, int nseg, rfi::PlaneSeg dY, rfi::Shape s);
    rfi::PWgradArgs convt_pwgrad_args(const rfi::UpConv& u, rfi::PlaneSeg dUp, rfi::PlaneSeg in, rfi::Shape s);
    // the flow tensor a debug name means (null: none of them) with its pixels and channels; a level out of range throws
    const rfi::FlowTensor* flow_named(const std::string& base, int idx, size_t& M, int& C) const;
    // debug_tensor of the plain U-Net on a plane data flow: bfloat16 and plane tensors as float32 values, "<name>:pad"
    void debug_tensor_planes(const std::string& name, const std::string& base, int idx, bool to_host, rfi::CallScope& sc, const float*& src,
                             size_t& n);
    // ... its conversion of ONE plane tensor (pl[pi]: M pixels, C channels, P_ pieces; pad: the padding lanes instead) ...
    void debug_plane_values(int pi, size_t M, int C, int P_, bool pad, bool to_host, rfi::CallScope& sc, const float*& src, size_t& n);
    // ... and the tensors of the ResNet-style encoder on the bf16 flow (false: `base` is none of them)
    bool debug_tensor_resnet_planes(const std::string& name, const std::string& base, int idx, bool to_host, rfi::CallScope& sc,
                                    const float*& src, size_t& n);
};

// 3-layer CNN (model_cnn.cpp)
struct Cnn3Model : rfi_model {
    Cnn3Model(int in, int out, int width) : rfi_model(in, out, width, 0) {}
    void build() override;
    void prepare_shape(int n, int h, int w) override;
    void forward_pass(const float* x_dev, int n, int h, int w, bool train_mode) override;
    void backward_pass(const float* x_dev, const uint8_t* labels_dev, int n, int h, int w) override;
    void algorithmic_flops(int n, int h, int w, double& fwd, double& step) const override;
    int cY1 = -1, cY2 = -1, cG1 = -1, cG2 = -1;
};

// Mask R-CNN's per-RoI mask head (model_mask.cpp; depth = conv layers): depth conv3x3+ReLU layers, a
// transposed conv + ReLU, a 1x1 head, the output map twice the input map in each direction.  Without `upsample`: the RPN
// head (the same stack without the transposed conv)
struct ConvHeadModel : rfi_model {
    const bool upsample;
    ConvHeadModel(int in, int layers, int out, bool up) : rfi_model(in, out, in, layers), upsample(up) {}
    void build() override;
    void prepare_shape(int n, int h, int w) override;
    void forward_pass(const float* x_dev, int n, int h, int w, bool train_mode) override;
    void backward_pass(const float* x_dev, const uint8_t* labels_dev, int n, int h, int w) override;
    void algorithmic_flops(int n, int h, int w, double& fwd, double& step) const override;
    void debug_tensor(const std::string& name, const std::string& base, int idx, bool to_host, rfi::CallScope& sc, const float*& src,
                      size_t& n) override;
    std::vector<int> mkY, mkG;
    int mkU = -1, mkGU = -1, head_wd = -1, head_w3 = -1, head_wd3 = -1;
    // the 1x1 head as a GEMM on the matrix cores (conv kernels forward / input gradient, weight-gradient kernel) instead of the
    // per-pixel VALU kernels written for one output channel: where it has enough outputs (the RPN head's 5 A = 20)
    bool head_on_mfma() const { return out_ch >= 8 && out_ch % 4 == 0 && in_ch % 4 == 0 && arith != Arith::F32; }
    float* head_in() { return upsample ? buf(mkU) : buf(mkY[depth - 1]); }     // what the 1x1 head reads ...
    float* head_din() { return upsample ? buf(mkGU) : buf(mkG[depth - 1]); }   // ... and the gradient it sends down
};

// ResNet-50-FPN backbone with frozen BatchNorm (model_backbone.cpp): feat = base width (64), out_ch = FPN channels
struct BackboneModel : rfi_model {
    BackboneModel(int in, int base_width, int fpn_ch) : rfi_model(in, fpn_ch, base_width, 0) {
        model_copies_every_pass = true;
        dense_head = false;
    }
    ~BackboneModel() override;
    void build() override;
    void prepare_shape(int n, int h, int w) override;
    void forward_pass(const float* x_dev, int n, int h, int w, bool train_mode) override;
    void backward_pass(const float* x_dev, const uint8_t* labels_dev, int n, int h, int w) override;
    void algorithmic_flops(int n, int h, int w, double& fwd, double& step) const override;
    void debug_tensor(const std::string& name, const std::string& base, int idx, bool to_host, rfi::CallScope& sc, const float*& src,
                      size_t& n) override;
    struct BBlock {
        int stage = 0, stride = 1, cin = 0, width = 0, cout = 0, lvl_in = 2, lvl = 2;      // resolution H >> lvl
        int c1 = -1, c2 = -1, c3 = -1, cd = -1;                                           // convs indices (cd: projection shortcut)
        int Y1 = -1, Y2 = -1, Y3 = -1, Yd = -1, A = -1, xs1 = -1, xsA = -1;               // bufs indices
        float *sc4 = nullptr, *sh4 = nullptr;             // conv1's affine coefficients tiled x 4 (space-to-depth input of a stride-2 conv2)
    };
    std::vector<BBlock> bb;
    int fpn_inner[4] = {-1, -1, -1, -1}, fpn_layer[4] = {-1, -1, -1, -1};
    int bY0 = -1, bP0 = -1, bArg = -1, bdW = -1, bS = -1, bCol = -1, bWp = -1, fP6 = -1, fdP6 = -1;
    int stem_kp() const { return (49 * in_ch + 15) / 16 * 16; }      // K of the K-packed 7x7 stem
    int fL[4] = {-1, -1, -1, -1}, fM[4] = {-1, -1, -1, -1}, fP[4] = {-1, -1, -1, -1}, fdM[4] = {-1, -1, -1, -1}, fdP[4] = {-1, -1, -1, -1};
    float* rs_wpool = nullptr;        // derived filters of the stride-2 convs, the stem's records, identity scale / shift
    float* rs_ones = nullptr;
    float* rs_zeros = nullptr;
    float* bb_stem_w3 = nullptr;      // 3 x bf16 records of the K-packed stem filters (rebuilt with them every step)
    int bG[6] = {-1, -1, -1, -1, -1, -1};
    int bT[4][3] = {{-1, -1, -1}, {-1, -1, -1}, {-1, -1, -1}, {-1, -1, -1}};   // dY3 / dY2 / dY1 / dYd of a Bottleneck, by block index mod 3: what the side stream's weight gradients read
    // frozen BatchNorm scale / shift where FROZEN is set, then the 2 x 2 forms of the stride-2 filters
    void refresh_model_weights(rfi::Half half) override;
};

// fully connected box head (model_mlp.cpp): depth FC + ReLU layers in_ch -> feat -> feat, head feat -> out_ch
struct BoxHeadModel : rfi_model {
    BoxHeadModel(int in, int hidden, int layers, int out) : rfi_model(in, out, hidden, layers) {}
    void build() override;
    void prepare_shape(int n, int h, int w) override;
    void forward_pass(const float* x_dev, int n, int h, int w, bool train_mode) override;
    void backward_pass(const float* x_dev, const uint8_t* labels_dev, int n, int h, int w) override;
    void algorithmic_flops(int n, int h, int w, double& fwd, double& step) const override;
    void debug_tensor(const std::string& name, const std::string& base, int idx, bool to_host, rfi::CallScope& sc, const float*& src,
                      size_t& n) override;
    std::vector<int> fcY, fcG;        // raw outputs of the FC layers and their gradients
};
