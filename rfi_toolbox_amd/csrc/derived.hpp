// Derived filter copies of a model ("Derived filter copies: who invalidates, who rebuilds"): which of them lag
// behind their sources, and the batched device tables that rebuild them.
#pragma once
#include "planes.hpp"

namespace rfi {

// one bit per row of the DESIGN.md table.  Events set bits (rfi_model::weights_changed / frozen_changed, a mode change);
// rfi_model::sync_filters -- and side_rebuild_wd for the half it left to the side stream -- clears what it rebuilt
enum Copy : unsigned {
    DGRAD = 1,          // dgrad layouts (wd_pool)
    IMAGES_FWD = 2,     // B-operand images of the wave-specialised kernels (ws_pool), forward direction ...
    IMAGES_BWD = 4,     // ... and input-gradient direction (built from the dgrad layouts)
    RECORDS = 8,        // pre-split 3 x bf16 records (w3_pool): stays set while the mode does not read them
    MODEL_FWD = 16,     // the model's own copies (refresh_model_weights): what the forward pass reads ...
    MODEL_BWD = 32,     // ... and what the input-gradient kernels read
    FROZEN = 64,        // frozen-BatchNorm scale / shift: set for every model, read and cleared by the backbone only
    INPUT_GRAD_HALF = DGRAD | IMAGES_BWD | MODEL_BWD,      // what a split rebuild leaves to the side stream
    WEIGHT_DERIVED = INPUT_GRAD_HALF | IMAGES_FWD | MODEL_FWD | RECORDS,
};

// which direction's copies a rebuild covers: what the forward pass reads, what the input-gradient kernels read, or both
enum class Half { Both, Forward, InputGrad };
// the direction(s) whose bit (`fwd`, `bwd`; at least one of them) is set in `bits`
inline Half half_of(unsigned bits, unsigned fwd, unsigned bwd) {
    return !(bits & bwd) ? Half::Forward : !(bits & fwd) ? Half::InputGrad : Half::Both;
}

// a device table of descriptors, one batched rebuild launch per use.  A table of B-operand images (WBDesc) keeps the
// forward-direction descriptors first (n_fwd of them, bytes_fwd of the traffic): launch() rebuilds either half or both
struct BatchTable {
    void* descs = nullptr;
    int n = 0, n_fwd = 0;
    double bytes = 0, bytes_fwd = 0;
    void launch(rfi_ctx* ctx, Half half) const {
        const WBDesc* d = static_cast<const WBDesc*>(descs);
        if (half == Half::Both && n) launch_weights_to_wb(ctx, d, n, bytes);
        if (half == Half::Forward && n_fwd) launch_weights_to_wb(ctx, d, n_fwd, bytes_fwd);
        if (half == Half::InputGrad && n > n_fwd) launch_weights_to_wb(ctx, d + n_fwd, n - n_fwd, bytes - bytes_fwd);
    }
    void release(rfi_ctx* ctx) {
        if (descs) ctx->release(descs);
        *this = BatchTable();
    }
};

// what the list of pre-split records was built for: layers with wave-specialised copies (of ws_P planes) are left out where
// their maps at the prepared H x W are 8 x 8 or larger
struct RecordKey {
    int ws_P = -1, shape = -1;
    bool operator==(const RecordKey& o) const { return ws_P == o.ws_P && shape == o.shape; }
};

}  // namespace rfi
