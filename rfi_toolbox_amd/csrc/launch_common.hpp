// Host helpers shared by the baseline flaggers' launch code (sumthreshold.hip, casa_flaggers.hip) and the entry points that
// carve the context's scratch for them (api_flaggers.cpp, rfi_model_predict_flags in api.cpp).
#pragma once
#include "common.hpp"

namespace rfi {

inline size_t dtype_bytes(int dtype) { return dtype == RFI_C128 ? 16 : (dtype == RFI_F32 ? 4 : 8); }

inline size_t al(size_t b) { return (b + 255) & ~(size_t)255; }      // regions of a workspace start 256 bytes aligned

struct Carve {                                              // consecutive 256-byte aligned regions of one workspace
    char* p;
    template <typename T> T* take(size_t count) {
        T* r = reinterpret_cast<T*>(p);
        p += al(count * sizeof(T));
        return r;
    }
};

inline unsigned grid_of(int64_t blocks, const char* what) {
    RFI_REQUIRE(blocks >= 1 && blocks <= 0x7fffffff, std::string(what) + ": too many workgroups for one launch");
    return (unsigned)blocks;
}

// Until disarmed, every exit (an exception included) waits for the context's stream, and for `side` first if there is
// one: a failure part way leaves no work in flight on buffers the caller owns.
struct Drain {
    rfi_ctx* c;
    hipStream_t side = nullptr;
    bool armed = true;
    ~Drain() {
        if (!armed) return;
        if (side) (void)hipStreamSynchronize(side);
        (void)hipStreamSynchronize(c->stream);
    }
};

}  // namespace rfi
