// The bf16 matrix arithmetic of the gfx950 kernels, defined once: the vector types, the float32 -> bf16 conversions,
// the three-piece split of a float32, the transposing LDS fragment read and the MFMA product sequence.
//
// "3 x bf16" float32 emulation.  A float32 value is the exact sum of three bf16 pieces (8 + 8 + 8
// significand bits): h = bf16(v), m = bf16(v - h), l = bf16(v - h - m).  A product a*b is then the sum of nine
// piece products, each exact in the float32 accumulator; the three smallest (m*l, l*m, l*l <= 2^-24 |a b|) are
// dropped, i.e. an error of the size of ONE float32 rounding per product.  Six v_mfma_f32_32x32x16_bf16
// (32 cycles each, K = 16) replace eight v_mfma_f32_32x32x2_f32 (64 cycles each): 2.7x the matrix-pipe
// throughput at float32-level accuracy (tools/mfma_rate.hip: 142 vs 2425 TFLOP/s raw).
#pragma once
#include <hip/hip_runtime.h>

namespace rfi {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef const __attribute__((address_space(1))) void gbl_void;

// two floats -> two bf16 in one register, round-to-nearest-even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned cvt_pair(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
// 4 floats (one lane's k-quad of a fragment) -> 4 bf16, round-to-nearest-even (2 x v_cvt_pk_bf16_f32)
__device__ __forceinline__ s16x4 pack_bf16(float a, float b, float c, float d) {
    const f32x2 lo = {a, b}, hi = {c, d};
    u32x2 r;
    r.x = __builtin_bit_cast(unsigned, __builtin_convertvector(lo, bf16x2));
    r.y = __builtin_bit_cast(unsigned, __builtin_convertvector(hi, bf16x2));
    return __builtin_bit_cast(s16x4, r);
}
__device__ __forceinline__ s16x4 pack_bf16(f32x4 x) { return pack_bf16(x.x, x.y, x.z, x.w); }

// v = h + m + l, each piece RNE-rounded to bf16 (exact: 3 x 8 significand bits cover float32's 24)
// (v_dot2c_f32_bf16 forms a residual "a - float(h.lo)" in one instruction, bit-identically (tools/probe_dot2_split.hip), but
// beside MFMA waves it is SLOWER than shift + subtract -- producer time per item 5.1 k -> 10.1 k cycles, round 3 -- the dot
// instructions appear to share the matrix pipe)
__device__ __forceinline__ void split_pair(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
    h = cvt_pair(a, b);
    const float ra = a - __builtin_bit_cast(float, h << 16), rb = b - __builtin_bit_cast(float, h & 0xffff0000u);
    m = cvt_pair(ra, rb);
    const float sa = ra - __builtin_bit_cast(float, m << 16), sb = rb - __builtin_bit_cast(float, m & 0xffff0000u);
    l = cvt_pair(sa, sb);
}

// one operand fragment: this lane's 8 pixels (k = 8 h + 0..7) of its channel, from two transposing reads of
// 4 pixel rows each.  `p0` / `p1`: byte addresses of THIS lane's row of the two 4x16 blocks
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* p0, const unsigned char* p1) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p0);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p1);
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// acc += A * B for one 32x32x16 block.  P = 1: plain bf16.  P = 3: the float32-by-3xbf16 product, pieces [0] = h,
// [1] = m, [2] = l; small terms first, the three products below 2^-24 |a b| dropped
template <int P>
__device__ __forceinline__ f32x16 mma(const bf16x8 (&a)[P], const bf16x8 (&b)[P], f32x16 acc) {
    static_assert(P == 1 || P == 3, "bf16 or 3 x bf16");
    if constexpr (P == 3) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc, 0, 0, 0);
    }
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc, 0, 0, 0);
}

}  // namespace rfi
