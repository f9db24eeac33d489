// Training augmentation on the device (scripts/train_model.py:44-53,70-75: HorizontalFlip, VerticalFlip, Rotate(15),
// ShiftScaleRotate(0.05, 0.05, 10), each with p = 0.5, image and mask warped together): the two flips and ONE affine
// warp through the composed transform, where the reference interpolates once per transform.  The semantics are this
// project's own (include/rfi_hip.h): the same distribution of transforms, not the reference
// library's bits.
//
// Sample i of call `call` draws u[0..11] from three Philox4x32-10 blocks, counter (i, call_lo, call_hi, k), key = seed
// (the generator of detect_sample.hip and oracle/synth_ref.philox4x32_10), u = (word + 0.5) 2^-32.  augment_draw turns
// them into the four gates and the row-major 2 x 3 map from an output pixel to its source position; it is the one
// source of both rfi_augment_params (host) and the kernel, which evaluates it per workgroup: nothing is uploaded.
//
// Kernel: a workgroup owns 256 consecutive output pixels of one sample; its first lane draws the sample's transform
// into LDS.  A lane owns one output pixel: all C channels and the mask byte.  Consecutive lanes write consecutive
// pixels (C floats each, in 16-byte pieces when C % 4 == 0) and, the rotations being small, read nearly consecutive
// ones.  A sample with neither rotation nor shift-scale-rotate is copied with the flips applied (bit-exact, whatever
// the values); every other one is a bilinear gather in fp64 rounded once to float32, the mask a nearest-neighbour
// gather, both with reflect-101 borders.  No atomics: the output is a function of the arguments alone.
#include "kernels.hpp"
#include "philox.hpp"

namespace rfi {
namespace {

constexpr int kBlock = 256;


// gates (hflip, vflip, rotate, ssr) and inv = [L | c - L (c + t)], L = F R(-a1) R(-a2) / s: the inverse of
// M = SSR R(a1) Fv Fh about the centre c = ((w - 1) / 2, (h - 1) / 2).  Gated-off factors enter as cos 1, sin 0, s 1,
// t 0, which makes an all-off sample the identity and a flip-only one [-1 0 w-1; 0 1 0] exactly.
__host__ __device__ inline void augment_draw(const rfi_augment_config& cfg, uint64_t call, int i, int h, int w, int* gates,
                                             double* inv) {
    double u[12];
    for (int k = 0; k < 3; ++k) {
        const U4 r = philox4x32_10<false>(U4{(unsigned)i, (unsigned)call, (unsigned)(call >> 32), (unsigned)k}, (unsigned)cfg.seed,
                                   (unsigned)(cfg.seed >> 32));
        u[4 * k + 0] = ((double)r.x + 0.5) * 2.3283064365386963e-10;
        u[4 * k + 1] = ((double)r.y + 0.5) * 2.3283064365386963e-10;
        u[4 * k + 2] = ((double)r.z + 0.5) * 2.3283064365386963e-10;
        u[4 * k + 3] = ((double)r.w + 0.5) * 2.3283064365386963e-10;
    }
    gates[0] = u[0] < (double)cfg.p_hflip;
    gates[1] = u[1] < (double)cfg.p_vflip;
    gates[2] = u[2] < (double)cfg.p_rotate;
    gates[3] = u[3] < (double)cfg.p_ssr;
    const double rad = 0.017453292519943295;
    const double a1 = gates[2] ? (2.0 * u[4] - 1.0) * (double)cfg.rotate_limit_deg * rad : 0.0;
    const double a2 = gates[3] ? (2.0 * u[5] - 1.0) * (double)cfg.ssr_rotate_limit_deg * rad : 0.0;
    const double s = gates[3] ? 1.0 + (2.0 * u[6] - 1.0) * (double)cfg.scale_limit : 1.0;
    const double dx = gates[3] ? (2.0 * u[7] - 1.0) * (double)cfg.shift_limit * (double)w : 0.0;
    const double dy = gates[3] ? (2.0 * u[8] - 1.0) * (double)cfg.shift_limit * (double)h : 0.0;
    const double c1 = gates[2] ? cos(a1) : 1.0, s1 = gates[2] ? sin(a1) : 0.0;
    const double c2 = gates[3] ? cos(a2) : 1.0, s2 = gates[3] ? sin(a2) : 0.0;
    const double pc = c1 * c2 - s1 * s2, ps = c1 * s2 + s1 * c2;          // R(-a1) R(-a2) = [pc ps; -ps pc]
    const double fh = gates[0] ? -1.0 : 1.0, fv = gates[1] ? -1.0 : 1.0;
    const double cx = ((double)w - 1.0) * 0.5, cy = ((double)h - 1.0) * 0.5;
    inv[0] = fh * pc / s;
    inv[1] = fh * ps / s;
    inv[3] = fv * -ps / s;
    inv[4] = fv * pc / s;
    inv[2] = cx - (inv[0] * (cx + dx) + inv[1] * (cy + dy));
    inv[5] = cy - (inv[3] * (cx + dx) + inv[4] * (cy + dy));
}

// reflect-101 of index i into [0, n): period 2 (n - 1), the edge pixel not repeated
__device__ __forceinline__ int reflect101(long long i, int n) {
    if (n == 1) return 0;
    if (i < 0) i = -i;
    if (i >= n) {
        const long long p = 2ll * (n - 1);
        if (i >= p) i %= p;                       // (far outside: only a large scale or shift limit gets here)
        if (i >= n) i = p - i;
    }
    return (int)i;
}

struct alignas(16) F4 { float v[4]; };

// CT: the channel count when it is one of the common ones, 0 = the run-time count c
template <int CT>
__global__ __launch_bounds__(kBlock) void augment_kernel(const float* __restrict__ x, const uint8_t* __restrict__ y, int h, int w, int c,
                                                         int blocks_per_sample, rfi_augment_config cfg, uint64_t call,
                                                         float* __restrict__ xo, uint8_t* __restrict__ yo) {
    __shared__ int s_gates[4];
    __shared__ double s_inv[6];
    const int C = CT ? CT : c;
    const int sample = blockIdx.x / blocks_per_sample;
    const int px = (blockIdx.x - sample * blocks_per_sample) * kBlock + threadIdx.x;
    if (threadIdx.x == 0) augment_draw(cfg, call, sample, h, w, s_gates, s_inv);
    __syncthreads();
    if (px >= h * w) return;
    const int oy = px / w, ox = px - oy * w;
    const int64_t base = (int64_t)sample * h * w;
    const float* xs = x + base * C;
    const uint8_t* ys = y + base;
    float* dst = xo + (base + px) * C;
    if (!s_gates[2] && !s_gates[3]) {             // flips only: a copy, bit for bit
        const int sx = s_gates[0] ? w - 1 - ox : ox, sy = s_gates[1] ? h - 1 - oy : oy;
        const int64_t sp = (int64_t)sy * w + sx;
        const float* src = xs + sp * C;
        if (C % 4 == 0) {
            for (int k = 0; k < C; k += 4) *reinterpret_cast<F4*>(dst + k) = *reinterpret_cast<const F4*>(src + k);
        } else {
            for (int k = 0; k < C; ++k) dst[k] = src[k];
        }
        yo[base + px] = ys[sp];
        return;
    }
    const double fx = s_inv[0] * (double)ox + s_inv[1] * (double)oy + s_inv[2];
    const double fy = s_inv[3] * (double)ox + s_inv[4] * (double)oy + s_inv[5];
    const double x0f = floor(fx), y0f = floor(fy);
    const double tx = fx - x0f, ty = fy - y0f;
    const long long ix = (long long)x0f, iy = (long long)y0f;
    const int xa = reflect101(ix, w), xb = reflect101(ix + 1, w);
    const int ya = reflect101(iy, h), yb = reflect101(iy + 1, h);
    const double w00 = (1.0 - tx) * (1.0 - ty), w01 = tx * (1.0 - ty), w10 = (1.0 - tx) * ty, w11 = tx * ty;
    const float* p00 = xs + ((int64_t)ya * w + xa) * C;
    const float* p01 = xs + ((int64_t)ya * w + xb) * C;
    const float* p10 = xs + ((int64_t)yb * w + xa) * C;
    const float* p11 = xs + ((int64_t)yb * w + xb) * C;
    if (C % 4 == 0) {
        for (int k = 0; k < C; k += 4) {
            const F4 a = *reinterpret_cast<const F4*>(p00 + k), b = *reinterpret_cast<const F4*>(p01 + k);
            const F4 d = *reinterpret_cast<const F4*>(p10 + k), e = *reinterpret_cast<const F4*>(p11 + k);
            F4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                o.v[j] = (float)(((w00 * (double)a.v[j] + w01 * (double)b.v[j]) + w10 * (double)d.v[j]) + w11 * (double)e.v[j]);
            *reinterpret_cast<F4*>(dst + k) = o;
        }
    } else {
        for (int k = 0; k < C; ++k)
            dst[k] = (float)(((w00 * (double)p00[k] + w01 * (double)p01[k]) + w10 * (double)p10[k]) + w11 * (double)p11[k]);
    }
    const int mx = reflect101((long long)floor(fx + 0.5), w), my = reflect101((long long)floor(fy + 0.5), h);
    yo[base + px] = ys[(int64_t)my * w + mx];
}

}  // namespace

void augment_params_host(const rfi_augment_config& cfg, uint64_t call, int n, int h, int w, int32_t* gates, double* inv) {
    for (int i = 0; i < n; ++i) {
        int g[4];
        augment_draw(cfg, call, i, h, w, g, inv + 6 * (size_t)i);
        for (int k = 0; k < 4; ++k) gates[4 * (size_t)i + k] = g[k];
    }
}

void launch_augment(rfi_ctx* ctx, const float* x, const uint8_t* y, int n, int h, int w, int c, const rfi_augment_config& cfg,
                    uint64_t call, float* x_out, uint8_t* y_out) {
    const int64_t px = (int64_t)n * h * w;
    ProfScope ps(ctx, FAM_PREPROCESS, 0, (double)px * 2 * (c * 4 + 1));
    const int bps = (int)cdiv((int64_t)h * w, kBlock);
    const dim3 g((unsigned)((int64_t)n * bps)), b(kBlock);
    switch (c) {
        case 1: hipLaunchKernelGGL(augment_kernel<1>, g, b, 0, ctx->stream, x, y, h, w, c, bps, cfg, call, x_out, y_out); break;
        case 3: hipLaunchKernelGGL(augment_kernel<3>, g, b, 0, ctx->stream, x, y, h, w, c, bps, cfg, call, x_out, y_out); break;
        case 8: hipLaunchKernelGGL(augment_kernel<8>, g, b, 0, ctx->stream, x, y, h, w, c, bps, cfg, call, x_out, y_out); break;
        default: hipLaunchKernelGGL(augment_kernel<0>, g, b, 0, ctx->stream, x, y, h, w, c, bps, cfg, call, x_out, y_out); break;
    }
    check_launch("augment_batch");
}

}  // namespace rfi
