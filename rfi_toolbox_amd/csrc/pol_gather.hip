// The network input of an 8-channel model straight from the observation: tiling, augmentation views, stacking of the
// four polarisations and the input normalisation in one pass (include/rfi_hip.h, rfi_norm_gather).
//   in   planes (n_samples, 4, C, T) complex128 / complex64, RR RL LR LL, T contiguous
//   out  (n, ps, ps, 8) float32 NHWC, channels RR.re RR.im RL.re ... LL.im, every value norm_value() of its source scalar
//        (a pixel past the view's edge: of 0 + 0j)
// A workgroup owns one 32 x 32 tile of one patch.  Views 0 and 1 (plane, rows flipped) read and write with the lanes
// along the patch row, which is the plane's T axis.  Views 2 and 3 (the transposed ones) have the patch row along the
// plane's C axis: the lanes read along the patch COLUMN (T again, 32 lanes x 8 or 16 B contiguous), leave the eight
// normalised channels in an LDS tile and pick them up transposed, lanes along the patch row, for the stores.  The tile
// rows are 33 floats apart: a 32-lane group writes 32 consecutive words and reads words 33 apart, which are 32
// different banks both times (ds_write_b32 / ds_read_b32 bank = word mod 32, conflicts within a 32-lane half only).
// Every pixel leaves as two 16-byte stores of one lane; consecutive lanes hold consecutive pixels, so a 32-lane group
// writes 1 KiB contiguous.  Algorithmic traffic per pixel: 4 complex values in (32 / 64 B), 32 B out; nothing is read twice.
// No atomics and no reductions: the result does not depend on the launch geometry.
#include <algorithm>

#include "kernels.hpp"

namespace rfi {
namespace {

constexpr int kBlock = 256;
constexpr int kTile = 32;                       // patch pixels per tile side
constexpr int kRows = kBlock / kTile;           // tile rows (or columns) the 32-lane groups of a workgroup take at a time
constexpr int kPitch = kTile + 1;

// vector accesses that ask for the element's alignment only (the buffers are slices of the caller's arrays)
typedef float f32x4 __attribute__((ext_vector_type(4), aligned(4)));
template <typename S> struct Cplx;
template <> struct Cplx<float> { typedef float type __attribute__((ext_vector_type(2), aligned(4))); };
template <> struct Cplx<double> { typedef double type __attribute__((ext_vector_type(2), aligned(8))); };

// the 8 channels of patch pixel whose four source values sit at z[0], z[px], z[2 px], z[3 px] (none when !inside)
template <typename S>
__device__ __forceinline__ void load_channels(const typename Cplx<S>::type* z, int64_t px, bool inside, double centre,
                                              double scale, float* v) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        typename Cplx<S>::type q = {(S)0, (S)0};
        if (inside) q = z[p * px];
        v[2 * p] = norm_value(q.x, centre, scale);
        v[2 * p + 1] = norm_value(q.y, centre, scale);
    }
}
__device__ __forceinline__ void store_channels(float* o, const float* v) {
    *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(o + 4) = f32x4{v[4], v[5], v[6], v[7]};
}

template <typename S>
__global__ __launch_bounds__(kBlock) void pol_gather_kernel(const S* __restrict__ src, const rfi_patch_src* __restrict__ table,
                                                            int C, int T, int ps, int tiles, double centre, double scale,
                                                            const double* __restrict__ params, float* __restrict__ out) {
    __shared__ float s_t[8][kTile][kPitch];                       // [channel][patch column][patch row]
    const int patch = blockIdx.y;
    const rfi_patch_src e = table[patch];
    if (params) {
        centre = params[2 * e.plane];
        scale = params[2 * e.plane + 1];
    }
    const int y0 = (int)(blockIdx.x / tiles) * kTile, x0 = (int)(blockIdx.x % tiles) * kTile;
    const bool tr = e.view >= 2, flip = (e.view & 1) != 0;
    const int Hv = tr ? T : C, Wv = tr ? C : T;
    const int64_t px = (int64_t)C * T;
    const typename Cplx<S>::type* z = reinterpret_cast<const typename Cplx<S>::type*>(src) + (int64_t)e.plane * 4 * px;
    float* o = out + (int64_t)patch * ps * ps * 8;
    const int l = threadIdx.x % kTile, g = threadIdx.x / kTile;
    float v[8];
    if (!tr) {                                                    // view[a][b] = plane[a or C-1-a][b]
        const int x = x0 + l, vx = e.col0 + x;
#pragma unroll
        for (int i = 0; i < kTile / kRows; ++i) {
            const int y = y0 + g + kRows * i, vy = e.row0 + y;
            if (x >= ps || y >= ps) continue;
            const bool inside = vy < Hv && vx < Wv;
            const int sy = flip ? Hv - 1 - vy : vy;
            load_channels<S>(z + ((int64_t)sy * T + vx), px, inside, centre, scale, v);
            store_channels(o + ((int64_t)y * ps + x) * 8, v);
        }
        return;
    }
    {                                                             // view[a][b] = plane[b][a or T-1-a]
        const int y = y0 + l, vy = e.row0 + y;
        const int sx = flip ? Hv - 1 - vy : vy;
#pragma unroll
        for (int i = 0; i < kTile / kRows; ++i) {
            const int xl = g + kRows * i, x = x0 + xl, vx = e.col0 + x;
            if (x >= ps || y >= ps) continue;
            const bool inside = vy < Hv && vx < Wv;
            load_channels<S>(z + ((int64_t)vx * T + sx), px, inside, centre, scale, v);
#pragma unroll
            for (int k = 0; k < 8; ++k) s_t[k][xl][l] = v[k];
        }
    }
    __syncthreads();
    const int x = x0 + l;
#pragma unroll
    for (int i = 0; i < kTile / kRows; ++i) {
        const int yl = g + kRows * i, y = y0 + yl;
        if (x >= ps || y >= ps) continue;
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = s_t[k][l][yl];
        store_channels(o + ((int64_t)y * ps + x) * 8, v);
    }
}

// ---- validity-aware gather (include/rfi_hip.h, rfi_valid_gather): pol_gather_kernel with the validity of every
// visibility decided where it is loaded, from the value and its prior flag byte; nothing else differs
// load_channels with flags: f points at the pixel's byte of polarisation 0 (or is null), fpol is the byte distance
// between polarisations (0 for per-baseline flags); both channels of an invalid visibility are `fill`
template <typename S>
__device__ __forceinline__ void load_channels_valid(const typename Cplx<S>::type* z, const uint8_t* f, int64_t px, int64_t fpol,
                                                    bool inside, double centre, double scale, float fill, float* v) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        typename Cplx<S>::type q = {(S)0, (S)0};
        bool inv = false;
        if (inside) {
            q = z[p * px];
            inv = (f && f[p * fpol] != 0) || !isfinite(q.x) || !isfinite(q.y);
        }
        v[2 * p] = inv ? fill : norm_value(q.x, centre, scale);
        v[2 * p + 1] = inv ? fill : norm_value(q.y, centre, scale);
    }
}

template <typename S>
__global__ __launch_bounds__(kBlock) void pol_gather_valid_kernel(const S* __restrict__ src, const rfi_patch_src* __restrict__ table,
                                                                  int C, int T, int ps, int tiles, double centre, double scale,
                                                                  const double* __restrict__ params,
                                                                  const uint8_t* __restrict__ flags, int64_t fsample, int64_t fpol,
                                                                  float fill, float* __restrict__ out) {
    __shared__ float s_t[8][kTile][kPitch];                       // [channel][patch column][patch row]
    const int patch = blockIdx.y;
    const rfi_patch_src e = table[patch];
    if (params) {
        centre = params[2 * e.plane];
        scale = params[2 * e.plane + 1];
    }
    const int y0 = (int)(blockIdx.x / tiles) * kTile, x0 = (int)(blockIdx.x % tiles) * kTile;
    const bool tr = e.view >= 2, flip = (e.view & 1) != 0;
    const int Hv = tr ? T : C, Wv = tr ? C : T;
    const int64_t px = (int64_t)C * T;
    const typename Cplx<S>::type* z = reinterpret_cast<const typename Cplx<S>::type*>(src) + (int64_t)e.plane * 4 * px;
    const uint8_t* fb = flags ? flags + (int64_t)e.plane * fsample : nullptr;
    float* o = out + (int64_t)patch * ps * ps * 8;
    const int l = threadIdx.x % kTile, g = threadIdx.x / kTile;
    float v[8];
    if (!tr) {                                                    // view[a][b] = plane[a or C-1-a][b]
        const int x = x0 + l, vx = e.col0 + x;
#pragma unroll
        for (int i = 0; i < kTile / kRows; ++i) {
            const int y = y0 + g + kRows * i, vy = e.row0 + y;
            if (x >= ps || y >= ps) continue;
            const bool inside = vy < Hv && vx < Wv;
            const int sy = flip ? Hv - 1 - vy : vy;
            const int64_t at = (int64_t)sy * T + vx;
            load_channels_valid<S>(z + at, fb && inside ? fb + at : nullptr, px, fpol, inside, centre, scale, fill, v);
            store_channels(o + ((int64_t)y * ps + x) * 8, v);
        }
        return;
    }
    {                                                             // view[a][b] = plane[b][a or T-1-a]
        const int y = y0 + l, vy = e.row0 + y;
        const int sx = flip ? Hv - 1 - vy : vy;
#pragma unroll
        for (int i = 0; i < kTile / kRows; ++i) {
            const int xl = g + kRows * i, x = x0 + xl, vx = e.col0 + x;
            if (x >= ps || y >= ps) continue;
            const bool inside = vy < Hv && vx < Wv;
            const int64_t at = (int64_t)vx * T + sx;
            load_channels_valid<S>(z + at, fb && inside ? fb + at : nullptr, px, fpol, inside, centre, scale, fill, v);
#pragma unroll
            for (int k = 0; k < 8; ++k) s_t[k][xl][l] = v[k];
        }
    }
    __syncthreads();
    const int x = x0 + l;
#pragma unroll
    for (int i = 0; i < kTile / kRows; ++i) {
        const int yl = g + kRows * i, y = y0 + yl;
        if (x >= ps || y >= ps) continue;
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = s_t[k][l][yl];
        store_channels(o + ((int64_t)y * ps + x) * 8, v);
    }
}

// merged[b][p][i] = model[b][i] | invalid(b, p, i): one lane per visibility, one byte out
template <typename S>
__global__ __launch_bounds__(kBlock) void valid_merge_kernel(const S* __restrict__ src, const uint8_t* __restrict__ flags,
                                                             int64_t fsample, int64_t fpol, int64_t px, int64_t total,
                                                             const uint8_t* __restrict__ model, uint8_t* __restrict__ merged) {
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= total) return;
    const int64_t plane = gid / px, i = gid - plane * px, b = plane >> 2, p = plane & 3;
    const typename Cplx<S>::type q = reinterpret_cast<const typename Cplx<S>::type*>(src)[gid];
    const bool inv = (flags && flags[b * fsample + p * fpol + i] != 0) || !isfinite(q.x) || !isfinite(q.y);
    merged[gid] = (model[b * px + i] != 0 || inv) ? 1 : 0;
}

// ---- label tiles (include/rfi_hip.h, rfi_label_gather): the label plane of every sample cut into the tiles of the same
// table, one byte per pixel.  out = label | 0x80 where the pixel is invalid -- any (or, all_rule, all) of the npol invalid
// bytes ipol apart -- and `pad` past the view's edge.  Same tile walk as pol_gather_kernel: the transposed views read with
// the lanes along T, stage the bytes in LDS (one word each, rows 33 words apart) and store with the lanes along the patch
// row.  2 to 5 bytes in and one out per pixel
__device__ __forceinline__ unsigned label_byte(const uint8_t* lab, const uint8_t* inv, int64_t at, int npol, int64_t ipol, bool all_rule) {
    unsigned b = lab[at];
    if (inv) {
        bool any = false, all = true;
        for (int p = 0; p < npol; ++p) {
            const bool f = inv[p * ipol + at] != 0;
            any |= f;
            all &= f;
        }
        if (all_rule ? all : any) b |= 0x80u;
    }
    return b;
}

__global__ __launch_bounds__(kBlock) void label_gather_kernel(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ invalid,
                                                              int64_t isample, int64_t ipol, int npol, int all_rule,
                                                              const rfi_patch_src* __restrict__ table, int C, int T, int ps, int tiles,
                                                              unsigned pad, uint8_t* __restrict__ out) {
    __shared__ unsigned s_t[kTile][kPitch];                       // [patch column][patch row]
    const int patch = blockIdx.y;
    const rfi_patch_src e = table[patch];
    const int y0 = (int)(blockIdx.x / tiles) * kTile, x0 = (int)(blockIdx.x % tiles) * kTile;
    const bool tr = e.view >= 2, flip = (e.view & 1) != 0;
    const int Hv = tr ? T : C, Wv = tr ? C : T;
    const int64_t px = (int64_t)C * T;
    const uint8_t* lab = labels + (int64_t)e.plane * px;
    const uint8_t* inv = invalid ? invalid + (int64_t)e.plane * isample : nullptr;
    uint8_t* o = out + (int64_t)patch * ps * ps;
    const int l = threadIdx.x % kTile, g = threadIdx.x / kTile;
    if (!tr) {                                                    // view[a][b] = plane[a or C-1-a][b]
        const int x = x0 + l, vx = e.col0 + x;
#pragma unroll
        for (int i = 0; i < kTile / kRows; ++i) {
            const int y = y0 + g + kRows * i, vy = e.row0 + y;
            if (x >= ps || y >= ps) continue;
            const bool inside = vy < Hv && vx < Wv;
            const int sy = flip ? Hv - 1 - vy : vy;
            o[(int64_t)y * ps + x] = (uint8_t)(inside ? label_byte(lab, inv, (int64_t)sy * T + vx, npol, ipol, all_rule != 0) : pad);
        }
        return;
    }
    {                                                             // view[a][b] = plane[b][a or T-1-a]
        const int y = y0 + l, vy = e.row0 + y;
        const int sx = flip ? Hv - 1 - vy : vy;
#pragma unroll
        for (int i = 0; i < kTile / kRows; ++i) {
            const int xl = g + kRows * i, x = x0 + xl, vx = e.col0 + x;
            if (x >= ps || y >= ps) continue;
            const bool inside = vy < Hv && vx < Wv;
            s_t[xl][l] = inside ? label_byte(lab, inv, (int64_t)vx * T + sx, npol, ipol, all_rule != 0) : pad;
        }
    }
    __syncthreads();
    const int x = x0 + l;
#pragma unroll
    for (int i = 0; i < kTile / kRows; ++i) {
        const int yl = g + kRows * i, y = y0 + yl;
        if (x >= ps || y >= ps) continue;
        o[(int64_t)y * ps + x] = (uint8_t)s_t[l][yl];
    }
}

}  // namespace

void launch_label_gather(rfi_ctx* ctx, const uint8_t* labels_dev, int C, int T, const uint8_t* invalid_dev, bool per_baseline,
                         bool all_rule, const rfi_patch_src* table_dev, int n, int ps, int pad_value, uint8_t* out) {
    RFI_REQUIRE(C > 0 && T > 0 && ps > 0 && n >= 0, "label_gather: bad shape");
    if (n == 0) return;
    const size_t per = (size_t)ps * ps;
    const int64_t px = (int64_t)C * T, isample = per_baseline ? px : 4 * px, ipol = per_baseline ? 0 : px;
    ProfScope pf(ctx, FAM_PREPROCESS, 0, (double)n * per * (2 + (invalid_dev ? (per_baseline ? 1 : 4) : 0)), "label_gather");
    const int tiles = (int)cdiv(ps, kTile);
    RFI_REQUIRE((int64_t)tiles * tiles <= 0x7fffffff, "label_gather: patch too large for one launch");
    for (int n0 = 0; n0 < n; n0 += kMaxGridY) {
        const dim3 grid((unsigned)(tiles * tiles), (unsigned)std::min(n - n0, kMaxGridY));
        hipLaunchKernelGGL(label_gather_kernel, grid, dim3(kBlock), 0, ctx->stream, labels_dev, invalid_dev, isample, ipol,
                           per_baseline ? 1 : 4, (int)all_rule, table_dev + n0, C, T, ps, tiles, (unsigned)(pad_value & 0xFF),
                           out + (size_t)n0 * per);
        check_launch("label_gather");
    }
}

void launch_pol_gather_valid(rfi_ctx* ctx, const void* planes, int dtype, int C, int T, const rfi_patch_src* table_dev, int n, int ps,
                             double centre, double scale, const double* params_dev, const uint8_t* flags_dev, bool per_baseline,
                             float fill, float* out_nhwc) {
    RFI_REQUIRE(dtype == RFI_C128 || dtype == RFI_C64, "valid_gather: planes must be complex128 or complex64");
    RFI_REQUIRE(C > 0 && T > 0 && ps > 0 && n >= 0, "valid_gather: bad shape");
    if (n == 0) return;
    const size_t per = (size_t)ps * ps;
    const int64_t px = (int64_t)C * T, fsample = per_baseline ? px : 4 * px, fpol = per_baseline ? 0 : px;
    ProfScope pf(ctx, FAM_PREPROCESS, 0, (double)n * per * ((dtype == RFI_C128 ? 64 : 32) + 32 + (flags_dev ? (per_baseline ? 1 : 4) : 0)),
                 "pol_gather_valid");
    const int tiles = (int)cdiv(ps, kTile);
    RFI_REQUIRE((int64_t)tiles * tiles <= 0x7fffffff, "valid_gather: patch too large for one launch");
    for (int n0 = 0; n0 < n; n0 += kMaxGridY) {
        const dim3 grid((unsigned)(tiles * tiles), (unsigned)std::min(n - n0, kMaxGridY));
        if (dtype == RFI_C128)
            hipLaunchKernelGGL(pol_gather_valid_kernel<double>, grid, dim3(kBlock), 0, ctx->stream, static_cast<const double*>(planes),
                               table_dev + n0, C, T, ps, tiles, centre, scale, params_dev, flags_dev, fsample, fpol, fill,
                               out_nhwc + (size_t)n0 * per * 8);
        else
            hipLaunchKernelGGL(pol_gather_valid_kernel<float>, grid, dim3(kBlock), 0, ctx->stream, static_cast<const float*>(planes),
                               table_dev + n0, C, T, ps, tiles, centre, scale, params_dev, flags_dev, fsample, fpol, fill,
                               out_nhwc + (size_t)n0 * per * 8);
        check_launch("pol_gather_valid");
    }
}

void launch_valid_merge(rfi_ctx* ctx, const void* planes, int dtype, int n_samples, int64_t px, const uint8_t* flags_dev,
                        bool per_baseline, const uint8_t* model_flags, uint8_t* merged) {
    RFI_REQUIRE(dtype == RFI_C128 || dtype == RFI_C64, "valid_merge: planes must be complex128 or complex64");
    const int64_t total = (int64_t)n_samples * 4 * px;
    if (total == 0) return;
    RFI_REQUIRE(cdiv(total, kBlock) <= 0x7fffffff, "valid_merge: too many visibilities for one launch");
    ProfScope pf(ctx, FAM_PREPROCESS, 0, (double)total * ((dtype == RFI_C128 ? 16 : 8) + 2.25), "valid_merge");
    const int64_t fsample = per_baseline ? px : 4 * px, fpol = per_baseline ? 0 : px;
    const dim3 grid((unsigned)cdiv(total, kBlock));
    if (dtype == RFI_C128)
        hipLaunchKernelGGL(valid_merge_kernel<double>, grid, dim3(kBlock), 0, ctx->stream, static_cast<const double*>(planes), flags_dev,
                           fsample, fpol, px, total, model_flags, merged);
    else
        hipLaunchKernelGGL(valid_merge_kernel<float>, grid, dim3(kBlock), 0, ctx->stream, static_cast<const float*>(planes), flags_dev,
                           fsample, fpol, px, total, model_flags, merged);
    check_launch("valid_merge");
}

void launch_pol_gather(rfi_ctx* ctx, const void* planes, int dtype, int C, int T, const rfi_patch_src* table_dev, int n, int ps,
                       double centre, double scale, const double* params_dev, float* out_nhwc) {
    RFI_REQUIRE(dtype == RFI_C128 || dtype == RFI_C64, "norm_gather: planes must be complex128 or complex64");
    RFI_REQUIRE(C > 0 && T > 0 && ps > 0 && n >= 0, "norm_gather: bad shape");
    if (n == 0) return;
    const size_t per = (size_t)ps * ps;
    ProfScope pf(ctx, FAM_PREPROCESS, 0, (double)n * per * ((dtype == RFI_C128 ? 64 : 32) + 32), "pol_gather");
    const int tiles = (int)cdiv(ps, kTile);
    RFI_REQUIRE((int64_t)tiles * tiles <= 0x7fffffff, "norm_gather: patch too large for one launch");
    for (int n0 = 0; n0 < n; n0 += kMaxGridY) {
        const dim3 grid((unsigned)(tiles * tiles), (unsigned)std::min(n - n0, kMaxGridY));
        if (dtype == RFI_C128)
            hipLaunchKernelGGL(pol_gather_kernel<double>, grid, dim3(kBlock), 0, ctx->stream, static_cast<const double*>(planes),
                               table_dev + n0, C, T, ps, tiles, centre, scale, params_dev, out_nhwc + (size_t)n0 * per * 8);
        else
            hipLaunchKernelGGL(pol_gather_kernel<float>, grid, dim3(kBlock), 0, ctx->stream, static_cast<const float*>(planes),
                               table_dev + n0, C, T, ps, tiles, centre, scale, params_dev, out_nhwc + (size_t)n0 * per * 8);
        check_launch("pol_gather");
    }
}

}  // namespace rfi
