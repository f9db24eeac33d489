// Instance stitch: the per-tile detections of a tiled observation -> one event per emitter of the whole plane (include/rfi_hip.h,
// "instance stitch"; the instance counterpart of stitch.hip).  Every quantity is a min, a max, an OR or a sort on a total order:
// the result is bitwise reproducible and independent of launch order.  Seven launches, each after the one before has ended:
//   1 member   one workgroup per (tile, slot) reads the slot's mask once with 16-byte loads: in-plane area and bounding box,
//              the member decision, the mapped float32 box; initialises the slot's node (parent, box and score accumulators)
//   2 link     one workgroup per pair of tiles whose rectangles intersect or abut (host table, cached per shape): lanes test
//              64 slot pairs at a time on label and bounding box, one ballot picks the candidates, and the wave walks the
//              shared bounding box of a candidate until one pixel proves the link; unions by atomicMin (union_find.hpp)
//   3 reduce   root of every member; box (min / min / max / max) and best (score, smallest index) to the root with integer
//              atomics on order-preserving images of the floats
//   4 keys     one 64-bit key per slot: (descending score, ascending id) for a root, the largest key for anything else
//   5 sort     launch_segsort_u64, one segment per plane
//   6 emit     rank of every root; boxes, scores, labels and counts of the first max_events
//   7 paste    gather form as in stitch.hip: a thread owns one plane pixel, visits every covering tile and its member slots
//              (bounding box first, then the mask byte), ORs into rfi_mask and sets the pixel in the event's mask plane
// The grid, the tile order of the host table and the walk over covering tiles are those of tiling.hpp.
// The mask bytes dominate: N D ps^2 in (read once by 1; 7 reads the bytes inside member boxes only), P E C T out.
#include <algorithm>
#include <map>
#include <memory>
#include <tuple>

#include "kernels.hpp"
#include "launch_common.hpp"
#include "tiling.hpp"
#include "union_find.hpp"

namespace rfi {
namespace {

constexpr int kBlock = 256;
constexpr unsigned long long kNoKey = ~0ull;

struct TileDesc {          // one tile of a plane: its view and origin, and its rectangle in plane coordinates (half open)
    int view, row0, col0, pad_;
    int c0, c1, t0, t1;
};
struct TilePair {          // tiles a < b of a plane; kind 0: the rectangles intersect, 1: they are disjoint and abut
    int a, b, kind, pad_;
};
struct Geo : TileGrid {    // (ppp x D <= 65536 here: the kernels index a plane's tiles and slots with int)
    int D;
};

// order-preserving integer images of a float (finite or infinite): signed for atomicMin / atomicMax, unsigned for sort keys
__device__ __forceinline__ int ord_i(float f) {
    const int i = __float_as_int(f);
    return i ^ ((i >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float ord_i_inv(int i) { return __int_as_float(i ^ ((i >> 31) & 0x7fffffff)); }
__device__ __forceinline__ unsigned ord_u(float f) {
    const unsigned u = (unsigned)__float_as_int(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_u_inv(unsigned u) { return __int_as_float((int)((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u)); }

// offset of plane pixel (c, t) inside a tile, -1 when the tile does not hold it
__device__ __forceinline__ int tile_offset(const TileDesc& d, const Geo& g, int c, int t) {
    const ViewPixel p = view_pixel(g, d.view, c, t);
    const int r = p.y - d.row0, cc = p.x - d.col0;
    if ((unsigned)r >= (unsigned)g.ps || (unsigned)cc >= (unsigned)g.ps) return -1;
    return r * g.ps + cc;
}

__device__ __forceinline__ int cut_count(const int* counts, int64_t tile, int D) { return min(max(counts[tile], 0), D); }

// ---- 1: grid (N D).  WIDE: ps % 16 == 0 and `masks` 16-byte aligned
template <bool WIDE>
__global__ void __launch_bounds__(kBlock) member_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                        const int* __restrict__ counts, const uint8_t* __restrict__ masks,
                                                        const TileDesc* __restrict__ tiles, Geo g, int min_area, float min_score,
                                                        int4* __restrict__ mbox, int* __restrict__ parent, int4* __restrict__ acc_box,
                                                        unsigned long long* __restrict__ acc_key) {
    __shared__ int red[kBlock / 64][5];
    const int m = blockIdx.x, tile = m / g.D, slot = m % g.D;
    const int4 empty = make_int4(1, 0, 1, 0);
    if (slot >= cut_count(counts, tile, g.D) || !(scores[m] >= min_score)) {       // (uniform over the workgroup)
        if (threadIdx.x == 0) {
            mbox[m] = empty;
            parent[m] = -1;
        }
        return;
    }
    const int in_plane = tile % (int)g.ppp;
    const TileDesc d = tiles[in_plane];
    const bool tr = d.view >= 2;
    const int Hv = tr ? g.T : g.C, Wv = tr ? g.C : g.T;
    const int rows = min(g.ps, Hv - d.row0), cols = min(g.ps, Wv - d.col0);       // the tile's non-padding part
    const uint8_t* mk = masks + (int64_t)m * g.ps * g.ps;
    int area = 0, r_lo = g.ps, r_hi = -1, c_lo = g.ps, c_hi = -1;
    auto take = [&](int r, int cc) {
        ++area;
        r_lo = min(r_lo, r);
        r_hi = max(r_hi, r);
        c_lo = min(c_lo, cc);
        c_hi = max(c_hi, cc);
    };
    if (WIDE) {
        const int per_row = g.ps / 16, n16 = rows * per_row;                       // (padding rows are never read)
        for (int i = threadIdx.x; i < n16; i += kBlock) {
            const int r = i / per_row, cc0 = (i % per_row) * 16;
            if (cc0 >= cols) continue;
            const uint4 v = *reinterpret_cast<const uint4*>(mk + (int64_t)r * g.ps + cc0);
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (((w[k >> 2] >> (8 * (k & 3))) & 0xffu) && cc0 + k < cols) take(r, cc0 + k);
        }
    } else {
        for (int i = threadIdx.x; i < rows * g.ps; i += kBlock) {
            const int r = i / g.ps, cc = i % g.ps;
            if (cc < cols && mk[i]) take(r, cc);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        area += __shfl_xor(area, o, 64);
        r_lo = min(r_lo, __shfl_xor(r_lo, o, 64));
        r_hi = max(r_hi, __shfl_xor(r_hi, o, 64));
        c_lo = min(c_lo, __shfl_xor(c_lo, o, 64));
        c_hi = max(c_hi, __shfl_xor(c_hi, o, 64));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[wave][0] = area;
        red[wave][1] = r_lo;
        red[wave][2] = r_hi;
        red[wave][3] = c_lo;
        red[wave][4] = c_hi;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < kBlock / 64; ++w) {
        area += red[w][0];
        r_lo = min(r_lo, red[w][1]);
        r_hi = max(r_hi, red[w][2]);
        c_lo = min(c_lo, red[w][3]);
        c_hi = max(c_hi, red[w][4]);
    }
    if (area < min_area) {
        mbox[m] = empty;
        parent[m] = -1;
        return;
    }
    // bounding box of the in-plane pixels, tile -> view -> plane (inclusive)
    int y0 = d.row0 + r_lo, y1 = d.row0 + r_hi;
    const int x0 = d.col0 + c_lo, x1 = d.col0 + c_hi;
    if (d.view & 1) {
        const int a = Hv - 1 - y1, b = Hv - 1 - y0;
        y0 = a;
        y1 = b;
    }
    mbox[m] = tr ? make_int4(x0, x1, y0, y1) : make_int4(y0, y1, x0, x1);
    parent[m] = m;
    // the box: add the origin, mirror, transpose, restore the order, clip -- float32, one operation per step
    const float* bx = boxes + (int64_t)m * 4;
    float bx1 = bx[0] + (float)d.col0, by1 = bx[1] + (float)d.row0, bx2 = bx[2] + (float)d.col0, by2 = bx[3] + (float)d.row0;
    if (d.view & 1) {
        by1 = (float)Hv - by1;
        by2 = (float)Hv - by2;
    }
    if (tr) {
        float t_ = bx1; bx1 = by1; by1 = t_;
        t_ = bx2; bx2 = by2; by2 = t_;
    }
    if (bx1 > bx2) { const float t_ = bx1; bx1 = bx2; bx2 = t_; }
    if (by1 > by2) { const float t_ = by1; by1 = by2; by2 = t_; }
    const float fT = (float)g.T, fC = (float)g.C;
    bx1 = fminf(fmaxf(bx1, 0.0f), fT);
    bx2 = fminf(fmaxf(bx2, 0.0f), fT);
    by1 = fminf(fmaxf(by1, 0.0f), fC);
    by2 = fminf(fmaxf(by2, 0.0f), fC);
    acc_box[m] = make_int4(ord_i(bx1), ord_i(by1), ord_i(bx2), ord_i(by2));
    const unsigned local = (unsigned)(in_plane * g.D + slot);
    acc_key[m] = ((unsigned long long)ord_u(scores[m]) << 32) | (0xffffffffu - local);       // max: best score, then smallest index
}

// ---- 2: grid (pairs, planes)
__global__ void __launch_bounds__(kBlock) link_kernel(const int* __restrict__ labels, const int* __restrict__ counts,
                                                      const uint8_t* __restrict__ masks, const TileDesc* __restrict__ tiles,
                                                      const TilePair* __restrict__ pairs, Geo g, int class_aware, int conn8,
                                                      const int4* __restrict__ mbox, int* parent) {
    const TilePair pr = pairs[blockIdx.x];
    const int ppp = (int)g.ppp;
    const int ta = blockIdx.y * ppp + pr.a, tb = blockIdx.y * ppp + pr.b;
    const int ca = cut_count(counts, ta, g.D), cb = cut_count(counts, tb, g.D);
    if (ca == 0 || cb == 0) return;
    const TileDesc da = tiles[pr.a], db = tiles[pr.b];
    const int grow = pr.kind;                                 // abutting rectangles: b's box grown by the one pixel of adjacency
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, total = ca * cb;
    const int64_t ps2 = (int64_t)g.ps * g.ps;
    const AgentLoad ld;
    for (int base = wave * 64; base < total; base += (kBlock / 64) * 64) {
        const int idx = base + lane;
        int ma = 0, mb = 0;
        int4 box = make_int4(1, 0, 1, 0);                     // a's box cut to b's (grown) box
        if (idx < total) {
            ma = ta * g.D + idx / cb;
            mb = tb * g.D + idx % cb;
            const int4 ba = mbox[ma], bb = mbox[mb];
            if (ba.x <= ba.y && bb.x <= bb.y && (!class_aware || labels[ma] == labels[mb]))
                box = make_int4(max(ba.x, bb.x - grow), min(ba.y, bb.y + grow), max(ba.z, bb.z - grow), min(ba.w, bb.w + grow));
        }
        unsigned long long cand = __ballot(box.x <= box.y && box.z <= box.w);
        while (cand) {                                        // (uniform over the wave)
            const int l = __ffsll((long long)cand) - 1;
            cand &= cand - 1;
            const int a = __shfl(ma, l, 64), b = __shfl(mb, l, 64);
            const int c0 = __shfl(box.x, l, 64), c1 = __shfl(box.y, l, 64), t0 = __shfl(box.z, l, 64), t1 = __shfl(box.w, l, 64);
            // joined already, by this pair or another?  One lane looks, so that the whole wave takes the same way
            const int joined = lane == 0 ? (find_root(parent, a, ld) == find_root(parent, b, ld) ? 1 : 0) : 0;
            if (__shfl(joined, 0, 64)) continue;
            const uint8_t* pa = masks + a * ps2;
            const uint8_t* pb = masks + b * ps2;
            const int w = t1 - t0 + 1, n = (c1 - c0 + 1) * w;
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                bool hit = false;
                if (i < n) {
                    const int c = c0 + i / w, t = t0 + i % w;
                    const int oa = tile_offset(da, g, c, t);
                    if (oa >= 0 && pa[oa]) {
                        if (pr.kind == 0) {
                            const int ob = tile_offset(db, g, c, t);
                            hit = ob >= 0 && pb[ob];
                        } else {
                            for (int dc = -1; dc <= 1; ++dc)
                                for (int dt = -1; dt <= 1; ++dt) {
                                    if ((dc == 0 && dt == 0) || (!conn8 && dc != 0 && dt != 0)) continue;
                                    const int cn = c + dc, tn = t + dt;
                                    if (cn < 0 || cn >= g.C || tn < 0 || tn >= g.T) continue;
                                    const int ob = tile_offset(db, g, cn, tn);
                                    if (ob >= 0 && pb[ob]) hit = true;
                                }
                        }
                    }
                }
                if (__any(hit)) {
                    if (lane == 0) unite(parent, a, b, ld);
                    break;
                }
            }
        }
    }
}

// ---- 3: grid (cdiv(N D, kBlock)).  The link launch has ended: plain loads; `root` is written, `parent` only read
__global__ void __launch_bounds__(kBlock) reduce_kernel(const int* __restrict__ parent, int64_t nd, int* __restrict__ root,
                                                        int4* acc_box, unsigned long long* acc_key) {
    const int64_t m = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (m >= nd) return;
    int r = parent[m];
    if (r >= 0) r = find_root(parent, (int)m, PlainLoad());
    root[m] = r;
    if (r < 0 || r == m) return;
    const int4 b = acc_box[m];                                 // (a non-root's own accumulators are never written)
    int* rb = reinterpret_cast<int*>(acc_box + r);
    atomicMin(rb + 0, b.x);
    atomicMin(rb + 1, b.y);
    atomicMax(rb + 2, b.z);
    atomicMax(rb + 3, b.w);
    atomicMax(acc_key + r, acc_key[m]);
}

// ---- 4: grid (cdiv(stride, kBlock), planes)
__global__ void __launch_bounds__(kBlock) keys_kernel(const int* __restrict__ root, const unsigned long long* __restrict__ acc_key,
                                                      int per_plane, int stride, unsigned long long* __restrict__ keys) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= stride) return;
    unsigned long long key = kNoKey;
    if (i < per_plane) {
        const int64_t m = (int64_t)blockIdx.y * per_plane + i;
        if (root[m] == m) key = ((unsigned long long)(~(unsigned)(acc_key[m] >> 32)) << 32) | (unsigned)i;
    }
    keys[(int64_t)blockIdx.y * stride + i] = key;
}

// ---- 6: grid (cdiv(stride, kBlock), planes); the outputs were zeroed
__global__ void __launch_bounds__(kBlock) emit_kernel(const unsigned long long* __restrict__ keys, int per_plane, int stride, int E,
                                                      const int* __restrict__ labels, const int4* __restrict__ acc_box,
                                                      const unsigned long long* __restrict__ acc_key, int* __restrict__ rank_of,
                                                      float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                      int* __restrict__ out_labels, int* __restrict__ out_counts) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= stride) return;
    const int64_t plane = blockIdx.y, base = plane * per_plane;
    const unsigned long long key = keys[plane * stride + k];
    if (key == kNoKey) return;                                 // (the valid keys are a prefix of the sorted segment)
    if (k + 1 == stride || keys[plane * stride + k + 1] == kNoKey) out_counts[plane] = min(k + 1, E);
    const int64_t m = base + (unsigned)key;
    rank_of[m] = k;
    if (k >= E) return;
    const int4 b = acc_box[m];
    const unsigned long long best = acc_key[m];
    float* ob = out_boxes + (plane * E + k) * 4;
    ob[0] = ord_i_inv(b.x);
    ob[1] = ord_i_inv(b.y);
    ob[2] = ord_i_inv(b.z);
    ob[3] = ord_i_inv(b.w);
    out_scores[plane * E + k] = ord_u_inv((unsigned)(best >> 32));
    out_labels[plane * E + k] = labels[base + (0xffffffffu - (unsigned)best)];
}

// ---- 7: block (64, 4), grid (cdiv(T, 64), cdiv(C, 4), planes); out_masks was zeroed
__global__ void __launch_bounds__(256) paste_kernel(const int* __restrict__ counts, const uint8_t* __restrict__ masks, Geo g,
                                                    const int4* __restrict__ mbox, const int* __restrict__ root,
                                                    const int* __restrict__ rank_of, int E, uint8_t* __restrict__ rfi_mask,
                                                    uint8_t* __restrict__ out_masks) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y * blockDim.y + threadIdx.y;
    const int64_t plane = blockIdx.z;
    if (t >= g.T || c >= g.C) return;
    const int64_t ps2 = (int64_t)g.ps * g.ps, px = (int64_t)g.C * g.T;
    uint8_t any = 0;
    for_each_covering_tile<int>(g, c, t, [&](int tile_in_plane, int off) {          // (ppp x D <= 65536, ps <= 32768)
        const int64_t tile = plane * g.ppp + tile_in_plane;
        const int cnt = cut_count(counts, tile, g.D);
        for (int k = 0; k < cnt; ++k) {
            const int64_t m = tile * g.D + k;
            const int4 b = mbox[m];
            if (c < b.x || c > b.y || t < b.z || t > b.w || !masks[m * ps2 + off]) continue;
            any = 1;
            if (out_masks) {
                const int rk = rank_of[root[m]];
                if (rk < E) out_masks[(plane * E + rk) * px + (int64_t)c * g.T + t] = 1;
            }
        }
    });
    rfi_mask[plane * px + (int64_t)c * g.T + t] = any;
}

// ---- the host tables of one (C, T, tiling): tiles of a plane in rfi_tiling order, pairs whose rectangles intersect or abut
struct Tables {
    std::vector<TileDesc> tiles;
    std::vector<TilePair> pairs;
};

const Tables& tables_for(int C, int T, const rfi_tiling& tl) {
    static std::mutex mu;
    static std::map<std::tuple<int, int, int, int, int, int>, std::unique_ptr<Tables>> cache;
    std::lock_guard<std::mutex> lock(mu);
    auto& slot = cache[std::make_tuple(C, T, tl.ps, tl.stride, tl.edge, tl.views)];
    if (slot) return *slot;
    auto tb = std::make_unique<Tables>();
    const TileGrid g = make_tile_grid(C, T, tl);
    for (const rfi_patch_src& e : tile_table(g, 1)) {
        const int v = e.view;
        const ViewPixel vw = view_pixel(g, v, 0, 0);
        TileDesc d{};
        d.view = v;
        d.row0 = e.row0;
        d.col0 = e.col0;
        int y0 = d.row0, y1 = std::min(d.row0 + g.ps, vw.Hv);
        const int x0 = d.col0, x1 = std::min(d.col0 + g.ps, vw.Wv);
        if (v & 1) {
            const int a = vw.Hv - y1, b = vw.Hv - y0;
            y0 = a;
            y1 = b;
        }
        if (v >= 2) { d.c0 = x0; d.c1 = x1; d.t0 = y0; d.t1 = y1; }
        else { d.c0 = y0; d.c1 = y1; d.t0 = x0; d.t1 = x1; }
        tb->tiles.push_back(d);
    }
    const int n = (int)tb->tiles.size();
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b) {
            const TileDesc &p = tb->tiles[a], &q = tb->tiles[b];
            const bool meet = p.c0 < q.c1 && q.c0 < p.c1 && p.t0 < q.t1 && q.t0 < p.t1;
            const bool near = p.c0 <= q.c1 && q.c0 <= p.c1 && p.t0 <= q.t1 && q.t0 <= p.t1;      // gap of at most one pixel edge
            if (near) tb->pairs.push_back(TilePair{a, b, meet ? 0 : 1, 0});
        }
    slot = std::move(tb);
    return *slot;
}

int sort_stride(int64_t per_plane) {
    int s = 2;
    while (s < per_plane) s <<= 1;
    return s;
}

}  // namespace

void launch_stitch_instances(rfi_ctx* ctx, const float* boxes, const float* scores, const int* labels, const int* counts,
                             const uint8_t* masks, int n_planes, int C, int T, const rfi_tiling& tl, int D, int max_events, int min_area,
                             float min_score, int class_aware, int connectivity, float* out_boxes, float* out_scores, int* out_labels,
                             int* out_counts, uint8_t* rfi_mask, uint8_t* out_masks) {
    check_tiling(tl);
    RFI_REQUIRE(C > 0 && T > 0 && (int64_t)C * T < ((int64_t)1 << 31), "stitch_instances: planes of 1 .. 2^31 - 1 pixels");
    RFI_REQUIRE(n_planes >= 0 && n_planes <= 65535, "stitch_instances: at most 65535 planes per call");
    RFI_REQUIRE(D >= 1 && D <= 256, "stitch_instances: 1 <= D <= 256");
    RFI_REQUIRE(max_events >= 1 && max_events <= 256, "stitch_instances: 1 <= max_events <= 256");
    RFI_REQUIRE(min_area >= 1, "stitch_instances: min_area must be at least 1");
    RFI_REQUIRE(connectivity == 4 || connectivity == 8, "stitch_instances: connectivity must be 4 or 8");
    RFI_REQUIRE(tl.ps <= 32768, "stitch_instances: patch size at most 32768");
    if (n_planes == 0) return;
    const int64_t ppp = tiling_patches_per_plane(C, T, tl), per_plane = ppp * D, nd = per_plane * n_planes;
    RFI_REQUIRE(per_plane <= 65536, "stitch_instances: patches per plane x D must not exceed 65536 (the ranking sorts one segment per plane)");
    RFI_REQUIRE(nd < ((int64_t)1 << 31), "stitch_instances: fewer than 2^31 detection slots per call");
    RFI_REQUIRE(cdiv(C, 4) <= 65535, "stitch_instances: at most 262140 channels");
    const Tables& tb = tables_for(C, T, tl);
    const int stride = sort_stride(per_plane), E = max_events;
    Geo g{make_tile_grid(C, T, tl), D};

    const size_t n_pairs = tb.pairs.size();
    const size_t bytes = al(tb.tiles.size() * sizeof(TileDesc)) + al(n_pairs * sizeof(TilePair)) + 2 * al(nd * sizeof(int4)) +
                         3 * al(nd * sizeof(int)) + al(nd * sizeof(unsigned long long)) +
                         al((size_t)n_planes * stride * sizeof(unsigned long long));
    Carve ws{static_cast<char*>(ctx->get_scratch(bytes))};
    TileDesc* d_tiles = ws.take<TileDesc>(tb.tiles.size());
    TilePair* d_pairs = ws.take<TilePair>(n_pairs);
    int4* mbox = ws.take<int4>(nd);
    int4* acc_box = ws.take<int4>(nd);
    int* parent = ws.take<int>(nd);
    int* root = ws.take<int>(nd);
    int* rank_of = ws.take<int>(nd);
    auto* acc_key = ws.take<unsigned long long>(nd);
    auto* keys = ws.take<unsigned long long>((size_t)n_planes * stride);
    hipStream_t st = ctx->stream;
    // (the tables live in the cache for the life of the process: the copies may read them after this call returns)
    RFI_CHECK_HIP(hipMemcpyAsync(d_tiles, tb.tiles.data(), tb.tiles.size() * sizeof(TileDesc), hipMemcpyHostToDevice, st));
    if (n_pairs) RFI_CHECK_HIP(hipMemcpyAsync(d_pairs, tb.pairs.data(), n_pairs * sizeof(TilePair), hipMemcpyHostToDevice, st));
    RFI_CHECK_HIP(hipMemsetAsync(out_boxes, 0, (size_t)n_planes * E * 4 * sizeof(float), st));
    RFI_CHECK_HIP(hipMemsetAsync(out_scores, 0, (size_t)n_planes * E * sizeof(float), st));
    RFI_CHECK_HIP(hipMemsetAsync(out_labels, 0, (size_t)n_planes * E * sizeof(int), st));
    RFI_CHECK_HIP(hipMemsetAsync(out_counts, 0, (size_t)n_planes * sizeof(int), st));
    if (out_masks) RFI_CHECK_HIP(hipMemsetAsync(out_masks, 0, (size_t)n_planes * E * C * T, st));

    const double mask_bytes = (double)nd * tl.ps * tl.ps;
    {
        ProfScope p_(ctx, FAM_METRICS, 0, mask_bytes, "stitch_inst_member");
        const bool wide = tl.ps % 16 == 0 && reinterpret_cast<uintptr_t>(masks) % 16 == 0;
        if (wide)
            hipLaunchKernelGGL(member_kernel<true>, dim3((unsigned)nd), dim3(kBlock), 0, st, boxes, scores, counts, masks, d_tiles, g,
                               min_area, min_score, mbox, parent, acc_box, acc_key);
        else
            hipLaunchKernelGGL(member_kernel<false>, dim3((unsigned)nd), dim3(kBlock), 0, st, boxes, scores, counts, masks, d_tiles, g,
                               min_area, min_score, mbox, parent, acc_box, acc_key);
        check_launch("stitch_inst_member");
    }
    if (n_pairs) {
        ProfScope p_(ctx, FAM_METRICS, 0, 0, "stitch_inst_link");
        hipLaunchKernelGGL(link_kernel, dim3(grid_of((int64_t)n_pairs, "stitch_instances"), (unsigned)n_planes), dim3(kBlock), 0, st, labels,
                           counts, masks, d_tiles, d_pairs, g, class_aware ? 1 : 0, connectivity == 8 ? 1 : 0, mbox, parent);
        check_launch("stitch_inst_link");
    }
    {
        ProfScope p_(ctx, FAM_METRICS, 0, (double)nd * 40, "stitch_inst_rank");
        hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)cdiv(nd, kBlock)), dim3(kBlock), 0, st, parent, nd, root, acc_box, acc_key);
        check_launch("stitch_inst_reduce");
        const dim3 kgrid((unsigned)cdiv(stride, kBlock), (unsigned)n_planes);
        hipLaunchKernelGGL(keys_kernel, kgrid, dim3(kBlock), 0, st, root, acc_key, (int)per_plane, stride, keys);
        check_launch("stitch_inst_keys");
        launch_segsort_u64(ctx, keys, n_planes, stride);
        hipLaunchKernelGGL(emit_kernel, kgrid, dim3(kBlock), 0, st, keys, (int)per_plane, stride, E, labels, acc_box, acc_key, rank_of,
                           out_boxes, out_scores, out_labels, out_counts);
        check_launch("stitch_inst_emit");
    }
    {
        ProfScope p_(ctx, FAM_METRICS, 0, mask_bytes + (double)n_planes * C * T * (1 + (out_masks ? E : 0)), "stitch_inst_paste");
        const dim3 grid((unsigned)cdiv(T, 64), (unsigned)cdiv(C, 4), (unsigned)n_planes);
        hipLaunchKernelGGL(paste_kernel, grid, dim3(64, 4), 0, st, counts, masks, g, mbox, root, rank_of, E, rfi_mask, out_masks);
        check_launch("stitch_inst_paste");
    }
}

}  // namespace rfi
