// Connected-component labelling of binary planes, with its three consumers: the component table (area, bounding box),
// despeckling and the detector's instance targets (include/rfi_hip.h, "connected components").  All integer work: every
// result is exact and independent of launch geometry and of the order in which atomics arrive.
//
// Labelling is label equivalence with union-find on `parent` [n][H W] int32, -1 for background: a foreground pixel starts
// as its own parent (its linear index y W + x inside its plane), a union hangs the larger root under the smaller one with
// atomicMin, so parent[p] <= p always, parents only ever decrease and the root of a set is its smallest pixel -- the pixel
// the numbering rule ranks components by.  Six launches, each after the one before has ended:
//   1 tile      one workgroup per kTileH x kTileW tile labels it in LDS (LDS atomics) and writes parent = the tile-local root
//   2 merge     one thread per pixel on a tile's first row / first column unites it with its neighbours across the border
//               (global atomicMin; absent when the plane is one tile)
//   3 flatten   root[p] = find(p) into `labels` (parent is only read), roots counted per run of kScanBlock pixels
//   4 scan      exclusive scan of those counts per plane; the total is n_components
//   5 rank      every root r gets parent[r] = its 1-based rank among the plane's roots in raster order
//   6 renumber  labels[p] = parent[root[p]], 0 for background
// Whether a union succeeded is decided from the value atomicMin RETURNED, never from a load: on gfx950 every XCD has an L2 of
// its own, and a load may see an older parent while another XCD is merging.  That is harmless to find() -- an older parent
// is still an ancestor, the walk merely starts higher up -- and find()'s loads in the merge launch are agent-scope atomic
// loads anyway.  No workgroup ever waits for another one's progress.
#include <algorithm>
#include <climits>

#include "kernels.hpp"
#include "launch_common.hpp"
#include "union_find.hpp"

namespace rfi {
namespace {

constexpr int kBlock = 256;
constexpr int kTileH = 32, kTileW = 64, kTilePx = kTileH * kTileW;      // 8 KB of LDS labels
constexpr int kPerThread = 8;
constexpr int kScanBlock = kBlock * kPerThread;                         // pixels of one root count
static_assert(kTilePx == kBlock * kPerThread, "a thread labels kPerThread pixels of its tile");

__device__ __forceinline__ bool nonzero(uint8_t v) { return v != 0; }
__device__ __forceinline__ bool nonzero(float v) { return v != 0.0f; }      // (NaN is non-zero, as in NumPy)

// (union-find: PlainLoad / AgentLoad, find_root, unite -- union_find.hpp; find_root takes at most H W steps here, unite at
// most 2 H W passes)

// ---- 1: label one tile in LDS.  grid (tiles of a plane, row-major; planes)
template <typename T>
__global__ void __launch_bounds__(kBlock) ccl_tile_kernel(const T* __restrict__ mask, int H, int W, int tiles_x, int conn8,
                                                          int* __restrict__ parent) {
    __shared__ int L[kTilePx];
    const int64_t plane = (int64_t)blockIdx.y * H * W;
    const int x0 = (int)(blockIdx.x % tiles_x) * kTileW, y0 = (int)(blockIdx.x / tiles_x) * kTileH, tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int i = tid + k * kBlock, x = x0 + i % kTileW, y = y0 + i / kTileW;
        L[i] = (x < W && y < H && nonzero(mask[plane + (int64_t)y * W + x])) ? i : -1;
    }
    __syncthreads();
    const PlainLoad ld;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {          // (a word's sign never changes: L[j] >= 0 == "j is foreground")
        const int i = tid + k * kBlock, lx = i % kTileW, ly = i / kTileW;
        if (L[i] < 0) continue;
        if (lx > 0 && L[i - 1] >= 0) unite(L, i, i - 1, ld);
        if (ly > 0) {
            if (L[i - kTileW] >= 0) unite(L, i, i - kTileW, ld);
            if (conn8 && lx > 0 && L[i - kTileW - 1] >= 0) unite(L, i, i - kTileW - 1, ld);
            if (conn8 && lx < kTileW - 1 && L[i - kTileW + 1] >= 0) unite(L, i, i - kTileW + 1, ld);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int i = tid + k * kBlock, x = x0 + i % kTileW, y = y0 + i / kTileW;
        if (x >= W || y >= H) continue;
        int r = -1;
        if (L[i] >= 0) {
            const int lr = find_root(L, i, ld);       // the tile-local order is the plane's order restricted to the tile
            r = (y0 + lr / kTileW) * W + x0 + lr % kTileW;
        }
        parent[plane + (int64_t)y * W + x] = r;
    }
}

// ---- 2: unions across tile borders.  Items of a plane: (tiles x - 1) H pixels on first columns, then (tiles y - 1) W on
// first rows.  A first-column pixel joins (y, x-1) and, 8-connected, (y-1, x-1) and (y+1, x-1); a first-row pixel joins
// (y-1, x) and (y-1, x-1), (y-1, x+1): every neighbouring pair that lies in two tiles is one of these.  grid (blocks, planes)
__global__ void __launch_bounds__(kBlock) ccl_merge_kernel(int H, int W, int conn8, int n_col, int n_items, int* __restrict__ parent) {
    const int it = blockIdx.x * kBlock + threadIdx.x;
    if (it >= n_items) return;
    int* L = parent + (int64_t)blockIdx.y * H * W;
    const AgentLoad ld;
    auto join = [&](int p, int y, int x) {
        if (y < 0 || y >= H || x < 0 || x >= W) return;
        const int q = y * W + x;
        if (ld(L + q) >= 0) unite(L, p, q, ld);
    };
    if (it < n_col) {
        const int x = (it / H + 1) * kTileW, y = it % H, p = y * W + x;
        if (ld(L + p) < 0) return;
        join(p, y, x - 1);
        if (conn8) {
            join(p, y - 1, x - 1);
            join(p, y + 1, x - 1);
        }
    } else {
        const int j = it - n_col, y = (j / W + 1) * kTileH, x = j % W, p = y * W + x;
        if (ld(L + p) < 0) return;
        join(p, y - 1, x);
        if (conn8) {
            join(p, y - 1, x - 1);
            join(p, y - 1, x + 1);
        }
    }
}

// exclusive scan of one value per thread over the workgroup (kBlock threads, all of them call); total: the sum
__device__ __forceinline__ int block_scan_exclusive(int v, int* wave_sums, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < kBlock / 64; ++i) {
        off += i < wave ? wave_sums[i] : 0;
        total += wave_sums[i];
    }
    __syncthreads();                                  // (wave_sums may be written again right away)
    return off + inc - v;
}

// ---- 3: root[p] = find(p) (the merging launch has ended: plain loads), roots per run of kScanBlock pixels.
// grid (runs, planes); thread t of run b owns pixels b kScanBlock + t kPerThread + (0 .. kPerThread - 1)
__global__ void __launch_bounds__(kBlock) ccl_flatten_kernel(const int* __restrict__ parent, int HW, int runs, int* __restrict__ root,
                                                             int* __restrict__ run_roots) {
    __shared__ int wave_sums[kBlock / 64];
    const int64_t plane = (int64_t)blockIdx.y * HW;
    const int p0 = blockIdx.x * kScanBlock + threadIdx.x * kPerThread;
    const PlainLoad ld;
    int mine = 0;
    for (int k = 0; k < kPerThread; ++k) {
        const int p = p0 + k;
        if (p >= HW) break;
        int r = parent[plane + p];
        if (r >= 0) {
            r = find_root(parent + plane, p, ld);
            mine += r == p;
        }
        root[plane + p] = r;
    }
    int total;
    block_scan_exclusive(mine, wave_sums, total);
    if (threadIdx.x == 0) run_roots[(int64_t)blockIdx.y * runs + blockIdx.x] = total;
}

// ---- 4: out[row][i] = sum of in[row][0 .. i - 1], totals[row] = the row's sum (null: not wanted).  in may equal out.
// grid (rows); the loop runs cdiv(len, kBlock) times
__global__ void __launch_bounds__(kBlock) scan_rows_kernel(const int* in, int len, int* out, int* __restrict__ totals) {
    __shared__ int wave_sums[kBlock / 64];
    const int64_t row = (int64_t)blockIdx.x * len;
    int carry = 0;
    for (int i0 = 0; i0 < len; i0 += kBlock) {
        const int i = i0 + threadIdx.x;
        const int v = i < len ? in[row + i] : 0;
        int total;
        const int ex = block_scan_exclusive(v, wave_sums, total);
        if (i < len) out[row + i] = carry + ex;
        carry += total;
    }
    if (totals && threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// ---- 5: parent[r] = 1 + the number of roots before r in raster order, for every root r.  grid as for 3
__global__ void __launch_bounds__(kBlock) ccl_rank_kernel(const int* __restrict__ root, int HW, int runs, const int* __restrict__ run_offset,
                                                          int* __restrict__ parent) {
    __shared__ int wave_sums[kBlock / 64];
    const int64_t plane = (int64_t)blockIdx.y * HW;
    const int p0 = blockIdx.x * kScanBlock + threadIdx.x * kPerThread;
    int mine = 0;
    for (int k = 0; k < kPerThread; ++k)
        if (p0 + k < HW) mine += root[plane + p0 + k] == p0 + k;
    int total;
    int rank = run_offset[(int64_t)blockIdx.y * runs + blockIdx.x] + block_scan_exclusive(mine, wave_sums, total);
    for (int k = 0; k < kPerThread; ++k)
        if (p0 + k < HW && root[plane + p0 + k] == p0 + k) parent[plane + p0 + k] = ++rank;
}

// ---- 6: labels = rank of the root (in place over root).  One thread per pixel of the stack
__global__ void __launch_bounds__(kBlock) ccl_renumber_kernel(const int* __restrict__ rank_of, int HW, int64_t total, int* __restrict__ labels) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int r = labels[i];
    labels[i] = r >= 0 ? rank_of[i / HW * HW + r] : 0;
}

// ---- table: area and box of every component, slot comp_base[plane] + label - 1.  Reduced on the way to global memory
// (Guideline 12; RFI masks are long lines and most of a plane's foreground is one component, so the adds of a plane pile
// onto one slot): a thread walks kPerThread consecutive pixels and closes a run when the label or the row changes; the runs
// a wave closes at the same step are combined per label across the wave with shuffles; the wave's leader adds them to
// the workgroup's table in LDS -- kTableSlots (label, area, box) entries, open addressing, at most kTableProbes probes, a
// label that finds no entry goes straight to global memory; a workgroup walks kTableChunks runs of kScanBlock pixels and
// then issues five integer atomics per entry it filled.  Integer adds, minima and maxima: exact in any order.
constexpr int kTableSlots = 64, kTableProbes = 8, kTableChunks = 8;

__global__ void __launch_bounds__(kBlock) table_init_kernel(int64_t total, int* __restrict__ area, int* __restrict__ box) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    area[i] = 0;
    reinterpret_cast<int4*>(box)[i] = make_int4(INT_MAX, INT_MAX, -1, -1);
}

struct Run {
    int label, count, xmin, xmax, y;
};
struct BlockTable {                                   // (in LDS; label 0: the entry is free)
    int label[kTableSlots], count[kTableSlots], x0[kTableSlots], y0[kTableSlots], x1[kTableSlots], y1[kTableSlots];
};
__device__ __forceinline__ void global_add(int64_t s, int c, int x0, int y0, int x1, int y1, int* __restrict__ area, int* __restrict__ box) {
    atomicAdd(area + s, c);
    atomicMin(box + 4 * s, x0);
    atomicMin(box + 4 * s + 1, y0);
    atomicMax(box + 4 * s + 2, x1);
    atomicMax(box + 4 * s + 3, y1);
}
__device__ __forceinline__ void wave_add_runs(bool has, const Run& r, int slot0, BlockTable& t, int* __restrict__ area, int* __restrict__ box) {
    const int lane = threadIdx.x & 63;
    unsigned long long pending = __ballot(has);
    while (pending) {                                 // every pass clears the leader's bit at least: at most 64 passes
        const int leader = __ffsll((long long)pending) - 1;
        const int label = __shfl(r.label, leader, 64);
        const bool mine = has && r.label == label;
        const unsigned long long group = __ballot(mine);
        int c = mine ? r.count : 0, x0 = mine ? r.xmin : INT_MAX, x1 = mine ? r.xmax : -1, y0 = mine ? r.y : INT_MAX, y1 = mine ? r.y : -1;
        if (group & (group - 1)) {                    // more than one lane holds this label
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                c += __shfl_xor(c, o, 64);
                x0 = min(x0, __shfl_xor(x0, o, 64));
                x1 = max(x1, __shfl_xor(x1, o, 64));
                y0 = min(y0, __shfl_xor(y0, o, 64));
                y1 = max(y1, __shfl_xor(y1, o, 64));
            }
        }
        if (lane == leader) {
            int e = (int)(((unsigned)label * 2654435761u) >> 26) & (kTableSlots - 1), probe = 0;
            for (; probe < kTableProbes; ++probe, e = (e + 1) & (kTableSlots - 1)) {
                const int old = atomicCAS(&t.label[e], 0, label);      // the entry is this label's iff it was free or already its own
                if (old == 0 || old == label) break;
            }
            if (probe < kTableProbes) {
                atomicAdd(&t.count[e], c);
                atomicMin(&t.x0[e], x0);
                atomicMin(&t.y0[e], y0);
                atomicMax(&t.x1[e], x1);
                atomicMax(&t.y1[e], y1);
            } else {
                global_add((int64_t)slot0 + label - 1, c, x0, y0, x1, y1, area, box);
            }
        }
        pending &= ~group;
    }
}
// grid (groups of kTableChunks runs of kScanBlock pixels, planes)
__global__ void __launch_bounds__(kBlock) table_kernel(const int* __restrict__ labels, int HW, int W, const int* __restrict__ comp_base,
                                                       int* __restrict__ area, int* __restrict__ box) {
    __shared__ BlockTable t;
    const int64_t plane = (int64_t)blockIdx.y * HW;
    const int slot0 = comp_base[blockIdx.y];
    for (int e = threadIdx.x; e < kTableSlots; e += kBlock) {
        t.label[e] = t.count[e] = 0;
        t.x0[e] = t.y0[e] = INT_MAX;
        t.x1[e] = t.y1[e] = -1;
    }
    __syncthreads();
    for (int chunk = 0; chunk < kTableChunks; ++chunk) {
        const int p0 = ((int)blockIdx.x * kTableChunks + chunk) * kScanBlock + threadIdx.x * kPerThread;      // (< 2^30 + 2^15)
        Run open{0, 0, 0, 0, 0};
        for (int k = 0; k <= kPerThread; ++k) {       // (step kPerThread closes what is still open)
            const int p = p0 + k;
            const int l = (k < kPerThread && p < HW) ? labels[plane + p] : 0;
            const int y = p / W, x = p - y * W;
            const bool extend = l > 0 && open.count > 0 && l == open.label && y == open.y;
            const bool close = open.count > 0 && !extend;
            wave_add_runs(close, open, slot0, t, area, box);
            if (extend) {
                ++open.count;
                open.xmax = x;
            } else {
                open = Run{l, l > 0 ? 1 : 0, x, x, y};
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kTableSlots; e += kBlock)
        if (t.label[e]) global_add((int64_t)slot0 + t.label[e] - 1, t.count[e], t.x0[e], t.y0[e], t.x1[e], t.y1[e], area, box);
}

// ---- despeckle: keep the foreground whose component has at least min_area pixels
__global__ void __launch_bounds__(kBlock) keep_kernel(const int* __restrict__ labels, int HW, int64_t total, const int* __restrict__ comp_base,
                                                      const int* __restrict__ area, int min_area, uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int l = labels[i];
    out[i] = l > 0 && area[(int64_t)comp_base[i / HW] + l - 1] >= min_area;
}

// ---- instances: one workgroup per plane.  Keys (~area << 32 | label) are distinct, ascending = area descending, ties by
// label.  More survivors than G: the G-th smallest key is found by a radix select over the 64-bit key (eight passes of 8
// bits, most significant first, over the plane's table); then the keys up to it are gathered and ordered by rank.
__device__ __forceinline__ unsigned long long instance_key(int area, int label) {
    return (unsigned long long)(0xFFFFFFFFu - (unsigned)area) << 32 | (unsigned)label;
}
__global__ void __launch_bounds__(kBlock) instances_select_kernel(const int* __restrict__ n_components, const int* __restrict__ comp_base,
                                                                  const int* __restrict__ area, const int* __restrict__ box, int min_area,
                                                                  int min_side, int G, float* __restrict__ boxes, int* __restrict__ cls,
                                                                  int* __restrict__ count, int* __restrict__ n_survivors,
                                                                  int* __restrict__ component) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long keys[256], sorted[256], prefix_s;
    __shared__ int n_s, rank_s;
    const int plane = blockIdx.x, tid = threadIdx.x, K = n_components[plane];
    const int64_t s0 = comp_base[plane];
    const int4* box4 = reinterpret_cast<const int4*>(box);
    auto survives = [&](int c) {
        const int4 b = box4[s0 + c];
        return area[s0 + c] >= min_area && b.z - b.x + 1 >= min_side && b.w - b.y + 1 >= min_side;
    };
    if (tid == 0) n_s = 0;
    __syncthreads();
    int mine = 0;
    for (int c = tid; c < K; c += kBlock) mine += survives(c);
    if (mine) atomicAdd(&n_s, mine);
    __syncthreads();
    const int S = n_s, cnt = min(S, G);
    unsigned long long limit = ~0ull;                 // the largest key that is kept
    if (S > G) {
        if (tid == 0) {
            prefix_s = 0;
            rank_s = G - 1;                           // 0-based rank of the key looked for among the keys matching prefix_s
        }
        for (int shift = 56; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            const unsigned long long prefix = prefix_s;
            for (int c = tid; c < K; c += kBlock) {
                if (!survives(c)) continue;
                const unsigned long long key = instance_key(area[s0 + c], c + 1);
                if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                int r = rank_s, d = 0;
                while (d < 255 && (unsigned)r >= hist[d]) r -= (int)hist[d++];      // (at most 255 steps)
                rank_s = r;
                prefix_s = prefix | (unsigned long long)d << shift;
            }
            __syncthreads();
        }
        limit = prefix_s;
    }
    __syncthreads();
    if (tid == 0) n_s = 0;
    __syncthreads();
    for (int c = tid; c < K; c += kBlock) {
        if (!survives(c)) continue;
        const unsigned long long key = instance_key(area[s0 + c], c + 1);
        if (key <= limit) {
            const int slot = atomicAdd(&n_s, 1);      // (exactly cnt keys pass: keys are distinct)
            if (slot < 256) keys[slot] = key;
        }
    }
    __syncthreads();
    if (tid < cnt) {
        int r = 0;
        for (int j = 0; j < cnt; ++j) r += keys[j] < keys[tid];
        sorted[r] = keys[tid];
    }
    __syncthreads();
    for (int j = tid; j < G; j += kBlock) {
        const int64_t o = (int64_t)plane * G + j;
        float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
        int label = 0;
        if (j < cnt) {
            label = (int)(sorted[j] & 0xFFFFFFFFu);
            const int4 b = box4[s0 + label - 1];
            bx = make_float4((float)b.x, (float)b.y, (float)(b.z + 1), (float)(b.w + 1));
        }
        reinterpret_cast<float4*>(boxes)[o] = bx;
        cls[o] = j < cnt ? 1 : 0;
        component[o] = label;
    }
    if (tid == 0) {
        count[plane] = cnt;
        n_survivors[plane] = S;
    }
}

// masks[base[plane] + j][p] = (labels[plane][p] == component[plane][j]), j < count[plane].  grid (pixel blocks, planes)
__global__ void __launch_bounds__(kBlock) instance_masks_kernel(const int* __restrict__ labels, int HW, const int* __restrict__ component,
                                                                const int* __restrict__ count, const int* __restrict__ base, int G,
                                                                uint8_t* __restrict__ masks) {
    __shared__ int comp[256];
    const int plane = blockIdx.y, cnt = count[plane];
    if (cnt == 0) return;
    for (int j = threadIdx.x; j < cnt; j += kBlock) comp[j] = component[(int64_t)plane * G + j];
    __syncthreads();
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= HW) return;
    const int l = labels[(int64_t)plane * HW + p];
    uint8_t* m = masks + (int64_t)base[plane] * HW + p;
    for (int j = 0; j < cnt; ++j) m[(int64_t)j * HW] = l == comp[j];
}

int runs_of(int h, int w) { return (int)cdiv((int64_t)h * w, kScanBlock); }

void check_planes(const char* who, int n, int h, int w) {
    RFI_REQUIRE(n >= 1 && h >= 1 && w >= 1 && (int64_t)h * w <= (int64_t(1) << 30), std::string(who) + ": needs n >= 1, H, W >= 1 and H W <= 2^30");
    RFI_REQUIRE(n <= 65535, std::string(who) + ": at most 65535 planes in one call");
}

}  // namespace

void components_limits(int* tile_h, int* tile_w, int* scan_block) {
    *tile_h = kTileH;
    *tile_w = kTileW;
    *scan_block = kScanBlock;
}

size_t components_ws_bytes(int n, int h, int w) {
    return al((size_t)n * h * w * sizeof(int)) + al((size_t)n * runs_of(h, w) * sizeof(int));
}

void launch_label_components(rfi_ctx* ctx, const void* masks, int dtype, int n, int h, int w, int connectivity, void* ws, int* labels,
                             int* n_components) {
    check_planes("label_components", n, h, w);
    RFI_REQUIRE(connectivity == 4 || connectivity == 8, "label_components: connectivity must be 4 or 8");
    RFI_REQUIRE(dtype == RFI_U8 || dtype == RFI_FLOAT32, "label_components: masks must be u8 or f32");
    const int HW = h * w, runs = runs_of(h, w), conn8 = connectivity == 8;
    const int64_t total = (int64_t)n * HW;
    Carve cv{static_cast<char*>(ws)};
    int* parent = cv.take<int>((size_t)total);
    int* run_roots = cv.take<int>((size_t)n * runs);
    ProfScope ps(ctx, FAM_METRICS, 0, (double)total * 30.0);
    const int tx = (int)cdiv(w, kTileW), ty = (int)cdiv(h, kTileH);
    const dim3 tiles(grid_of((int64_t)tx * ty, "ccl_tile"), n);
    if (dtype == RFI_U8)
        hipLaunchKernelGGL(ccl_tile_kernel<uint8_t>, tiles, dim3(kBlock), 0, ctx->stream, static_cast<const uint8_t*>(masks), h, w, tx, conn8,
                           parent);
    else
        hipLaunchKernelGGL(ccl_tile_kernel<float>, tiles, dim3(kBlock), 0, ctx->stream, static_cast<const float*>(masks), h, w, tx, conn8, parent);
    check_launch("ccl_tile");
    const int64_t n_col = (int64_t)(tx - 1) * h, n_items = n_col + (int64_t)(ty - 1) * w;       // (< 2 H W <= 2^31)
    if (n_items > 0) {
        hipLaunchKernelGGL(ccl_merge_kernel, dim3(grid_of(cdiv(n_items, kBlock), "ccl_merge"), n), dim3(kBlock), 0, ctx->stream, h, w, conn8,
                           (int)n_col, (int)n_items, parent);
        check_launch("ccl_merge");
    }
    const dim3 by_run(runs, n);
    hipLaunchKernelGGL(ccl_flatten_kernel, by_run, dim3(kBlock), 0, ctx->stream, parent, HW, runs, labels, run_roots);
    check_launch("ccl_flatten");
    hipLaunchKernelGGL(scan_rows_kernel, dim3(n), dim3(kBlock), 0, ctx->stream, run_roots, runs, run_roots, n_components);
    check_launch("ccl_scan");
    hipLaunchKernelGGL(ccl_rank_kernel, by_run, dim3(kBlock), 0, ctx->stream, labels, HW, runs, run_roots, parent);
    check_launch("ccl_rank");
    hipLaunchKernelGGL(ccl_renumber_kernel, dim3(grid_of(cdiv(total, kBlock), "ccl_renumber")), dim3(kBlock), 0, ctx->stream, parent, HW,
                       total, labels);
    check_launch("ccl_renumber");
}

void launch_component_table(rfi_ctx* ctx, const int* labels, int n, int h, int w, const int* comp_base, int64_t total, int* area, int* box) {
    check_planes("component_table", n, h, w);
    RFI_REQUIRE(total >= 0 && total <= 0x7fffffff, "component_table: 0 .. 2^31 - 1 components in all");
    RFI_REQUIRE(reinterpret_cast<uintptr_t>(box) % 16 == 0, "component_table: box must be 16-byte aligned");
    if (total == 0) return;
    ProfScope ps(ctx, FAM_METRICS, 0, (double)n * h * w * 4.0);
    hipLaunchKernelGGL(table_init_kernel, dim3(grid_of(cdiv(total, kBlock), "table_init")), dim3(kBlock), 0, ctx->stream, total, area, box);
    check_launch("table_init");
    hipLaunchKernelGGL(table_kernel, dim3((unsigned)cdiv(runs_of(h, w), kTableChunks), n), dim3(kBlock), 0, ctx->stream, labels, h * w, w,
                       comp_base, area, box);
    check_launch("component_table");
}

void launch_components_keep(rfi_ctx* ctx, const int* labels, int n, int h, int w, const int* comp_base, const int* area, int min_area,
                            uint8_t* out) {
    check_planes("components_keep", n, h, w);
    RFI_REQUIRE(min_area >= 1, "components_keep: min_area must be >= 1");
    const int64_t total = (int64_t)n * h * w;
    ProfScope ps(ctx, FAM_METRICS, 0, (double)total * 5.0);
    hipLaunchKernelGGL(keep_kernel, dim3(grid_of(cdiv(total, kBlock), "components_keep")), dim3(kBlock), 0, ctx->stream, labels, h * w, total,
                       comp_base, area, min_area, out);
    check_launch("components_keep");
}

void launch_instances_select(rfi_ctx* ctx, const int* n_components, const int* comp_base, const int* area, const int* box, int n,
                             int min_area, int min_side, int max_instances, float* boxes, int* cls, int* count, int* n_survivors, int* base,
                             int* component) {
    RFI_REQUIRE(n >= 1 && n <= 0x7fffffff / 256, "instances_select: bad plane count");
    RFI_REQUIRE(min_area >= 1 && min_side >= 1, "instances_select: min_area and min_side must be >= 1");
    RFI_REQUIRE(max_instances >= 1 && max_instances <= 256, "instances_select: max_instances must be in 1 .. 256");
    RFI_REQUIRE(reinterpret_cast<uintptr_t>(box) % 16 == 0 && reinterpret_cast<uintptr_t>(boxes) % 16 == 0,
                "instances_select: box tensors must be 16-byte aligned");
    ProfScope ps(ctx, FAM_METRICS);
    hipLaunchKernelGGL(instances_select_kernel, dim3(n), dim3(kBlock), 0, ctx->stream, n_components, comp_base, area, box, min_area, min_side,
                       max_instances, boxes, cls, count, n_survivors, component);
    check_launch("instances_select");
    hipLaunchKernelGGL(scan_rows_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, count, n, base, static_cast<int*>(nullptr));
    check_launch("instances_base");
}

void launch_instance_masks(rfi_ctx* ctx, const int* labels, int n, int h, int w, const int* component, const int* count, const int* base,
                           int max_instances, uint8_t* masks) {
    check_planes("instance_masks", n, h, w);
    RFI_REQUIRE(max_instances >= 1 && max_instances <= 256, "instance_masks: max_instances must be in 1 .. 256");
    ProfScope ps(ctx, FAM_METRICS);
    hipLaunchKernelGGL(instance_masks_kernel, dim3(grid_of(cdiv((int64_t)h * w, kBlock), "instance_masks"), n), dim3(kBlock), 0, ctx->stream,
                       labels, h * w, component, count, base, max_instances, masks);
    check_launch("instance_masks");
}

}  // namespace rfi
