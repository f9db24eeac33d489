// The rfi_tiling of a C x T plane in code, once (stitch.hip, instance_stitch.hip, api.cpp): the grid, the patch order and the
// walk over the tiles that cover a pixel.  The rule's text is the comment above rfi_tiling in include/rfi_hip.h; a change
// to it is made there and here, nowhere else.  The float32 mean of the stitch is a running sum in the walk's visiting
// order and the instance stitch indexes tiles by their position in the table, so both orders are part of the contract.
#pragma once
#include "common.hpp"

namespace rfi {

// tiles along an axis of length L, and the origin of tile i of those n
__host__ __device__ inline int axis_tiles(int L, int ps, int s) { return L <= ps ? 1 : (L - ps + s - 1) / s + 1; }
__host__ __device__ inline int tile_origin(int i, int n, int L, int ps, int s, int shift) {
    return (shift && i == n - 1 && L > ps) ? L - ps : i * s;
}

struct TileGrid {
    int C, T, ps, s, shift, views;
    int nC, nT;                    // tiles along C and along T
    int64_t ppp;                   // patches per plane
};

inline TileGrid make_tile_grid(int C, int T, const rfi_tiling& tl) {
    TileGrid g{C, T, tl.ps, tl.stride, tl.edge == RFI_EDGE_SHIFT ? 1 : 0, tl.views, axis_tiles(C, tl.ps, tl.stride),
               axis_tiles(T, tl.ps, tl.stride), 0};
    g.ppp = (int64_t)g.views * g.nC * g.nT;
    return g;
}

// view v of the plane (0 plane, 1 plane[::-1,:], 2 plane.T, 3 plane.T[::-1,:]): its size Hv x Wv, its tile rows and columns
// nr x nc, and plane pixel (c, t) in its coordinates (y, x)
struct ViewPixel {
    int Hv, Wv, nr, nc, y, x;
};
__host__ __device__ inline ViewPixel view_pixel(const TileGrid& g, int v, int c, int t) {
    const bool tr = v >= 2;
    const int Hv = tr ? g.T : g.C, Wv = tr ? g.C : g.T;
    const int nr = tr ? g.nT : g.nC, nc = tr ? g.nC : g.nT;
    const int yy = tr ? t : c, x = tr ? c : t;
    return ViewPixel{Hv, Wv, nr, nc, (v & 1) ? Hv - 1 - yy : yy, x};
}

// f(tile in plane, offset in tile) for every tile that covers plane pixel (c, t): views ascending, then tile rows, then
// tile columns.  Index is the integer type both are formed in: int only where the caller has bounded ppp and ps
template <class Index, class F>
__device__ __forceinline__ void for_each_covering_tile(const TileGrid& g, int c, int t, F&& f) {
    for (int v = 0; v < g.views; ++v) {
        const ViewPixel p = view_pixel(g, v, c, t);
        const Index vbase = (Index)v * p.nr * p.nc;            // (every view holds nC nT tiles)
        const int i0 = p.y >= g.ps ? (p.y - g.ps) / g.s + 1 : 0;
        const int j0 = p.x >= g.ps ? (p.x - g.ps) / g.s + 1 : 0;
        for (int i = i0; i < p.nr; ++i) {
            const int r0 = tile_origin(i, p.nr, p.Hv, g.ps, g.s, g.shift);
            if (r0 > p.y) break;
            if (p.y >= r0 + g.ps) continue;
            for (int j = j0; j < p.nc; ++j) {
                const int c0 = tile_origin(j, p.nc, p.Wv, g.ps, g.s, g.shift);
                if (c0 > p.x) break;
                if (p.x >= c0 + g.ps) continue;
                f(vbase + (Index)i * p.nc + j, (Index)(p.y - r0) * g.ps + (p.x - c0));
            }
        }
    }
}

// the table of n_units planes in patch order: unit, view, tile row, tile column
inline std::vector<rfi_patch_src> tile_table(const TileGrid& g, int n_units) {
    std::vector<rfi_patch_src> table;
    table.reserve((size_t)n_units * g.ppp);
    for (int u = 0; u < n_units; ++u)
        for (int v = 0; v < g.views; ++v) {
            const ViewPixel p = view_pixel(g, v, 0, 0);
            for (int i = 0; i < p.nr; ++i)
                for (int j = 0; j < p.nc; ++j)
                    table.push_back(rfi_patch_src{u, v, tile_origin(i, p.nr, p.Hv, g.ps, g.s, g.shift),
                                                  tile_origin(j, p.nc, p.Wv, g.ps, g.s, g.shift)});
        }
    return table;
}

}  // namespace rfi
