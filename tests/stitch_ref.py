"""NumPy restatement of the whole-observation tiling and its inverse (include/rfi_hip.h, rfi_tiling /
rfi_stitch_patches), written from the rules, not from the kernel:

* views 1, 2, 4 select {0}, {0,1}, {0,1,2,3}: plane, plane[::-1,:], plane.T, plane.T[::-1,:];
* tile origins along an axis of length L: [0] when L <= ps, else 0, s, ..., k*s with k = ceil((L-ps)/s);
  edge "shift" replaces the last one by L-ps;
* patch order: plane, view, tile row, tile column;
* per pixel, the covering (view, tile) pairs are visited in that same order; each visit reads
  p = 1 / (1 + exp(-x)) in float32 (logits) or x; "mean" is a float32 running sum / float32 count, "max" the
  maximum; flag = combined > threshold.
"""
import numpy as np

VIEW_SETS = {1: (0,), 2: (0, 1), 4: (0, 1, 2, 3)}


def origins(L, ps, stride, edge="pad"):
    if L <= ps:
        return [0]
    k = -(-(L - ps) // stride)
    o = [i * stride for i in range(k + 1)]
    if edge == "shift":
        o[-1] = L - ps
    return o


def view_of(a, v):
    """View v of the last two axes (a NumPy view: writing through it writes `a`)."""
    if v == 0:
        return a
    if v == 1:
        return a[..., ::-1, :]
    t = np.swapaxes(a, -1, -2)
    return t if v == 2 else t[..., ::-1, :]


def patch_table(n_planes, C, T, ps, stride=None, views=1, edge="pad"):
    stride = ps if stride is None else stride
    rows = []
    for p in range(n_planes):
        for v in VIEW_SETS[views]:
            hv, wv = (T, C) if v >= 2 else (C, T)
            for r0 in origins(hv, ps, stride, edge):
                for c0 in origins(wv, ps, stride, edge):
                    rows.append((p, v, r0, c0))
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def reference_patch_table(n_planes, C, T, rot, ps):
    """One (plane, view, row0, col0) entry per patch, in the reference's order: plane-major, then
    view (:413-446), then row-major tiles of the zero-padded view (:478-560).  Written from the reference's
    Preprocessor, not from the rules above: patch_table at stride == ps, edge "pad" must equal it."""
    views = (0,) if rot < 2 else ((0, 1) if rot < 4 else (0, 1, 2, 3))
    whole = C <= ps and T <= ps          # small waterfalls are used whole, unpadded (:340-347)
    rows = []
    for plane in range(n_planes):
        for v in views:
            hv, wv = (T, C) if v >= 2 else (C, T)
            if whole:
                rows.append((plane, v, 0, 0))
                continue
            for r0 in range(0, max(hv, ps), ps):
                if r0 >= hv and r0 > 0:
                    break
                for c0 in range(0, max(wv, ps), ps):
                    if c0 >= wv and c0 > 0:
                        break
                    rows.append((plane, v, r0, c0))
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def patches_per_plane(C, T, ps, stride=None, views=1, edge="pad"):
    stride = ps if stride is None else stride
    return len(VIEW_SETS[views]) * len(origins(C, ps, stride, edge)) * len(origins(T, ps, stride, edge))


def cut(planes, table, ps):
    """The patches of `table` cut from (n_planes, C, T) `planes`, zero padded past a view's edge."""
    out = np.zeros((len(table), ps, ps), dtype=planes.dtype)
    for e, (p, v, r0, c0) in enumerate(table):
        blk = view_of(planes[p], v)[r0:r0 + ps, c0:c0 + ps]
        out[e, :blk.shape[0], :blk.shape[1]] = blk
    return out


def sigmoid32(x):
    x = np.asarray(x, dtype=np.float32)
    one = np.float32(1.0)
    return one / (one + np.exp(-x))


def stitch(values, n_planes, C, T, ps, stride=None, views=1, edge="pad", combine="mean", threshold=0.5,
           logits=True):
    """(N, ps, ps) patch values in patch_table order -> (flags bool, combined float32), each (n_planes, C, T)."""
    table = patch_table(n_planes, C, T, ps, stride, views, edge)
    values = np.asarray(values, dtype=np.float32).reshape(len(table), ps, ps)
    acc = np.zeros((n_planes, C, T), dtype=np.float32)
    cnt = np.zeros((n_planes, C, T), dtype=np.int64)
    for e, (p, v, r0, c0) in enumerate(table):           # table order == the per-pixel visiting order
        a, n = view_of(acc[p], v), view_of(cnt[p], v)
        h, w = min(ps, a.shape[0] - r0), min(ps, a.shape[1] - c0)
        val = values[e, :h, :w]
        val = sigmoid32(val) if logits else val
        dst, dn = a[r0:r0 + h, c0:c0 + w], n[r0:r0 + h, c0:c0 + w]
        if combine == "mean":
            dst += val
        else:
            dst[...] = np.where((dn == 0) | (val > dst), val, dst)
        dn += 1
    assert cnt.min() >= 1, "a pixel no tile covers"
    out = acc / cnt.astype(np.float32) if combine == "mean" else acc
    return out > np.float32(threshold), out.astype(np.float32)
