"""The rules of the instance stitch (include/rfi_hip.h, "instance stitch") restated in NumPy: plain loops over tiles and
pairs of members on whole-plane masks, float32 where the header says float32.  Shares no code with the kernels."""
import numpy as np

import stitch_ref


def tile_table(C, T, ps, s, views, edge):
    """(view, row0, col0) of the tiles of one plane in rfi_tiling order (stitch_ref holds the restatement)."""
    return [(int(v), int(r0), int(c0)) for _, v, r0, c0 in stitch_ref.patch_table(1, C, T, ps, s, views, edge)]


def view_of(plane, v):
    """View v of a (C, T) plane: plane, plane[::-1, :], plane.T, plane.T[::-1, :]."""
    return (plane, plane[::-1, :], plane.T, plane.T[::-1, :])[v]


def to_plane(tile, v, r0, c0, C, T):
    """The non-padding pixels of a (ps, ps) tile of view v at (r0, c0) as a (C, T) bool plane."""
    Hv, Wv = (T, C) if v >= 2 else (C, T)
    ps = tile.shape[0]
    h, w = min(ps, Hv - r0), min(ps, Wv - c0)
    img = np.zeros((Hv, Wv), bool)
    img[r0:r0 + h, c0:c0 + w] = tile[:h, :w] != 0
    if v & 1:
        img = img[::-1, :]
    return np.ascontiguousarray(img.T if v >= 2 else img)


def map_box(box, v, r0, c0, C, T):
    f = np.float32
    x1, y1, x2, y2 = (f(b) for b in box)
    x1, x2, y1, y2 = f(x1 + f(c0)), f(x2 + f(c0)), f(y1 + f(r0)), f(y2 + f(r0))
    if v & 1:
        L = f(T if v >= 2 else C)
        y1, y2 = f(L - y1), f(L - y2)
    if v >= 2:
        x1, y1, x2, y2 = y1, x1, y2, x2
    if x1 > x2:
        x1, x2 = x2, x1
    if y1 > y2:
        y1, y2 = y2, y1
    clip = lambda a, hi: np.minimum(np.maximum(a, f(0)), f(hi))  # noqa: E731
    return np.array([clip(x1, T), clip(y1, C), clip(x2, T), clip(y2, C)], np.float32)


def neighbours(mask, connectivity):
    """Pixels at Chebyshev (8) or Manhattan (4) distance exactly 1 from a pixel of `mask`, inside the plane."""
    out = np.zeros_like(mask)
    for dc in (-1, 0, 1):
        for dt in (-1, 0, 1):
            if (dc, dt) == (0, 0) or (connectivity == 4 and dc and dt):
                continue
            sh = np.zeros_like(mask)
            src = mask[max(0, -dc):mask.shape[0] - max(0, dc), max(0, -dt):mask.shape[1] - max(0, dt)]
            sh[max(0, dc):max(0, dc) + src.shape[0], max(0, dt):max(0, dt) + src.shape[1]] = src
            out |= sh
    return out


def stitch(boxes, scores, labels, counts, masks, C, T, ps, stride=None, views=1, edge="pad", max_events=64, min_area=1,
           min_score=0.0, class_aware=True, connectivity=8, stats=None):
    """-> dict boxes (P, E, 4), scores, labels, counts, rfi_mask (P, C, T), masks (P, E, C, T).  `stats` (a dict) collects what
    happened: links by branch, drops by reason, per event the tiles of its members and whether every pair was linked directly."""
    s = ps if stride is None else stride
    table = tile_table(C, T, ps, s, views, edge)
    ppp, (N, D) = len(table), scores.shape
    assert N % ppp == 0
    P, E = N // ppp, max_events
    st = {"shared": 0, "adjacent": 0, "drop_score": 0, "drop_area": 0, "padding_only": 0, "events": []}
    out = {"boxes": np.zeros((P, E, 4), np.float32), "scores": np.zeros((P, E), np.float32), "labels": np.zeros((P, E), np.int32),
           "counts": np.zeros((P,), np.int32), "rfi_mask": np.zeros((P, C, T), np.uint8), "masks": np.zeros((P, E, C, T), np.uint8)}
    rects = [to_plane(np.ones((ps, ps), np.uint8), v, r0, c0, C, T) for v, r0, c0 in table]
    meet = np.array([[bool((a & b).any()) for b in rects] for a in rects])
    for p in range(P):
        mem = []                                   # (index, tile, plane mask, box, score, label)
        for ti in range(ppp):
            i = p * ppp + ti
            v, r0, c0 = table[ti]
            for j in range(min(max(int(counts[i]), 0), D)):
                if not scores[i, j] >= np.float32(min_score):
                    st["drop_score"] += 1
                    continue
                m = to_plane(masks[i, j], v, r0, c0, C, T)
                if int(m.sum()) < min_area:
                    st["drop_area"] += 1
                    st["padding_only"] += int(masks[i, j].any() and not m.any())
                    continue
                mem.append((i * D + j, ti, m, map_box(boxes[i, j], v, r0, c0, C, T), np.float32(scores[i, j]), int(labels[i, j])))
        parent = list(range(len(mem)))

        def find(a):
            while parent[a] != a:
                a = parent[a]
            return a
        direct = set()
        for a in range(len(mem)):
            for b in range(a + 1, len(mem)):
                A, B = mem[a], mem[b]
                if A[1] == B[1] or (class_aware and A[5] != B[5]):
                    continue
                if meet[A[1], B[1]]:
                    hit = bool((A[2] & B[2]).any())
                    st["shared"] += hit
                else:
                    hit = bool((neighbours(A[2], connectivity) & B[2]).any())
                    st["adjacent"] += hit
                if hit:
                    direct.add((a, b))
                    ra, rb = find(a), find(b)
                    parent[max(ra, rb)] = min(ra, rb)
        groups = {}
        for a in range(len(mem)):
            groups.setdefault(find(a), []).append(a)
        events = []
        for g in groups.values():
            best = g[0]
            for a in g[1:]:
                if mem[a][4] > mem[best][4]:
                    best = a
            bx = np.stack([mem[a][3] for a in g])
            box = np.array([bx[:, 0].min(), bx[:, 1].min(), bx[:, 2].max(), bx[:, 3].max()], np.float32)
            mask = np.zeros((C, T), bool)
            for a in g:
                mask |= mem[a][2]
            events.append((mem[g[0]][0], mem[best][4], mem[best][5], box, mask))
            st["events"].append({"plane": p, "tiles": sorted({mem[a][1] for a in g}),
                                 "complete": all((a, b) in direct for a in g for b in g if a < b and mem[a][1] != mem[b][1])})
        events.sort(key=lambda e: (-float(e[1]), e[0]))
        for m in mem:
            out["rfi_mask"][p] |= m[2].astype(np.uint8)
        out["counts"][p] = min(len(events), E)
        for k, (_, sc, lab, box, mask) in enumerate(events[:E]):
            out["boxes"][p, k], out["scores"][p, k], out["labels"][p, k], out["masks"][p, k] = box, sc, lab, mask
        st.setdefault("n_events", []).append(len(events))
    if stats is not None:
        stats.update(st)
    return out
