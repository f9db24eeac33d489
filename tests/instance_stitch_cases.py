"""Inputs of the instance-stitch tests: the 96 x 80 scene and its perfect per-tile detections, the case table, seeded random
cases.  Every case is a dict: det (boxes, scores, labels, counts, masks of the tiles), C, T and the keyword arguments
(ps, stride, views, edge, max_events, min_area, min_score, class_aware, connectivity)."""
import numpy as np

import instance_stitch_ref as ref

SCENE_SHAPE = (96, 80)
SCENE_TILINGS = [(32, 32), (32, 16), (32, 24), (64, 48)]
DEFAULTS = dict(stride=None, views=1, edge="pad", max_events=64, min_area=1, min_score=0.0, class_aware=True, connectivity=8)


def scene():
    """-> [(label, score, (C, T) bool mask)]: two parallel lines of class 1 two pixels apart, two lines of class 2 crossing
    them, a 2-pixel-wide diagonal sweep (3), a blob inside a tile (4), a blob on a tile corner (5)."""
    C, T = SCENE_SHAPE
    z = lambda: np.zeros((C, T), bool)  # noqa: E731
    ev = []
    for row, score in ((10, 0.95), (12, 0.9)):
        m = z(); m[row, :] = True; ev.append((1, score, m))
    for col, score in ((20, 0.85), (50, 0.8)):
        m = z(); m[:, col] = True; ev.append((2, score, m))
    m = z()
    for i in range(78):
        m[i + 14, i] = m[i + 14, i + 1] = True
    ev.append((3, 0.75, m))
    m = z(); m[70:76, 4:10] = True; ev.append((4, 0.7, m))
    m = z(); m[30:35, 62:67] = True; ev.append((5, 0.65, m))
    return ev


def cut(events, C, T, ps, s, views, edge, D, planes=1):
    """The perfect detections of `events` (one list per plane, or one list for every plane): per tile, every event's mask
    restricted to the tile, boxed by its extent in tile coordinates."""
    table = ref.tile_table(C, T, ps, s, views, edge)
    N = planes * len(table)
    det = {"boxes": np.zeros((N, D, 4), np.float32), "scores": np.zeros((N, D), np.float32), "labels": np.zeros((N, D), np.int32),
           "counts": np.zeros((N,), np.int32), "masks": np.zeros((N, D, ps, ps), np.uint8)}
    for p in range(planes):
        evs = events[p] if isinstance(events[0], list) else events
        for ti, (v, r0, c0) in enumerate(table):
            i, k = p * len(table) + ti, 0
            for label, score, mask in evs:
                vw = ref.view_of(mask, v)[r0:r0 + ps, c0:c0 + ps]
                if not vw.any():
                    continue
                ys, xs = np.nonzero(vw)
                det["masks"][i, k, :vw.shape[0], :vw.shape[1]] = vw
                det["boxes"][i, k] = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
                det["scores"][i, k], det["labels"][i, k] = score, label
                k += 1
            det["counts"][i] = k
    return det


def scene_case(ps, s, views, edge, connectivity, D=8, **kw):
    C, T = SCENE_SHAPE
    return dict(det=cut(scene(), C, T, ps, s, views, edge, D), C=C, T=T, ps=ps,
                **{**DEFAULTS, "stride": s, "views": views, "edge": edge, "connectivity": connectivity, **kw})


def _garbage(det, seed):
    """Fill everything behind the counts with values that would change the result if they were read."""
    rng = np.random.default_rng(seed)
    N, D = det["scores"].shape
    for i in range(N):
        k = int(det["counts"][i])
        det["masks"][i, k:] = 255
        det["scores"][i, k:] = 2.0
        det["labels"][i, k:] = det["labels"][i, 0] if k else 1
        det["boxes"][i, k:] = rng.uniform(-50, 50, (D - k, 4)).astype(np.float32)
    return det


def _seam_case(connectivity):
    """Two segments one pixel apart diagonally across the seam of a 32 x 64 plane: linked 8-connected, apart 4-connected."""
    det = {"boxes": np.zeros((2, 1, 4), np.float32), "scores": np.full((2, 1), 0.5, np.float32), "labels": np.ones((2, 1), np.int32),
           "counts": np.ones((2,), np.int32), "masks": np.zeros((2, 1, 32, 32), np.uint8)}
    det["masks"][0, 0, 10, 20:32] = 1
    det["masks"][1, 0, 11, 0:9] = 3
    det["boxes"][0, 0], det["boxes"][1, 0] = (20, 10, 32, 11), (0, 11, 9, 12)
    return dict(det=det, C=32, T=64, ps=32, **{**DEFAULTS, "connectivity": connectivity})


def _edge_case():
    """40 x 40 planes in padded 32-tiles, D = 130, two planes (the second without detections): a padding-only detection,
    a score tie, a low score, a two-pixel detection under min_area = 3, more events than max_events = 3, and slot 129 of a
    full tile as one half of an event."""
    C = T = 40
    D, ps = 130, 32
    N = 2 * 4
    det = {"boxes": np.zeros((N, D, 4), np.float32), "scores": np.zeros((N, D), np.float32), "labels": np.ones((N, D), np.int32),
           "counts": np.zeros((N,), np.int32), "masks": np.zeros((N, D, ps, ps), np.uint8)}

    def put(i, j, r, c, h, w, score, label=1, value=1):
        det["masks"][i, j, r:r + h, c:c + w] = value
        det["boxes"][i, j] = (c, r, c + w, r + h)
        det["scores"][i, j], det["labels"][i, j] = score, label
    # tile 0 (rows 0-31, cols 0-31): 130 slots; 0 .. 128 are single pixels with a score under min_score, 129 reaches the seam
    for j in range(129):
        put(0, j, 2 + (j // 16) * 2, 1 + (j % 16) * 2, 1, 1, 0.05)
    put(0, 129, 28, 20, 3, 12, 0.6, value=200)
    det["counts"][0] = 130
    # tile 1 (cols 32-71, 8 of them in the plane): the other half of slot 129's event; a padding-only one; a tie
    put(1, 0, 29, 0, 1, 6, 0.6)
    put(1, 1, 3, 10, 5, 5, 0.99)                      # columns 42 .. 46 of the plane do not exist
    put(1, 2, 5, 2, 4, 3, 0.8, label=2)
    det["counts"][1] = 3
    # tile 2 (rows 32-71): the partner of the tie, a two-pixel one, and a straddler of which one pixel is in the plane
    put(2, 0, 1, 3, 4, 4, 0.8, label=3)
    put(2, 1, 5, 20, 1, 2, 0.9, label=4)
    put(2, 2, 7, 10, 4, 2, 0.7, label=5)              # rows 39 .. 42: two pixels in the plane
    put(2, 3, 2, 25, 3, 3, 0.5, label=4)
    det["counts"][2] = 4
    put(3, 0, 0, 0, 6, 6, 0.4, label=2)
    det["counts"][3] = 1
    return dict(det=_garbage(det, 5), C=C, T=T, ps=ps, **{**DEFAULTS, "max_events": 3, "min_area": 3, "min_score": 0.1})


def _aligned_case():
    """One 64 x 64 plane, ps = 64, two views, D = 256: every tile is the whole plane, all links are shared pixels."""
    rng = np.random.default_rng(11)
    ev = []
    for k in range(5):
        m = np.zeros((64, 64), bool)
        r, c = rng.integers(0, 50, 2)
        m[r:r + rng.integers(1, 14), c:c + rng.integers(1, 14)] = True
        ev.append((1 + k % 3, 0.9 - 0.1 * k, m))
    det = cut(ev, 64, 64, 64, 64, 2, "pad", 256)
    return dict(det=_garbage(det, 6), C=64, T=64, ps=64, **{**DEFAULTS, "views": 2})


def table():
    """name -> case."""
    t = {
        "scene_s32": scene_case(32, 32, 1, "pad", 8),
        "scene_s24_v4_shift_c4_any": scene_case(32, 24, 4, "shift", 4, D=64, class_aware=False),
        "scene_s24_pad": scene_case(32, 24, 1, "pad", 4, D=7),
        "scene_s16_v2": scene_case(32, 16, 2, "pad", 8, D=65),
        "seam_c8": _seam_case(8),
        "seam_c4": _seam_case(4),
        "edges_d130": _edge_case(),
        "aligned_d256": _aligned_case(),
    }
    _garbage(t["scene_s16_v2"]["det"], 3)
    return t


def random_case(seed, D, planes):
    """Random rectangles and lines per plane, cut into perfect detections of random classes, then disturbed: a few slots
    dropped, scores drawn from a small set (ties), garbage behind the counts."""
    rng = np.random.default_rng(seed)
    C, T = int(rng.integers(40, 97)), int(rng.integers(40, 81))
    ps, s = 32, int(rng.choice([32, 24, 16]))
    views, edge = int(rng.choice([1, 2, 4])), str(rng.choice(["pad", "shift"]))
    per_plane = []
    for _ in range(planes):
        ev = []
        for _ in range(int(rng.integers(min(D, 3), min(D, 10) + 1))):
            m = np.zeros((C, T), bool)
            kind = rng.integers(0, 3)
            if kind == 0:
                m[rng.integers(0, C), :] = True
            elif kind == 1:
                m[:, rng.integers(0, T)] = True
            else:
                r, c = rng.integers(0, C - 4), rng.integers(0, T - 4)
                m[r:r + rng.integers(1, 30), c:c + rng.integers(1, 30)] = True
            ev.append((int(rng.integers(1, 6)), float(rng.choice([0.3, 0.5, 0.7, 0.9])), m))
        per_plane.append(ev)
    if not any(per_plane):
        per_plane[0].append((1, 0.5, np.ones((C, T), bool)))
    events = [e if e else [(1, 0.5, np.zeros((C, T), bool))] for e in per_plane]
    det = cut(events, C, T, ps, s, views, edge, D, planes)
    if D > 10:                     # the first tile of every plane is full: its detections in the last slots, single pixels before
        ppp = len(det["counts"]) // planes
        for i in range(0, planes * ppp, ppp):
            k = int(det["counts"][i])
            for key in ("boxes", "scores", "labels", "masks"):
                det[key][i, D - k:] = det[key][i, :k].copy()
            for j in range(D - k):
                r, c = j % ps, (j * 7) % ps
                det["masks"][i, j] = 0
                det["masks"][i, j, r, c] = 1 + j % 255
                det["boxes"][i, j] = (c, r, c + 1, r + 1)
                det["scores"][i, j], det["labels"][i, j] = 0.35, 3
            det["counts"][i] = D
    drop = rng.random(det["counts"].shape) < 0.1
    det["counts"][drop] = np.maximum(det["counts"][drop] - 1, 0)
    return dict(det=_garbage(det, seed + 1), C=C, T=T, ps=ps,
                **{**DEFAULTS, "stride": s, "views": views, "edge": edge, "connectivity": int(rng.choice([4, 8])),
                   "class_aware": bool(rng.integers(0, 2)), "max_events": int(rng.choice([4, 64])), "min_area": int(rng.choice([1, 5])),
                   "min_score": float(rng.choice([0.0, 0.4]))})


RANDOM_CASES = [(21, 3, 2), (22, 65, 3), (23, 256, 2), (24, 3, 3), (25, 65, 2), (26, 256, 3), (27, 65, 3), (28, 3, 2)]


def run_ref(case, stats=None):
    d = case["det"]
    kw = {k: case[k] for k in DEFAULTS}
    return ref.stitch(d["boxes"], d["scores"], d["labels"], d["counts"], d["masks"], case["C"], case["T"], case["ps"], stats=stats, **kw)
