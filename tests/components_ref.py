"""The connected-component arithmetic of include/rfi_hip.h ("connected components") restated in NumPy and scipy, and the
case table of tests/test_components_host.py and tests/test_gpu_components.py.  Labels come from scipy.ndimage.label, which
numbers components by the smallest linear index they contain; everything else follows from the labels."""
import numpy as np
import scipy.ndimage as ndi


def structure(connectivity):
    return ndi.generate_binary_structure(2, 1 if connectivity == 4 else 2)


def label(mask, connectivity):
    """-> (labels int32 (H, W), K)."""
    lab, k = ndi.label(np.asarray(mask) != 0, structure(connectivity))
    return lab.astype(np.int32), int(k)


def table(labels, k):
    """-> area int32 (K,), box int32 (K, 4) = (xmin, ymin, xmax, ymax) inclusive, in label order."""
    area = np.bincount(labels.ravel(), minlength=k + 1)[1:].astype(np.int32)
    box = np.zeros((k, 4), np.int32)
    for l, sl in enumerate(ndi.find_objects(labels, max_label=k)):
        box[l] = (sl[1].start, sl[0].start, sl[1].stop - 1, sl[0].stop - 1)
    return area, box


def despeckle(mask, min_area, connectivity):
    """-> bool (H, W): foreground whose component has at least min_area pixels."""
    lab, k = label(mask, connectivity)
    area, _ = table(lab, k)
    return (lab > 0) & (np.concatenate([[0], area])[lab] >= min_area)


def instances(mask, connectivity, min_area=1, min_side=1, max_instances=64):
    """One plane's instance targets: dict of boxes float32 (G, 4) half-open, labels int32 (G,), component int32 (G,), count,
    n_survivors, n_components, masks uint8 (count, H, W); slots in descending area, ties by ascending label."""
    lab, k = label(mask, connectivity)
    area, box = table(lab, k)
    ok = (area >= min_area) & (box[:, 2] - box[:, 0] + 1 >= min_side) & (box[:, 3] - box[:, 1] + 1 >= min_side)
    surv = np.flatnonzero(ok)                                                  # ascending label
    order = surv[np.argsort(-area[surv].astype(np.int64), kind="stable")]      # descending area, ties ascending label
    kept = order[:max_instances]
    g = max_instances
    boxes, labels, comp = np.zeros((g, 4), np.float32), np.zeros(g, np.int32), np.zeros(g, np.int32)
    for j, c in enumerate(kept):
        boxes[j] = (box[c, 0], box[c, 1], box[c, 2] + 1, box[c, 3] + 1)
        labels[j], comp[j] = 1, c + 1
    masks = np.stack([lab == c + 1 for c in kept]).astype(np.uint8) if len(kept) else np.zeros((0,) + lab.shape, np.uint8)
    return {"boxes": boxes, "labels": labels, "component": comp, "count": len(kept), "n_survivors": len(surv), "n_components": k,
            "masks": masks, "areas": area[kept]}


def sweeps(mask, connectivity):
    """How many whole-plane sweeps of "take the smallest label among my neighbours" a plane needs before nothing changes:
    what a method without union-find would pay, and what makes a case hard for one with it."""
    fg = np.asarray(mask) != 0
    h, w = fg.shape
    big = h * w
    lab = np.where(fg, np.arange(big).reshape(h, w), big)
    offs = [(0, 1), (1, 0), (0, -1), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 8 else [])
    n = 0
    while True:
        n += 1
        pad = np.pad(lab, 1, constant_values=big)
        new = lab
        for dy, dx in offs:
            new = np.minimum(new, pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w])
        new = np.where(fg, new, big)
        if np.array_equal(new, lab):
            return n
        lab = new


# ---------------------------------------------------------------------------------------------- planes
def serpentine(h, w):
    """Every other row full, joined to the next full row at alternating ends: one long snake."""
    m = np.zeros((h, w), np.uint8)
    m[::2] = 1
    for i, r in enumerate(range(1, h - 1, 2)):
        m[r, -1 if i % 2 == 0 else 0] = 1
    return m


def checkerboard(h, w):
    return (np.indices((h, w)).sum(0) % 2 == 0).astype(np.uint8)


def diagonal(h, w):
    """y == x: through every tile corner (64 k, 64 k); one component under 8, every pixel its own under 4."""
    m = np.zeros((h, w), np.uint8)
    i = np.arange(min(h, w))
    m[i, i] = 1
    return m


def anti_diagonal(h, w, c=127):
    """x + y == c: crosses the tile corner (64, 64) from (63, 64) to (64, 63)."""
    m = np.zeros((h, w), np.uint8)
    y = np.arange(h)
    x = c - y
    ok = (x >= 0) & (x < w)
    m[y[ok], x[ok]] = 1
    return m


def cross(n):
    return ((np.eye(n) + np.eye(n)[::-1]) > 0).astype(np.uint8)


def corners(h, w):
    m = np.zeros((h, w), np.uint8)
    m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = 1
    return m


def random_plane(h, w, density, seed):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8)


def basic_cases():
    """name -> plane: the small cases every labelling test runs, under both connectivities."""
    rng = np.random.default_rng(0)
    return {
        "empty_5x7": np.zeros((5, 7), np.uint8),
        "full_9x65": np.ones((9, 65), np.uint8),
        "row_1x130": random_plane(1, 130, 0.6, 1),
        "column_130x1": random_plane(130, 1, 0.6, 2),
        "corners_6x9": corners(6, 9),
        "corners_1x1": np.ones((1, 1), np.uint8),
        "checker_16x18": checkerboard(16, 18),
        "cross_19": cross(19),
        "random_37x70": random_plane(37, 70, 0.5, 3),
        "random_64x64": random_plane(64, 64, 0.6, 4),
        "values_40x40": (rng.integers(0, 3, (40, 40)) * 85).astype(np.int64),
        "serpentine_33": serpentine(33, 33),
    }


def gate_shapes(tile_h, tile_w, scan_block):
    """Plane shapes just below, at and just above the sizes at which the kernels' paths change, plus shapes that are no
    multiple of the tile."""
    return [(tile_h, tile_w), (tile_h - 1, tile_w - 1), (tile_h + 1, tile_w), (tile_h, tile_w + 1), (1, scan_block), (1, scan_block + 1),
            (2 * tile_h + 1, 2 * tile_w + 1), (130, 67), (257, 300)]


def gate_cases(shape):
    h, w = shape
    return {"serpentine": serpentine(h, w), "random": random_plane(h, w, 0.5, h * 1000 + w), "diagonal": diagonal(h, w),
            "anti_diagonal": anti_diagonal(h, w)}


def batch_stack():
    """Planes of one shape for one batched call: the last row of plane 1 and the first row of plane 2 are full, plane 3 is
    empty, so a leak across planes changes labels and counts."""
    a = random_plane(37, 70, 0.5, 5)
    b = random_plane(37, 70, 0.3, 6)
    b[-1] = 1
    c = random_plane(37, 70, 0.3, 7)
    c[0] = 1
    return np.stack([a, b, c, np.zeros((37, 70), np.uint8), np.ones((37, 70), np.uint8), serpentine(37, 70)])


def _rect(m, y, x, h, w):
    m[y:y + h, x:x + w] = 1


def tie_plane(flip=False):
    """64 x 80, separated rectangles: two of area 100, two of area 25 (the cuts at 1 and at 3 instances fall between equal
    areas), a 1 x 20 line (min_side = 2 removes it, min_area = 16 keeps it), a 3 x 3 square (min_area = 16 removes it,
    min_side = 2 keeps it), a 4 x 4 square and two single pixels."""
    m = np.zeros((64, 80), np.uint8)
    _rect(m, 2, 2, 10, 10)
    _rect(m, 2, 20, 10, 10)
    _rect(m, 20, 2, 5, 5)
    _rect(m, 20, 12, 5, 5)
    _rect(m, 30, 2, 1, 20)
    _rect(m, 40, 2, 3, 3)
    _rect(m, 40, 10, 4, 4)
    m[50, 5] = m[55, 70] = 1
    return m[::-1, ::-1].copy() if flip else m


def speck_plane():
    """64 x 80 with isolated single pixels only: no survivor once min_area >= 2."""
    m = np.zeros((64, 80), np.uint8)
    m[5:60:9, 3:78:11] = 1
    return m


def instance_stack():
    return np.stack([tie_plane(), speck_plane(), tie_plane(flip=True)])


INSTANCE_PARAMS = [dict(min_area=1, min_side=1, max_instances=256), dict(min_area=4, min_side=1, max_instances=256),
                   dict(min_area=16, min_side=1, max_instances=3), dict(min_area=1, min_side=2, max_instances=1),
                   dict(min_area=2, min_side=2, max_instances=3)]
