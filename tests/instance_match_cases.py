"""Case table of instance matching, shared by the host test (which first checks that the table holds what it claims, with
the NumPy restatement alone) and the GPU test.  A case is a dict of padded arrays in the layout of the C ABI:

    det_masks uint8 (n, D, H, W), det_boxes float32 (n, D, 4), scores float32 (n, D), det_labels int32 (n, D), det_count (n,)
    gt_masks  uint8 (n, G, H, W), gt_boxes  float32 (n, G, 4), gt_labels int32 (n, G), gt_count (n,)

Every slot behind a count holds garbage that would change the result if anything read it: full masks of byte 255, the
highest score, label 1, a box over the whole plane."""
import numpy as np

TABLE_THRESHOLDS = np.asarray([0.25, 0.5, 0.75], np.float32)
TABLE_SHAPE = (6, 70)                  # two word columns, the second one 6 bits wide


def tight_box(mask):
    """(xmin, ymin, xmax + 1, ymax + 1) of the non-zero bytes, (0, 0, 0, 0) for an empty mask."""
    ys, xs = np.nonzero(mask)
    if not len(ys):
        return np.zeros(4, np.float32)
    return np.asarray([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1], np.float32)


def assemble(images, shape, pad_d=0, pad_g=0):
    """images: [(dets, gts)] with dets = [(mask, score, label)], gts = [(mask, label)] -> the padded case, garbage behind
    the counts.  pad_d / pad_g: extra slots beyond the longest list."""
    n, (H, W) = len(images), shape
    D = max(len(d) for d, _ in images) + pad_d
    G = max(len(g) for _, g in images) + pad_g
    c = {"det_masks": np.full((n, D, H, W), 255, np.uint8), "det_boxes": np.tile(np.asarray([0, 0, W, H], np.float32), (n, D, 1)),
         "scores": np.full((n, D), 5.0, np.float32), "det_labels": np.ones((n, D), np.int32), "det_count": np.zeros(n, np.int32),
         "gt_masks": np.full((n, G, H, W), 255, np.uint8), "gt_boxes": np.tile(np.asarray([0, 0, W, H], np.float32), (n, G, 1)),
         "gt_labels": np.ones((n, G), np.int32), "gt_count": np.zeros(n, np.int32), "shape": (H, W)}
    for i, (dets, gts) in enumerate(images):
        c["det_count"][i], c["gt_count"][i] = len(dets), len(gts)
        for d, (m, s, lab) in enumerate(dets):
            c["det_masks"][i, d], c["det_boxes"][i, d], c["scores"][i, d], c["det_labels"][i, d] = m, tight_box(m), s, lab
        for g, (m, lab) in enumerate(gts):
            c["gt_masks"][i, g], c["gt_boxes"][i, g], c["gt_labels"][i, g] = m, tight_box(m), lab
    return c


def lists_of(c):
    """The padded case as the two list forms of the Python surface (what lies behind the counts is dropped)."""
    dets, tgts = [], []
    for i in range(len(c["det_count"])):
        k, g = int(c["det_count"][i]), int(c["gt_count"][i])
        dets.append({"boxes": c["det_boxes"][i, :k].copy(), "scores": c["scores"][i, :k].copy(), "labels": c["det_labels"][i, :k].astype(np.int64),
                     "masks": c["det_masks"][i, :k] != 0})
        tgts.append({"boxes": c["gt_boxes"][i, :g].copy(), "labels": c["gt_labels"][i, :g].astype(np.int64), "masks": c["gt_masks"][i, :g].copy()})
    return dets, tgts


def _m(shape, *rects, value=1):
    """a mask with the half-open rectangles (r0, r1, c0, c1) set to `value`"""
    m = np.zeros(shape, np.uint8)
    for r0, r1, c0, c1 in rects:
        m[r0:r1, c0:c1] = value
    return m


def table():
    """The hand-made case; tests/test_instance_match_host.py asserts every property named here.

    image 0, all of label 1:
      g0 row 0 x 0..9; g1 row 1 x 0..9; g2 row 3 x 64..65; g3 (4, 0); g4 (4, 1); g5 row 5 x 0..4; g6 empty
      d0 .9  = g0 exactly                         IoU 1.0 (identical masks)
      d1 .8  row 0 x 0..9 + row 1 x 0..5          g0: 10/16, g1: 6/20 = 0.3: its best is taken by d0, it falls to g1 at t = .25
      d2 .7  (3, 64)                              g2: 1/2, exactly the threshold .5
      d3 .7  row 4 x 0..1                         g3 and g4: 1/2 each, the tie goes to g3
      d4 .6  row 5 x 0..2                         g5: 3/5: matched at .5, not at .75
      d5 .5  empty
      d6 .7  (3, 65)                              g2: 1/2, the same score as d2: the lower slot d2 wins g2
    image 1: g0 rows 0..1 x 60..69 in bytes of 255, label 1; d0 the same pixels in bytes of 2, label 2 (matches only when
             class-agnostic); d1 label 1, column 0, no overlap
    image 2: no detections, two ground truths.   image 3: two detections, no ground truth."""
    S = TABLE_SHAPE
    img0 = ([(_m(S, (0, 1, 0, 10)), 0.9, 1), (_m(S, (0, 1, 0, 10), (1, 2, 0, 6)), 0.8, 1), (_m(S, (3, 4, 64, 65)), 0.7, 1),
             (_m(S, (4, 5, 0, 2)), 0.7, 1), (_m(S, (5, 6, 0, 3)), 0.6, 1), (_m(S), 0.5, 1), (_m(S, (3, 4, 65, 66)), 0.7, 1)],
            [(_m(S, (0, 1, 0, 10)), 1), (_m(S, (1, 2, 0, 10)), 1), (_m(S, (3, 4, 64, 66)), 1), (_m(S, (4, 5, 0, 1)), 1),
             (_m(S, (4, 5, 1, 2)), 1), (_m(S, (5, 6, 0, 5)), 1), (_m(S), 1)])
    img1 = ([(_m(S, (0, 2, 60, 70), value=2), 0.9, 2), (_m(S, (0, 6, 0, 1)), 0.8, 1)], [(_m(S, (0, 2, 60, 70), value=255), 1)])
    img2 = ([], [(_m(S, (2, 3, 0, 70)), 1), (_m(S, (0, 6, 69, 70)), 2)])
    img3 = ([(_m(S, (2, 3, 0, 70)), 0.4, 1), (_m(S, (0, 6, 69, 70)), 0.3, 2)], [])
    return assemble([img0, img1, img2, img3], S, pad_d=1, pad_g=1)


def random_case(seed, n, D, G, shape, num_labels=3):
    """Thin rows and columns, rectangles, full and empty planes; counts at and below D and G; scores with ties (two
    decimals); boxes = the tight boxes moved by fractions of a pixel."""
    rng = np.random.default_rng(seed)
    H, W = shape

    def mask():
        kind = rng.integers(0, 10)
        m = np.zeros(shape, np.uint8)
        value = (1, 1, 2, 255)[rng.integers(0, 4)]
        if kind <= 2:
            r = rng.integers(0, H)
            a, b = sorted(rng.integers(0, W + 1, 2))
            m[r, a:max(b, a + 1)] = value
        elif kind <= 5:
            col = rng.integers(0, W)
            a, b = sorted(rng.integers(0, H + 1, 2))
            m[a:max(b, a + 1), col] = value
        elif kind <= 7:
            r0, r1 = sorted(rng.integers(0, H + 1, 2))
            c0, c1 = sorted(rng.integers(0, W + 1, 2))
            m[r0:max(r1, r0 + 1), c0:max(c1, c0 + 1)] = value
        elif kind == 8:
            m[:] = value
        return m

    images = []
    for i in range(n):
        nd = D if i == 0 else int(rng.integers(0, D + 1))
        ng = G if i == 0 else int(rng.integers(0, G + 1))
        gts = [(mask(), int(rng.integers(1, num_labels + 1))) for _ in range(ng)]
        dets = []
        for d in range(nd):
            # half of the detections are a ground truth (mostly with its label), cut by a row or grown by a few pixels,
            # so that overlaps at every threshold occur
            lab = int(rng.integers(1, num_labels + 1))
            if gts and rng.random() < 0.5:
                m, glab = gts[int(rng.integers(0, len(gts)))]
                m = m.copy()
                r, x = int(rng.integers(0, H)), int(rng.integers(0, W))
                if rng.random() < 0.5:
                    m[r, :] = 0
                else:
                    m[r, x:x + int(rng.integers(1, 5))] = 1
                if rng.random() < 0.75:
                    lab = glab
            else:
                m = mask()
            dets.append((m, np.float32(np.round(rng.random(), 2)), lab))
        images.append((dets, gts))
    c = assemble(images, shape)
    # the list lengths of image 0 are D and G: the padded widths are exactly those asked for
    assert c["det_masks"].shape[1] == D and c["gt_masks"].shape[1] == G
    jitter = lambda b: (b + rng.uniform(-0.75, 0.75, b.shape)).astype(np.float32)  # noqa: E731
    c["det_boxes"], c["gt_boxes"] = jitter(c["det_boxes"]), jitter(c["gt_boxes"])
    return c


# (n, D, G, T, shape): n in {1, 3}; D, G in {1, 5, 64, 65, 256} (65: a second ground truth per lane, 256: the cap);
# T in {1, 10, 32}.  The plain double loop of the restatement costs n T D G steps: the products stay below 2e5.
RANDOM_SETS = [(1, 1, 1, 1, (3, 63)), (3, 5, 65, 10, (5, 64)), (1, 64, 5, 32, (4, 65)), (3, 65, 64, 10, (7, 130)),
               (1, 256, 256, 1, (9, 70)), (1, 5, 256, 32, (5, 64)), (3, 256, 5, 10, (4, 65)), (1, 65, 256, 10, (7, 130)),
               (3, 64, 1, 1, (33, 257)), (1, 1, 64, 10, (64, 64))]
PACK_SHAPES = [(1, 1), (3, 63), (5, 64), (4, 65), (7, 130), (33, 257), (64, 64)]


def thresholds_of(T):
    """T thresholds in (0, 1]: COCO's ten, a single 0.5, or 32 evenly spaced ones that end at 1."""
    if T == 10:
        return np.arange(50, 100, 5, dtype=np.float32) / np.float32(100)
    if T == 1:
        return np.asarray([0.5], np.float32)
    return (np.arange(1, T + 1, dtype=np.float32) / np.float32(T)).astype(np.float32)
