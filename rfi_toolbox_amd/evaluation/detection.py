"""Scoring detections per instance: which emitters were found, at which overlap, with how many false alarms, at what AP.

    det = detector.detect(images, out="device")                        # boxes, scores, labels, counts, masks in HBM
    targets = event_instances(batch, max_instances=16)                 # InstanceTargets in HBM
    m = match_instances(det, targets)                                  # InstanceMatch: iou, inter, det_match, gt_match
    print(score_detections(det, targets, num_classes=6, class_names=EVENT_CLASSES))

``match_instances`` runs on the GPU (csrc/instance_match.hip; the rules are pinned in include/rfi_hip.h, "instance
matching"): the masks of both sides are packed to bit planes, every (detection, ground truth) pair of an image gets its
mask or box IoU, and COCO's greedy matching runs at every IoU threshold in one launch.  With the device dict of
``MaskRCNN.detect(out="device")`` and ``InstanceTargets`` nothing is uploaded or downloaded.  There is no CPU path.

``DetectionScorer`` collects one record per detection (score, label, matched or not at every threshold) over any number
of batches and forms AP / AR on the host in float64 (``scores_from_matches``): the arithmetic of COCO's ``accumulate``
for one area range and one ``maxDets``, without crowd or ignore regions.  The definition is COCO's; it was not compared
against pycocotools.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from .._lib import check, lib
from ..runtime import DeviceArray, P, context_for, describe, operand

MAX_SLOTS = 256                 # D and G of one call: detect's post_nms cap and components.MAX_INSTANCES
MAX_THRESHOLDS = 32
MAX_PLANE = 1 << 24
MAX_IMAGES = 65535
KINDS = ("mask", "box")
RECALL_POINTS = np.linspace(0.0, 1.0, 101)


def default_iou_thresholds():
    """0.50, 0.55, ..., 0.95 in float32 (COCO's); contains exactly ``np.float32(0.5)`` and ``np.float32(0.75)``."""
    return np.arange(50, 100, 5, dtype=np.float32) / np.float32(100)


def _thresholds(iou_thresholds):
    thr = default_iou_thresholds() if iou_thresholds is None else np.asarray(iou_thresholds)
    if thr.ndim != 1 or not 1 <= thr.size <= MAX_THRESHOLDS:
        raise ValueError(f"iou_thresholds must be a 1-D sequence of 1 .. {MAX_THRESHOLDS} values, got shape {thr.shape}")
    with np.errstate(over="ignore", invalid="ignore"):
        thr = np.ascontiguousarray(thr.astype(np.float32))
    if not np.all(np.isfinite(thr)) or not np.all((thr > 0) & (thr <= 1)):
        raise ValueError(f"iou_thresholds must be finite and in (0, 1], got {thr.tolist()}")
    return thr


# ---------------------------------------------------------------------------------------------- the two sides
class _Side:
    """One side of the comparison as the kernels take it, before anything touches a device: padded arrays of ``slots``
    per image -- DeviceArrays used in place or host arrays still to upload -- and the plane shape of the masks."""

    def __init__(self, n, slots, boxes, labels, count, scores=None, masks=None, base=None, planes=0, shape=None):
        self.n, self.slots, self.boxes, self.labels, self.count, self.scores = n, slots, boxes, labels, count, scores
        self.masks, self.base, self.planes, self.shape = masks, base, planes, shape

    def arrays(self):
        return [a for a in (self.boxes, self.labels, self.count, self.scores, self.masks, self.base) if a is not None]


def _pad_list(items, name, with_scores):
    """list of per-image dicts -> host arrays padded to the longest list (no device call)."""
    n = len(items)
    for it in items:
        if not isinstance(it, dict) or "boxes" not in it or "labels" not in it or (with_scores and "scores" not in it):
            raise ValueError(f"{name}: every item must be a dict with 'boxes', 'labels'" + (", 'scores'" if with_scores else ""))
    boxes = [np.asarray(it["boxes"], np.float32).reshape(-1, 4) for it in items]
    count = np.asarray([len(b) for b in boxes], np.int32)
    slots = int(count.max()) if n else 0
    if slots > MAX_SLOTS:
        raise ValueError(f"{name}: at most {MAX_SLOTS} per image, got {slots}")
    pb, pl = np.zeros((n, slots, 4), np.float32), np.zeros((n, slots), np.int32)
    ps = np.zeros((n, slots), np.float32) if with_scores else None
    for i, it in enumerate(items):
        k = int(count[i])
        lab = np.asarray(it["labels"]).reshape(-1)
        if len(lab) != k:
            raise ValueError(f"{name}[{i}]: {k} boxes but {len(lab)} labels")
        pb[i, :k], pl[i, :k] = boxes[i], lab
        if with_scores:
            sc = np.asarray(it["scores"], np.float32).reshape(-1)
            if len(sc) != k:
                raise ValueError(f"{name}[{i}]: {k} boxes but {len(sc)} scores")
            if not np.all(np.isfinite(sc)):
                raise ValueError(f"{name}[{i}]: scores must be finite")
            ps[i, :k] = sc
    have = [it.get("masks") is not None for it in items]
    shape, masks = None, None
    if n and all(have):
        ms = []
        for i, it in enumerate(items):
            m = np.asarray(it["masks"])
            if m.ndim != 3 or len(m) != int(count[i]):
                raise ValueError(f"{name}[{i}]: masks must be ({int(count[i])}, H, W), got {m.shape}")
            if shape is None:
                shape = tuple(m.shape[1:])
            elif tuple(m.shape[1:]) != shape:
                raise ValueError(f"{name}[{i}]: mask planes of {m.shape[1:]} among planes of {shape}")
            ms.append((m != 0).view(np.uint8) if m.dtype != np.uint8 else m)
        masks = ms
    return n, slots, pb, pl, count, ps, masks, shape


def _detections(det):
    if isinstance(det, dict):
        for k in ("boxes", "scores", "labels", "counts"):
            if k not in det:
                raise ValueError(f"detections: the dict lacks {k!r} (expected the result of MaskRCNN.detect(out='device'))")
        bshape = describe(det["boxes"])[0]
        if len(bshape) != 3 or bshape[2] != 4:
            raise ValueError(f"detections['boxes'] must be (n, D, 4), got {bshape}")
        n, D = bshape[0], bshape[1]
        for k, want in (("scores", (n, D)), ("labels", (n, D)), ("counts", (n,))):
            if describe(det[k])[0] != want:
                raise ValueError(f"detections[{k!r}] must be {want}, got {describe(det[k])[0]}")
        if D > MAX_SLOTS:
            raise ValueError(f"detections: at most {MAX_SLOTS} per image, got {D}")
        if not isinstance(det["scores"], DeviceArray) and not (hasattr(det["scores"], "is_cuda") and det["scores"].is_cuda):
            if not np.all(np.isfinite(np.asarray(det["scores"], np.float32))):
                raise ValueError("detections['scores'] must be finite")
        masks, shape = det.get("masks"), None
        if masks is not None:
            mshape = describe(masks)[0]
            if len(mshape) != 4 or mshape[:2] != (n, D):
                raise ValueError(f"detections['masks'] must be ({n}, {D}, H, W), got {mshape}")
            shape = tuple(mshape[2:])
        return _Side(n, D, det["boxes"], det["labels"], det["counts"], det["scores"], masks, None, n * D, shape)
    if not isinstance(det, (list, tuple)):
        raise ValueError(f"detections must be the dict of detect(out='device') or a list of dicts, got {type(det).__name__}")
    n, D, pb, pl, count, ps, masks, shape = _pad_list(det, "detections", True)
    pm = None
    if masks is not None:
        pm = np.zeros((n, D) + shape, np.uint8)
        for i, m in enumerate(masks):
            pm[i, :len(m)] = m
    return _Side(n, D, pb, pl, count, ps, pm, None, n * D, shape)


def _targets(tg):
    from ..components import InstanceTargets
    if isinstance(tg, InstanceTargets):
        n, G = len(tg), describe(tg.boxes)[0][1]
        return _Side(n, G, tg.boxes, tg.labels, tg.count, None, tg.masks, tg.base, tg.total, tuple(tg.shape) if tg.masks is not None else None)
    if not isinstance(tg, (list, tuple)):
        raise ValueError(f"targets must be InstanceTargets or a list of dicts, got {type(tg).__name__}")
    n, G, pb, pl, count, _, masks, shape = _pad_list(tg, "targets", False)
    cm, base = None, np.concatenate([[0], np.cumsum(count, dtype=np.int64)])[:-1].astype(np.int32)
    if masks is not None:
        cm = np.concatenate(masks).astype(np.uint8, copy=False) if len(masks) else np.zeros((0,) + shape, np.uint8)
    return _Side(n, G, pb, pl, count, None, cm, base, int(count.sum(dtype=np.int64)), shape)


# ---------------------------------------------------------------------------------------------- the match
@dataclass
class InstanceMatch:
    """What ``match_instances`` found.  ``iou`` float32 (n, D, G); ``inter`` int32 (n, D, G), the intersections in pixels
    (``kind="mask"`` only, else None); ``det_match`` int32 (n, T, D) and ``gt_match`` int32 (n, T, G), the partner's slot
    or -1 -- ``DeviceArray``s (NumPy arrays for an empty input).  Entries behind an image's counts are 0 and -1."""
    kind: str
    thresholds: np.ndarray
    class_aware: bool
    iou: object
    inter: object
    det_match: object
    gt_match: object
    _det: object = None
    _gt: object = None

    def numpy(self):
        """-> dict of host arrays: iou, inter (mask kind), det_match, gt_match, thresholds."""
        num = lambda a: a.numpy() if isinstance(a, DeviceArray) else np.asarray(a)  # noqa: E731
        out = {"iou": num(self.iou), "det_match": num(self.det_match), "gt_match": num(self.gt_match), "thresholds": self.thresholds.copy()}
        if self.inter is not None:
            out["inter"] = num(self.inter)
        return out

    def records(self):
        """The small arrays a scorer needs, on the host: det_match (n, T, D), scores (n, D), det labels (n, D), det counts
        (n,), ground-truth labels (n, G) and counts (n,)."""
        num = lambda a, dt: (a.numpy() if isinstance(a, DeviceArray) else _host(a)).astype(dt, copy=False)  # noqa: E731
        d, g = self._det, self._gt
        return (num(self.det_match, np.int32), num(d.scores, np.float32), num(d.labels, np.int32), num(d.count, np.int32),
                num(g.labels, np.int32), num(g.count, np.int32))


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _scratch(ctx, nbytes):
    """The context's grow-only scratch of this module: the bit planes, areas and extents of one call."""
    s = getattr(ctx, "_match_scratch", None)
    if s is None or s.nbytes < nbytes:
        ctx._match_scratch = s = None
        ctx._match_scratch = s = ctx.empty((nbytes,), np.uint8)
    return s


def _al(b):
    return (b + 255) & ~255


def match_instances(detections, targets, iou_thresholds=None, kind="mask", class_aware=True, device=None):
    """Pairwise IoU of every detection with every ground truth of its image, and COCO's greedy matching at every
    threshold of ``iou_thresholds`` (default 0.50 ... 0.95; at most 32, each in (0, 1]) -> ``InstanceMatch``.

    ``detections``: the dict of ``MaskRCNN.detect(out="device")`` (used in place) or the list of dicts of ``predict`` /
    ``detect(out="host")`` (padded to the longest list and uploaded once).  ``targets``: ``InstanceTargets`` or the list
    of dicts ``train_step`` takes.  ``kind="mask"`` compares instance masks, ``"box"`` boxes.  A detection takes the
    still-free ground truth of greatest IoU >= t, ties to the lowest slot, in descending score order, ties to the lower
    slot; with ``class_aware`` only a ground truth of its own label."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    thr = _thresholds(iou_thresholds)
    det, gt = _detections(detections), _targets(targets)
    if det.n != gt.n:
        raise ValueError(f"{det.n} images of detections, {gt.n} of targets")
    if det.n > MAX_IMAGES:
        raise ValueError(f"at most {MAX_IMAGES} images in one call, got {det.n}")
    if kind == "mask" and det.n:
        if gt.masks is None:
            raise ValueError("kind='mask' needs target masks (these targets were made with instance_masks=False); use kind='box'")
        if det.masks is None:
            raise ValueError("kind='mask' needs detections with 'masks' (detect(instance_masks=True)); use kind='box'")
        if det.n and det.slots and gt.slots and det.shape != gt.shape:
            raise ValueError(f"detection masks are {det.shape} planes, target masks {gt.shape}")
        if det.shape is not None and (min(det.shape) < 1 or det.shape[0] * det.shape[1] > MAX_PLANE):
            raise ValueError(f"mask planes need H, W >= 1 and H W <= 2^24, got {det.shape}")
    n, D, G, T = det.n, det.slots, gt.slots, thr.size
    class_aware = bool(class_aware)
    if n == 0 or D == 0 or G == 0:                                  # well-formed and empty: nothing is launched
        z = np.zeros((n, D, G), np.float32)
        return InstanceMatch(kind, thr, class_aware, z, np.zeros((n, D, G), np.int32) if kind == "mask" else None,
                             np.full((n, T, D), -1, np.int32), np.full((n, T, G), -1, np.int32), det, gt)
    ctx = context_for(device, *det.arrays(), *gt.arrays())
    up = lambda a, dt: operand(a, ctx, (dt,), "cast", to_device=True)  # noqa: E731
    d_scores, d_labels, d_count = up(det.scores, np.float32), up(det.labels, np.int32), up(det.count, np.int32)
    g_labels, g_count = up(gt.labels, np.int32), up(gt.count, np.int32)
    iou = ctx.empty((n, D, G), np.float32)
    inter, keep = None, [o.keep for o in (d_scores, d_labels, d_count, g_labels, g_count)]
    if kind == "box":
        d_boxes, g_boxes = up(det.boxes, np.float32), up(gt.boxes, np.float32)
        keep += [d_boxes.keep, g_boxes.keep]
        check(lib.rfi_op_box_iou(ctx.handle, C.c_void_p(d_boxes.ptr), C.c_void_p(d_count.ptr), C.c_void_p(g_boxes.ptr),
                                 C.c_void_p(g_count.ptr), n, D, G, P(iou)))
    else:
        h, w = det.shape
        wc = (w + 63) // 64
        d_masks = operand(det.masks, ctx, (np.uint8,), "nonzero", to_device=True)
        g_masks = operand(gt.masks, ctx, (np.uint8,), "nonzero", to_device=True) if gt.planes else None
        g_base = up(gt.base, np.int32)
        d_base = ctx.to_device(np.arange(n, dtype=np.int32) * D)
        keep += [d_masks.keep, g_masks.keep if g_masks else None, g_base.keep, d_base]
        sizes = []
        for m in (det.planes, gt.planes):
            sizes += [_al(8 * m * h * wc), _al(4 * m), _al(16 * m)]
        s = _scratch(ctx, sum(sizes) + 256)
        ptrs, p = [], _al(s.ptr)
        for b in sizes:
            ptrs.append(C.c_void_p(p))
            p += b
        check(lib.rfi_op_pack_masks(ctx.handle, C.c_void_p(d_masks.ptr), det.planes, h, w, *ptrs[:3]))
        if gt.planes:
            check(lib.rfi_op_pack_masks(ctx.handle, C.c_void_p(g_masks.ptr), gt.planes, h, w, *ptrs[3:]))
        inter = ctx.empty((n, D, G), np.int32)
        check(lib.rfi_op_mask_iou(ctx.handle, *ptrs[:3], C.c_void_p(d_count.ptr), P(d_base), det.planes, *ptrs[3:],
                                  C.c_void_p(g_count.ptr), C.c_void_p(g_base.ptr), gt.planes, n, D, G, h, w, P(inter), P(iou)))
    det_match, gt_match = ctx.empty((n, T, D), np.int32), ctx.empty((n, T, G), np.int32)
    check(lib.rfi_op_match_instances(ctx.handle, P(iou), C.c_void_p(d_scores.ptr), C.c_void_p(d_labels.ptr), C.c_void_p(d_count.ptr),
                                     C.c_void_p(g_labels.ptr), C.c_void_p(g_count.ptr), n, D, G, thr.ctypes.data_as(C.c_void_p), T,
                                     int(class_aware), P(det_match), P(gt_match)))
    iou._keep = keep                                  # (work in flight reads the inputs: they live as long as the result)
    # what a scorer reads back later: the arrays the kernels saw
    det_dev = _Side(n, D, None, d_labels.keep, d_count.keep, d_scores.keep)
    gt_dev = _Side(n, G, None, g_labels.keep, g_count.keep)
    return InstanceMatch(kind, thr, class_aware, iou, inter, det_match, gt_match, det_dev, gt_dev)


# ---------------------------------------------------------------------------------------------- AP on the host
def _ap_of(score, matched, n_gt):
    """COCO's accumulate for one (class, threshold): -> (AP, recall reached, precision, recall, score) with the three
    curves in descending score, stable over arrival order."""
    order = np.argsort(-score, kind="mergesort")
    m = matched[order]
    tp, fp = np.cumsum(m, dtype=np.float64), np.cumsum(~m, dtype=np.float64)
    recall, precision = tp / n_gt, tp / (tp + fp)
    env = precision.copy()
    for k in range(len(env) - 1, 0, -1):
        if env[k] > env[k - 1]:
            env[k - 1] = env[k]
    at = np.searchsorted(recall, RECALL_POINTS, side="left")
    q = np.zeros(len(RECALL_POINTS))
    ok = at < len(env)
    q[ok] = env[at[ok]]
    return float(q.mean()), float(recall[-1]) if len(recall) else 0.0, precision, recall, score[order]


def scores_from_matches(scores, labels, matched, n_gt, iou_thresholds=None, class_names=None):
    """AP / AR from plain host arrays, one entry per detection in arrival order: ``scores`` (N,), ``labels`` (N,) in
    1 .. num_classes - 1, ``matched`` (T, N) bool (matched at threshold t or not), ``n_gt`` (num_classes,) the ground truths
    per class (index 0, the background, is ignored).  -> {"AP", "AP50", "AP75", "AR", "per_class": {name: {"AP", "AP50",
    "AR", "n_gt", "n_det"}}} in float64.  A class without ground truth is NaN and left out of the means; AP50 / AP75 are NaN
    when 0.5 / 0.75 is not among the thresholds."""
    thr = _thresholds(iou_thresholds)
    scores, labels = np.asarray(scores, np.float64).reshape(-1), np.asarray(labels, np.int64).reshape(-1)
    matched, n_gt = np.asarray(matched, bool), np.asarray(n_gt, np.int64).reshape(-1)
    if matched.shape != (thr.size, scores.size) or labels.size != scores.size:
        raise ValueError(f"matched must be ({thr.size}, {scores.size}), got {matched.shape}; labels {labels.shape}")
    K = n_gt.size
    if class_names is None:
        class_names = [str(c) for c in range(K)]
    if len(class_names) != K:
        raise ValueError(f"{K} classes but {len(class_names)} class names")
    ap, ar = np.full((K, thr.size), np.nan), np.full((K, thr.size), np.nan)
    n_det = np.zeros(K, np.int64)
    for c in range(1, K):
        sel = labels == c
        n_det[c] = int(sel.sum())
        if n_gt[c] <= 0:
            continue
        for t in range(thr.size):
            ap[c, t], ar[c, t] = _ap_of(scores[sel], matched[t, sel], float(n_gt[c]))[:2]
    have = n_gt[1:] > 0

    def mean(a):                                                   # over the classes with ground truth (and thresholds)
        a = a[1:][have]
        return float(a.mean()) if a.size else float("nan")

    def at(a, v):
        k = np.flatnonzero(thr == np.float32(v))
        return a[:, k[0]] if len(k) else np.full(K, np.nan)

    ap50, ap75 = at(ap, 0.5), at(ap, 0.75)
    per = {str(class_names[c]): {"AP": float(ap[c].mean()), "AP50": float(ap50[c]), "AR": float(ar[c].mean()), "n_gt": int(n_gt[c]),
                                 "n_det": int(n_det[c])} for c in range(1, K)}
    return {"AP": mean(ap), "AP50": mean(ap50), "AP75": mean(ap75), "AR": mean(ar), "per_class": per}


class DetectionScorer:
    """Accumulates matches over batches and scores them: ``update(detections, targets)`` per batch, then ``summary()``.

    ``num_classes`` counts the background (6 for ``core.EVENT_CLASSES``).  With ``class_aware=False`` matching ignores the
    labels and everything is scored as one class named "all"."""

    def __init__(self, num_classes, iou_thresholds=None, kind="mask", class_aware=True, class_names=None):
        if isinstance(num_classes, (bool, np.bool_)) or not isinstance(num_classes, (int, np.integer)) or num_classes < 2:
            raise ValueError(f"num_classes must be an integer >= 2 (background included), got {num_classes!r}")
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
        self.num_classes, self.kind, self.class_aware = int(num_classes), kind, bool(class_aware)
        self.thresholds = _thresholds(iou_thresholds)
        if not self.class_aware:
            class_names = ("background", "all")
        elif class_names is None:
            class_names = [str(c) for c in range(self.num_classes)]
        if len(class_names) != (self.num_classes if self.class_aware else 2):
            raise ValueError(f"{self.num_classes} classes but {len(class_names)} class names")
        self.class_names = tuple(class_names)
        self.reset()

    def reset(self):
        self._scores, self._labels, self._matched = [], [], []
        self._n_gt = np.zeros(len(self.class_names), np.int64)
        self.images = 0

    def update(self, detections, targets, device=None):
        """Match one batch on the GPU and append one record per detection -> the ``InstanceMatch``."""
        m = match_instances(detections, targets, self.thresholds, self.kind, self.class_aware, device)
        det_match, scores, labels, counts, gt_labels, gt_counts = m.records()
        n, D = scores.shape
        valid = np.arange(D)[None, :] < np.clip(counts, 0, D)[:, None]
        gvalid = np.arange(gt_labels.shape[1])[None, :] < np.clip(gt_counts, 0, gt_labels.shape[1])[:, None]
        dl, gl = labels[valid], gt_labels[gvalid]
        if self.class_aware:
            for name, a in (("detections", dl), ("targets", gl)):
                if a.size and (a.min() < 1 or a.max() >= self.num_classes):
                    raise ValueError(f"{name}: labels must be in 1 .. {self.num_classes - 1}, got {int(a.min())} .. {int(a.max())}")
        else:
            dl, gl = np.ones_like(dl), np.ones_like(gl)
        self._scores.append(scores[valid].astype(np.float64))
        self._labels.append(dl.astype(np.int64))
        self._matched.append(np.stack([det_match[:, t][valid] >= 0 for t in range(self.thresholds.size)]) if n and D
                             else np.zeros((self.thresholds.size, 0), bool))
        self._n_gt += np.bincount(gl, minlength=len(self.class_names))
        self.images += n
        return m

    def _all(self):
        T = self.thresholds.size
        cat = lambda xs, empty: np.concatenate(xs, axis=-1) if xs else empty  # noqa: E731
        return (cat(self._scores, np.zeros(0)), cat(self._labels, np.zeros(0, np.int64)), cat(self._matched, np.zeros((T, 0), bool)))

    def summary(self):
        """-> ``scores_from_matches`` of everything seen so far."""
        scores, labels, matched = self._all()
        return scores_from_matches(scores, labels, matched, self._n_gt, self.thresholds, self.class_names)

    def pr_curve(self, cls, iou=0.5):
        """-> (precision, recall, score) of class ``cls`` (index or name) at threshold ``iou``, in descending score; the raw
        curve, before the envelope.  Recall is NaN for a class without ground truth."""
        c = self.class_names.index(cls) if isinstance(cls, str) else int(cls)
        if not 1 <= c < len(self.class_names):
            raise ValueError(f"cls must be one of {self.class_names[1:]} or its index, got {cls!r}")
        k = np.flatnonzero(self.thresholds == np.float32(iou))
        if not len(k):
            raise ValueError(f"iou must be one of {self.thresholds.tolist()}, got {iou!r}")
        scores, labels, matched = self._all()
        sel = labels == c
        with np.errstate(divide="ignore", invalid="ignore"):
            _, _, precision, recall, score = _ap_of(scores[sel], matched[k[0], sel], float(self._n_gt[c]) if self._n_gt[c] else np.nan)
        return precision, recall, score


def score_detections(detections, targets, num_classes=None, **kw):
    """One ``DetectionScorer.update`` followed by ``summary()``.  ``num_classes`` defaults to that of the targets
    (``InstanceTargets.num_classes``)."""
    if num_classes is None:
        num_classes = getattr(targets, "num_classes", None)
        if num_classes is None:
            raise ValueError("num_classes is needed when the targets are a list")
    device = kw.pop("device", None)
    s = DetectionScorer(num_classes, **kw)
    s.update(detections, targets, device=device)
    return s.summary()
