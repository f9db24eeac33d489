"""NumPy restatement of instance matching (include/rfi_hip.h, "instance matching"): mask IoU straight from the mask bytes
(no packing, so it checks the packed route independently), box IoU in float32 in the pinned order, the greedy matcher as
a plain double loop and the AP arithmetic of COCO's accumulate.  Everything works on the padded layout of the C ABI:
detections (n, D, ...), ground truths (n, G, ...), counts (n,); whatever lies behind a count is never looked at."""
import numpy as np

F32 = np.float32


def default_thresholds():
    return np.arange(50, 100, 5, dtype=np.float32) / np.float32(100)


# ---------------------------------------------------------------------------------------------- packing
def pack(masks):
    """uint8 (m, H, W) -> bits uint64 (m, H, ceil(W / 64)), area int32 (m,), extent int32 (m, 4)."""
    m, H, W = masks.shape
    wc = (W + 63) // 64
    on = np.zeros((m, H, wc * 64), bool)
    on[:, :, :W] = masks != 0
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    bits = (on.reshape(m, H, wc, 64).astype(np.uint64) * weights).sum(axis=3, dtype=np.uint64)
    area = on.sum(axis=(1, 2)).astype(np.int32)
    extent = np.zeros((m, 4), np.int32)
    for k in range(m):
        r, c = np.nonzero(bits[k])
        if len(r):
            extent[k] = (r.min(), c.min(), r.max() + 1, c.max() + 1)
    return bits, area, extent


# ---------------------------------------------------------------------------------------------- IoU
def mask_iou(det_masks, det_count, gt_masks, gt_count):
    """det_masks (n, D, H, W), gt_masks (n, G, H, W), any non-zero byte foreground -> inter int32, iou float32 (n, D, G)."""
    n, D = det_masks.shape[:2]
    G = gt_masks.shape[1]
    inter, iou = np.zeros((n, D, G), np.int32), np.zeros((n, D, G), np.float32)
    for i in range(n):
        nd, ng = min(int(det_count[i]), D), min(int(gt_count[i]), G)
        px = det_masks.shape[2] * det_masks.shape[3]
        a = (det_masks[i, :nd] != 0).reshape(nd, px).astype(np.int64)
        b = (gt_masks[i, :ng] != 0).reshape(ng, px).astype(np.int64)
        it = a @ b.T                                                  # pixels set in both, per pair
        un = a.sum(1)[:, None] + b.sum(1)[None, :] - it
        inter[i, :nd, :ng] = it
        with np.errstate(divide="ignore", invalid="ignore"):
            iou[i, :nd, :ng] = np.where(un == 0, 0.0, it.astype(np.float64) / un.astype(np.float64)).astype(np.float32)
    return inter, iou


def same(a, b):
    """Equality of nested dicts / arrays / floats in which NaN equals NaN."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=np.asarray(a).dtype.kind == "f")


def box_iou(det_boxes, det_count, gt_boxes, gt_count):
    """float32 throughout, one rounding per operation, in the order of the detector's iou_of."""
    n, D = det_boxes.shape[:2]
    G = gt_boxes.shape[1]
    iou = np.zeros((n, D, G), np.float32)
    with np.errstate(all="ignore"):
        for i in range(n):
            nd, ng = min(int(det_count[i]), D), min(int(gt_count[i]), G)
            a, b = det_boxes[i, :nd, None, :].astype(F32), gt_boxes[i, None, :ng, :].astype(F32)      # (float32 arrays: every
            ax1, ay1, ax2, ay2 = (a[..., k] for k in range(4))                                        # operation rounds once)
            bx1, by1, bx2, by2 = (b[..., k] for k in range(4))
            iw = np.maximum(np.minimum(ax2, bx2) - np.maximum(ax1, bx1), F32(0))
            ih = np.maximum(np.minimum(ay2, by2) - np.maximum(ay1, by1), F32(0))
            inter = iw * ih
            union = ((ax2 - ax1) * (ay2 - ay1) + (bx2 - bx1) * (by2 - by1)) - inter
            assert inter.dtype == F32 and union.dtype == F32
            iou[i, :nd, :ng] = np.where(union <= 0, F32(0), inter / union)
    return iou


# ---------------------------------------------------------------------------------------------- matching
def match(iou, scores, det_labels, det_count, gt_labels, gt_count, thresholds, class_aware=True):
    """-> det_match int32 (n, T, D), gt_match int32 (n, T, G)."""
    n, D, G = iou.shape
    thresholds = np.asarray(thresholds, np.float32)
    T = len(thresholds)
    det_match, gt_match = np.full((n, T, D), -1, np.int32), np.full((n, T, G), -1, np.int32)
    for i in range(n):
        nd, ng = min(int(det_count[i]), D), min(int(gt_count[i]), G)
        order = sorted(range(nd), key=lambda d: (-float(scores[i, d]), d))          # descending score, ties ascending slot
        for k, t in enumerate(thresholds):
            for d in order:
                best, best_v = -1, F32(-1)
                for g in range(ng):
                    if gt_match[i, k, g] >= 0:
                        continue
                    if class_aware and int(gt_labels[i, g]) != int(det_labels[i, d]):
                        continue
                    v = iou[i, d, g]
                    if v >= t and v > best_v:                                       # (strictly greater: ties stay with the lowest slot)
                        best, best_v = g, v
                if best >= 0:
                    det_match[i, k, d], gt_match[i, k, best] = best, d
    return det_match, gt_match


# ---------------------------------------------------------------------------------------------- AP
def average_precision(scores, matched, n_gt):
    """COCO's accumulate for one class and threshold -> (AP, recall reached).  scores (N,), matched (N,) bool, arrival order."""
    scores, matched = np.asarray(scores, np.float64), np.asarray(matched, bool)
    if n_gt == 0:
        return float("nan"), float("nan")
    order = np.argsort(-scores, kind="stable")
    tp = fp = 0
    recall, precision = [], []
    for j in order:
        tp, fp = tp + int(matched[j]), fp + int(not matched[j])
        recall.append(tp / n_gt)
        precision.append(tp / (tp + fp))
    for k in range(len(precision) - 2, -1, -1):
        precision[k] = max(precision[k], precision[k + 1])
    total = 0.0
    q = []
    for r in np.linspace(0.0, 1.0, 101):
        at = int(np.searchsorted(recall, r, side="left"))
        q.append(precision[at] if at < len(precision) else 0.0)
    total = float(np.mean(q))
    return total, (recall[-1] if recall else 0.0)


def summary(scores, labels, matched, n_gt, thresholds, class_names):
    """The dict ``evaluation.scores_from_matches`` returns, from the loops above."""
    thresholds = np.asarray(thresholds, np.float32)
    scores, labels, matched = np.asarray(scores, np.float64), np.asarray(labels, np.int64), np.asarray(matched, bool)
    K, T = len(n_gt), len(thresholds)
    ap, ar = np.full((K, T), np.nan), np.full((K, T), np.nan)
    for c in range(1, K):
        sel = labels == c
        for t in range(T):
            ap[c, t], ar[c, t] = average_precision(scores[sel], matched[t, sel], int(n_gt[c]))
    have = [c for c in range(1, K) if n_gt[c] > 0]
    mean = lambda a: float(np.mean(a[have])) if have else float("nan")  # noqa: E731

    def at(a, v):
        k = np.flatnonzero(thresholds == np.float32(v))
        return a[:, k[0]] if len(k) else np.full(K, np.nan)

    per = {str(class_names[c]): {"AP": float(np.mean(ap[c])), "AP50": float(at(ap, 0.5)[c]), "AR": float(np.mean(ar[c])),
                                 "n_gt": int(n_gt[c]), "n_det": int((labels == c).sum())} for c in range(1, K)}
    return {"AP": mean(ap), "AP50": mean(at(ap, 0.5)), "AP75": mean(at(ap, 0.75)), "AR": mean(ar), "per_class": per}


def score(det_lists, target_lists, num_classes, thresholds=None, kind="mask", class_aware=True, class_names=None):
    """``evaluation.score_detections`` for the list forms: detections [{"boxes", "scores", "labels", "masks"}], targets
    [{"boxes", "labels", "masks"}] -> the summary dict."""
    thresholds = default_thresholds() if thresholds is None else np.asarray(thresholds, np.float32)
    p = pad_lists(det_lists, target_lists)
    if kind == "mask":
        _, iou = mask_iou(p["det_masks"], p["det_count"], p["gt_masks"], p["gt_count"])
    else:
        iou = box_iou(p["det_boxes"], p["det_count"], p["gt_boxes"], p["gt_count"])
    dm, _ = match(iou, p["scores"], p["det_labels"], p["det_count"], p["gt_labels"], p["gt_count"], thresholds, class_aware)
    sc, lb, mt = [], [], []
    K = num_classes if class_aware else 2
    n_gt = np.zeros(K, np.int64)
    for i in range(len(det_lists)):
        for d in range(int(p["det_count"][i])):
            sc.append(float(p["scores"][i, d]))
            lb.append(int(p["det_labels"][i, d]) if class_aware else 1)
            mt.append([dm[i, t, d] >= 0 for t in range(len(thresholds))])
        for g in range(int(p["gt_count"][i])):
            n_gt[int(p["gt_labels"][i, g]) if class_aware else 1] += 1
    names = (class_names or [str(c) for c in range(K)]) if class_aware else ("background", "all")
    mt = np.asarray(mt, bool).reshape(len(sc), len(thresholds)).T
    return summary(sc, lb, mt, n_gt, thresholds, names)


def pad_lists(det_lists, target_lists):
    """Both list forms padded to the longest list of each side (masks too, where every item has them)."""
    n = len(det_lists)
    D = max([len(d["boxes"]) for d in det_lists], default=0)
    G = max([len(t["boxes"]) for t in target_lists], default=0)
    out = {"det_boxes": np.zeros((n, D, 4), np.float32), "scores": np.zeros((n, D), np.float32), "det_labels": np.zeros((n, D), np.int32),
           "det_count": np.zeros(n, np.int32), "gt_boxes": np.zeros((n, G, 4), np.float32), "gt_labels": np.zeros((n, G), np.int32),
           "gt_count": np.zeros(n, np.int32)}
    shape = None
    for x in list(det_lists) + list(target_lists):
        if x.get("masks") is not None:
            shape = tuple(np.asarray(x["masks"]).shape[1:])
    if shape is not None:
        out["det_masks"], out["gt_masks"] = np.zeros((n, D) + shape, np.uint8), np.zeros((n, G) + shape, np.uint8)
    for i, (d, t) in enumerate(zip(det_lists, target_lists)):
        k, g = len(d["boxes"]), len(t["boxes"])
        out["det_count"][i], out["gt_count"][i] = k, g
        out["det_boxes"][i, :k], out["scores"][i, :k], out["det_labels"][i, :k] = np.asarray(d["boxes"]).reshape(-1, 4), d["scores"], d["labels"]
        out["gt_boxes"][i, :g], out["gt_labels"][i, :g] = np.asarray(t["boxes"]).reshape(-1, 4), t["labels"]
        if shape is not None and d.get("masks") is not None and t.get("masks") is not None:
            out["det_masks"][i, :k] = np.asarray(d["masks"]) != 0
            out["gt_masks"][i, :g] = np.asarray(t["masks"]) != 0
    return out
