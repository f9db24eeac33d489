"""NumPy restatement of the detector-inference ops (include/rfi_hip.h: rfi_op_detect_candidates, rfi_op_detect_select,
rfi_op_rois_from_boxes, rfi_op_mask_paste and the greedy NMS between the first two), written from what
``MaskRCNN.predict`` / ``_paste`` compute (rfi_toolbox_amd/models/mask_rcnn.py), not from the kernels:

* candidates: per image and foreground class c, prob = softmax(class logits)[c] in float32; class c's deltas decoded against
  the proposal (weights 1, dw / dh clamped at log(1000/16)), clipped to (H, W); rows with prob > score_thresh and both sides
  >= min_size, in stable descending score order (ties: ascending proposal index);
* nms: greedy, in that order, a box goes when a kept one overlaps it by IoU > thr;
* select: the class-major concatenation of the kept boxes, ``np.argsort(-scores, kind="stable")[:max_det]``;
* paste: ``_paste`` per instance, the union over an image's instances.

Every function also returns its decision margins -- how far the reference's own discrete decisions are from flipping -- so
that a test can keep to cases the reference is sure of (tests/test_detect_infer_host.py).
"""
import math

import numpy as np

CLAMP = np.float32(math.log(1000.0 / 16))


def decode(props, deltas, h, w):
    """float32 box decode (weights 1) + clip, the order of operations of the package's box coder."""
    a, d = np.asarray(props, np.float32).reshape(-1, 4), np.asarray(deltas, np.float32).reshape(-1, 4)
    half = np.float32(0.5)
    aw, ah = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    cx, cy = a[:, 0] + half * aw, a[:, 1] + half * ah
    pcx, pcy = d[:, 0] * aw + cx, d[:, 1] * ah + cy
    pw, ph = np.exp(np.minimum(d[:, 2], CLAMP)) * aw, np.exp(np.minimum(d[:, 3], CLAMP)) * ah
    b = np.stack([pcx - half * pw, pcy - half * ph, pcx + half * pw, pcy + half * ph], 1).astype(np.float32)
    b[:, 0::2] = np.clip(b[:, 0::2], 0, np.float32(w))
    b[:, 1::2] = np.clip(b[:, 1::2], 0, np.float32(h))
    return b


def _gap(sorted_scores):
    """Smallest gap between adjacent sorted scores that are not bit-equal (inf: none)."""
    s = np.asarray(sorted_scores, np.float64)
    g = np.abs(np.diff(s))
    g = g[g > 0]
    return float(g.min()) if len(g) else math.inf


def candidates(head, props, pcount, k1, h, w, score_thresh, min_size=1e-2):
    """head (images pmax, 5 k1), props (images, pmax, 4), pcount (images,) -> boxes (sets, pmax, 4), scores (sets, pmax)
    (-inf behind the count), counts (sets,), margins; set = image (k1 - 1) + c - 1."""
    props = np.asarray(props, np.float32)
    n, pmax, _ = props.shape
    head = np.asarray(head, np.float32).reshape(n, pmax, 5 * k1)
    boxes = np.zeros((n * (k1 - 1), pmax, 4), np.float32)
    scores = np.full((n * (k1 - 1), pmax), -np.inf, np.float32)
    counts = np.zeros(n * (k1 - 1), np.int32)
    m_thr, m_gap, m_size, small = math.inf, math.inf, math.inf, 0
    for i in range(n):
        cnt = int(min(max(pcount[i], 0), pmax))
        if not cnt:
            continue
        hd = head[i, :cnt]
        z = hd[:, :k1] - hd[:, :k1].max(1, keepdims=True)
        prob = (np.exp(z) / np.exp(z).sum(1, keepdims=True)).astype(np.float32)
        for c in range(1, k1):
            b = decode(props[i, :cnt], hd[:, k1 + 4 * c:k1 + 4 * c + 4], h, w)
            s = prob[:, c]
            bw, bh = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
            ok = (s > np.float32(score_thresh)) & (bw >= np.float32(min_size)) & (bh >= np.float32(min_size))
            m_thr = min(m_thr, float(np.abs(s.astype(np.float64) - score_thresh).min()))
            m_size = min(m_size, float(np.abs(np.minimum(bw, bh).astype(np.float64) - min_size).min()))
            small += int(((bw < np.float32(min_size)) | (bh < np.float32(min_size))).sum())
            idx = np.flatnonzero(ok)
            order = idx[np.argsort(-s[idx], kind="stable")]
            m_gap = min(m_gap, _gap(s[order]))
            st = i * (k1 - 1) + c - 1
            boxes[st, :len(order)], scores[st, :len(order)], counts[st] = b[order], s[order], len(order)
    return boxes, scores, counts, {"threshold": m_thr, "score_gap": m_gap, "min_size": m_size, "dropped_small": small}


def iou32(a, b):
    """float32 IoU of box a with boxes b (the quantities the device compares: inter > thr * union)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32).reshape(-1, 4)
    iw = np.maximum(np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]), np.float32(0))
    ih = np.maximum(np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]), np.float32(0))
    inter = iw * ih
    union = (a[2] - a[0]) * (a[3] - a[1]) + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - inter
    return inter, union


def nms_sets(boxes, counts, thr):
    """Greedy NMS of every set (boxes (sets, k, 4) in descending score order, counts valid rows) -> keep bool (sets, k),
    margins over the pairs the greedy scan actually compares (a kept box against every later box not yet removed)."""
    boxes = np.asarray(boxes, np.float32)
    keep = np.zeros(boxes.shape[:2], bool)
    m_iou = math.inf
    suppressed = 0
    for s in range(boxes.shape[0]):
        cnt = int(counts[s])
        gone = np.zeros(cnt, bool)
        for i in range(cnt):
            if gone[i]:
                continue
            keep[s, i] = True
            later = np.flatnonzero(~gone[i + 1:]) + i + 1
            if not len(later):
                continue
            inter, union = iou32(boxes[s, i], boxes[s, later])
            with np.errstate(divide="ignore", invalid="ignore"):
                iou = np.where(union > 0, inter.astype(np.float64) / union.astype(np.float64), 0.0)
            m_iou = min(m_iou, float(np.abs(iou - thr).min()))
            hit = inter > np.float32(thr) * union
            gone[later[hit]] = True
            suppressed += int(hit.sum())
    return keep, {"iou": m_iou, "suppressed": suppressed}


def levels(boxes, thresholds):
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    area = np.maximum((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]), np.float32(1e-6))
    t1, t2, t3 = (np.float32(t) for t in thresholds)
    return ((area >= t1).astype(np.int32) + (area >= t2) + (area >= t3)).astype(np.int32)


def select(boxes, scores, keep, images, max_det, thresholds):
    """Candidate sets (images classes, k, ..) + keep -> det_boxes (images, max_det, 4), det_scores, det_labels (int32),
    det_count, rois (images max_det, 5), level, margins."""
    boxes, scores, keep = np.asarray(boxes, np.float32), np.asarray(scores, np.float32), np.asarray(keep, bool)
    classes, k = boxes.shape[0] // images, boxes.shape[1]
    db, ds = np.zeros((images, max_det, 4), np.float32), np.zeros((images, max_det), np.float32)
    dl, dc = np.zeros((images, max_det), np.int32), np.zeros(images, np.int32)
    m_gap, ties_in, ties_across = math.inf, 0, 0
    for i in range(images):
        sl = slice(i * classes, (i + 1) * classes)
        kp = keep[sl].reshape(-1)
        fb, fs = boxes[sl].reshape(-1, 4)[kp], scores[sl].reshape(-1)[kp]
        fl = (np.repeat(np.arange(classes), k)[kp] + 1).astype(np.int32)
        top = np.argsort(-fs, kind="stable")
        m_gap = min(m_gap, _gap(fs[top]))
        eq = np.flatnonzero(np.diff(fs[top].view(np.uint32)) == 0)
        ties_in += int((fl[top][eq] == fl[top][eq + 1]).sum())
        ties_across += int((fl[top][eq] != fl[top][eq + 1]).sum())
        top = top[:max_det]
        dc[i] = len(top)
        db[i, :len(top)], ds[i, :len(top)], dl[i, :len(top)] = fb[top], fs[top], fl[top]
    rois = np.concatenate([np.repeat(np.arange(images, dtype=np.float32), max_det)[:, None], db.reshape(-1, 4)], 1)
    return db, ds, dl, dc, rois, levels(db, thresholds), {"score_gap": m_gap, "ties_within_class": ties_in,
                                                         "ties_across_classes": ties_across}


def rois_from_boxes(props, pcount, thresholds):
    props = np.asarray(props, np.float32).copy()
    n, pmax, _ = props.shape
    for i in range(n):
        props[i, int(min(max(pcount[i], 0), pmax)):] = 0
    rois = np.concatenate([np.repeat(np.arange(n, dtype=np.float32), pmax)[:, None], props.reshape(-1, 4)], 1)
    return rois, levels(props, thresholds)


def paste_values(prob, box, h, w):
    """``_paste`` up to the threshold: (window (ix1, iy1, ix2, iy2), interpolated values of the window) or (None, None)."""
    x1, y1, x2, y2 = [float(v) for v in box]
    ix1, iy1, ix2, iy2 = max(int(math.floor(x1)), 0), max(int(math.floor(y1)), 0), min(int(math.ceil(x2)), w), min(int(math.ceil(y2)), h)
    if ix2 <= ix1 or iy2 <= iy1:
        return None, None
    m = prob.shape[0]
    gx = (np.arange(ix1, ix2) + 0.5 - x1) / max(x2 - x1, 1e-6) * m - 0.5
    gy = (np.arange(iy1, iy2) + 0.5 - y1) / max(y2 - y1, 1e-6) * m - 0.5
    x0, y0 = np.clip(np.floor(gx).astype(int), 0, m - 1), np.clip(np.floor(gy).astype(int), 0, m - 1)
    x1i, y1i = np.clip(x0 + 1, 0, m - 1), np.clip(y0 + 1, 0, m - 1)
    fx, fy = np.clip(gx - x0, 0, 1)[None, :], np.clip(gy - y0, 0, 1)[:, None]
    v = (prob[y0][:, x0] * (1 - fx) + prob[y0][:, x1i] * fx) * (1 - fy) + (prob[y1i][:, x0] * (1 - fx) + prob[y1i][:, x1i] * fx) * fy
    return (ix1, iy1, ix2, iy2), v


def paste(logits, det_boxes, det_count, h, w, eps=1e-4):
    """logits (images max_det, 28, 28), det_boxes (images, max_det, 4), det_count -> masks bool (images, max_det, h, w),
    rfi_mask bool (images, h, w), unsure bool like masks (in-window pixels with |v - 0.5| <= eps), per-instance lists of
    (window pixels, unsure pixels)."""
    det_boxes = np.asarray(det_boxes, np.float32)
    n, md, _ = det_boxes.shape
    lg = np.asarray(logits, np.float32).reshape(n, md, 28, 28)
    pm = (np.float32(1.0) / (np.float32(1.0) + np.exp(-lg))).astype(np.float32)
    masks, unsure = np.zeros((n, md, h, w), bool), np.zeros((n, md, h, w), bool)
    stats = []
    for i in range(n):
        for j in range(int(det_count[i])):
            win, v = paste_values(pm[i, j], det_boxes[i, j], h, w)
            if win is None:
                stats.append((i, j, 0, 0))
                continue
            ix1, iy1, ix2, iy2 = win
            masks[i, j, iy1:iy2, ix1:ix2] = v > 0.5
            unsure[i, j, iy1:iy2, ix1:ix2] = np.abs(v - 0.5) <= eps
            stats.append((i, j, v.size, int((np.abs(v - 0.5) <= eps).sum())))
    return masks, masks.any(1), unsure, stats
