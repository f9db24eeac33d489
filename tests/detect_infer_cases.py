"""The inputs of the detector-inference kernel tests (tests/test_gpu_detect_infer.py), built here so that
tests/test_detect_infer_host.py can check on the CPU that the reference (tests/detect_infer_ref.py) is sure of every discrete
decision in them: the seeds below were picked with that check, not by eye."""
import functools

import numpy as np

import detect_infer_ref as ref

# ---------------------------------------------------------------- candidates + NMS + select
H, W = 128, 192
PMAX, PCOUNT = 100, (100, 0, 37)
DET_NMS = 0.5
THRESHOLDS = tuple(float(np.float32(c * 96.0) ** 2) for c in (0.5, 1.0, 2.0))      # MaskRCNN._level_thresholds(max(H, W))
SEEDS = {2: 11, 4: 8}                                                                  # per k1
SELECT_CASES = [(k1, md, thr) for k1 in (2, 4) for md in (20, 100) for thr in (0.05, 0.0)]

_BASE = np.asarray([[8, 6, 40, 30], [50, 10, 110, 70], [120, 4, 186, 60], [4, 60, 60, 124], [70, 70, 100, 120], [110, 66, 188, 126],
                    [20, 20, 170, 110], [90, 30, 130, 50], [140, 80, 160, 100], [30, 90, 50, 110], [0, 0, 192, 128], [150, 20, 180, 44]],
                   np.float32)


def select_inputs(k1, seed=None):
    """head (3 PMAX, 5 k1), props (3, PMAX, 4), pcount: jittered copies of 12 base boxes (NMS has work), class logits N(0, 1.5),
    deltas N(0, 0.1), plus
    * rows 10 -> 11 and 20 -> 21 of image 0 duplicated exactly (bit-equal scores in a class's sort; NMS drops the copy),
    * rows 30, 31 of image 0: the same logits on two far-apart boxes, scores above every other (a tie within a class that
      survives NMS into the selection), and for k1 > 2 with equal logits and deltas for classes 1 and 2 (a tie across classes),
    * rows 40 .. 43 of image 0 and 5 of image 2: deltas that push the box out of the frame, sides 0 after clipping,
    * garbage behind pcount (must not influence anything)."""
    rng = np.random.default_rng(SEEDS[k1] if seed is None else seed)
    props = np.zeros((3, PMAX, 4), np.float32)
    for i in range(3):
        base = _BASE[rng.integers(0, len(_BASE), PMAX)]
        props[i] = base + rng.uniform(-3, 3, (PMAX, 4)).astype(np.float32)
    props[..., 0::2] = np.clip(props[..., 0::2], 0, W)
    props[..., 1::2] = np.clip(props[..., 1::2], 0, H)
    head = np.zeros((3, PMAX, 5 * k1), np.float32)
    head[..., :k1] = rng.normal(0, 1.5, (3, PMAX, k1))
    head[..., k1:] = rng.normal(0, 0.1, (3, PMAX, 4 * k1))
    for a, b in ((10, 11), (20, 21)):
        props[0, b], head[0, b] = props[0, a], head[0, a]
    props[0, 30], props[0, 31] = (10.25, 70.5, 44.75, 118.0), (130.5, 8.25, 181.0, 52.5)
    head[0, 30, :k1] = [-3.0] + [4.0] * (k1 - 1)
    if k1 > 2:
        head[0, 30, k1 + 8:k1 + 12] = head[0, 30, k1 + 4:k1 + 8]
    head[0, 31] = head[0, 30]
    for i, r in ((0, 40), (0, 41), (0, 42), (0, 43), (2, 5)):
        head[i, r, k1 + 4::4] = 9.0                   # dx = 9 widths to the right of every class: x1 = x2 = W
    pcount = np.asarray(PCOUNT, np.int32)
    for i in range(3):                                # behind the count: values that would win everything if they were read
        props[i, pcount[i]:] = (1.0, 1.0, 150.0, 120.0)
        head[i, pcount[i]:, 1:k1] = 50.0
    return head.reshape(3 * PMAX, 5 * k1), props, pcount


@functools.lru_cache(maxsize=None)
def select_reference(k1, max_det, score_thresh, seed=None):
    """The reference's candidates, keep bytes and selection for one case, computed once, with every margin."""
    head, props, pcount = select_inputs(k1, seed)
    cb, cs, cc, m_c = ref.candidates(head, props, pcount, k1, H, W, score_thresh)
    keep, m_n = ref.nms_sets(cb, cc, DET_NMS)
    db, ds, dl, dc, rois, lvl, m_s = ref.select(cb, cs, keep, 3, max_det, THRESHOLDS)
    kept = keep.reshape(3, -1).sum(1)
    return {"head": head, "props": props, "pcount": pcount, "cand_boxes": cb, "cand_scores": cs, "cand_counts": cc, "keep": keep,
            "boxes": db, "scores": ds, "labels": dl, "count": dc, "rois": rois, "level": lvl, "kept": kept,
            "margins": {"threshold": m_c["threshold"], "min_size": m_c["min_size"], "iou": m_n["iou"],
                        "score_gap": min(m_c["score_gap"], m_s["score_gap"]), "suppressed": m_n["suppressed"],
                        "ties_within_class": m_s["ties_within_class"], "ties_across_classes": m_s["ties_across_classes"],
                        "cand_ties": int(sum((np.diff(cs[s, :cc[s]].view(np.uint32)) == 0).sum() for s in range(len(cc)))),
                        "dropped_small": m_c["dropped_small"]}}


# ---------------------------------------------------------------- paste
PH, PW, PDET, PASTE_COUNT, PASTE_SEED = 64, 96, 8, (7, 0), 1
PASTE_BOXES = np.asarray([[10.3, 7.6, 41.2, 33.9],          # interior, fractional
                          [0.0, 0.0, 96.0, 64.0],           # the whole image
                          [70.4, 40.2, 99.3, 66.8],         # past the far corner: the window is clipped
                          [20.2, 10.5, 20.7, 50.5],         # narrower than one pixel
                          [33.5, 12.25, 33.5, 40.0],        # zero width
                          [0.0, 0.0, 2.5, 1.75],            # tiny, at the origin
                          [3.7, 2.2, 90.1, 61.6],           # large, fractional
                          [5.0, 5.0, 60.0, 60.0]], np.float32)      # slot 7 >= det_count: must stay empty


@functools.lru_cache(maxsize=None)
def paste_reference(seed=None):
    rng = np.random.default_rng(PASTE_SEED if seed is None else seed)
    logits = rng.normal(0, 3, (2 * PDET, 28, 28)).astype(np.float32)
    boxes = np.stack([PASTE_BOXES, PASTE_BOXES])              # image 1 has count 0: its boxes must not be read as instances
    count = np.asarray(PASTE_COUNT, np.int32)
    masks, union, unsure, stats = ref.paste(logits, boxes, count, PH, PW)
    return {"logits": logits, "boxes": boxes, "count": count, "masks": masks, "rfi_mask": union, "unsure": unsure, "stats": stats}
