"""CPU-only: the reference of the detector-inference ops (tests/detect_infer_ref.py) against ``_paste`` and the oracle's NMS,
and the case table of tests/test_gpu_detect_infer.py (tests/detect_infer_cases.py) against the reference's own decision
margins -- the GPU test compares discrete outputs exactly, so its inputs must be ones where a last-bit difference in a
score, an IoU or an interpolated mask value cannot flip a decision."""
import numpy as np
import pytest

import detect_infer_cases as cases
import detect_infer_ref as ref
from oracle import detection_ref


@pytest.mark.parametrize("k1, max_det, score_thresh", cases.SELECT_CASES)
def test_select_cases_are_decided(k1, max_det, score_thresh):
    r = cases.select_reference(k1, max_det, score_thresh)
    m = r["margins"]
    assert m["threshold"] >= 1e-4 and m["iou"] >= 1e-4 and m["min_size"] >= 1e-4, m
    assert m["score_gap"] >= 1e-6, m
    # the branches the GPU test is to reach
    assert m["suppressed"] > 50, m                                    # NMS really suppresses
    assert m["cand_ties"] >= 2 and m["ties_within_class"] >= 1, m     # bit-equal scores in a class's sort and in the selection
    assert m["ties_across_classes"] >= (1 if k1 > 2 else 0), m
    assert m["dropped_small"] >= 5 * (k1 - 1), m                      # sides < 1e-2 after clipping
    assert r["pcount"].tolist() == [100, 0, 37] and r["count"][1] == 0
    assert (r["count"] < max_det).any() and r["kept"][2] > 0          # an image where fewer than max_det survive ...
    if max_det == 20:
        assert r["kept"][0] > max_det and r["count"][0] == max_det    # ... and one where the selection cuts
    if score_thresh > 0:
        assert (r["cand_counts"].reshape(3, -1)[0] < 100 - 4).any()   # the score threshold drops rows
    assert len(set(r["level"][:r["count"][0]].tolist())) >= 2         # RoIs above level 0


def test_select_reference_is_predicts_rule():
    """The reference's NMS + selection against the oracle's NMS and predict's concatenate / stable argsort."""
    r = cases.select_reference(4, 20, 0.05)
    cb, cs, cc = r["cand_boxes"], r["cand_scores"], r["cand_counts"]
    for i in range(3):
        boxes, scores, labels = [], [], []
        for c in range(1, 4):
            s = i * 3 + c - 1
            b, sc = cb[s, :cc[s]], cs[s, :cc[s]]
            keep = detection_ref.nms(b, sc, cases.DET_NMS) if len(b) else np.zeros(0, np.int64)
            boxes.append(b[keep]); scores.append(sc[keep]); labels.append(np.full(len(keep), c))
        boxes, scores, labels = np.concatenate(boxes), np.concatenate(scores), np.concatenate(labels)
        top = np.argsort(-scores, kind="stable")[:20]
        k = r["count"][i]
        assert k == len(top)
        assert np.array_equal(r["boxes"][i, :k], boxes[top]) and np.array_equal(r["scores"][i, :k], scores[top])
        assert np.array_equal(r["labels"][i, :k], labels[top])
        assert not r["boxes"][i, k:].any() and not r["scores"][i, k:].any() and not r["labels"][i, k:].any()


def test_rois_from_boxes_reference():
    _, props, pcount = cases.select_inputs(2)
    rois, lvl = ref.rois_from_boxes(props, pcount, cases.THRESHOLDS)
    assert rois.shape == (300, 5) and (rois[:, 0] == np.repeat([0, 1, 2], 100)).all()
    assert not rois[100:200, 1:].any() and not rois[237:, 1:].any() and (lvl[100:200] == 0).all()
    assert np.array_equal(rois[:100, 1:], props[0]) and set(lvl[:100].tolist()) >= {0, 1, 2}


def test_paste_cases_are_decided():
    from rfi_toolbox_amd.models.mask_rcnn import _paste
    r = cases.paste_reference()
    assert [s[:2] for s in r["stats"]] == [(0, j) for j in range(7)]
    for (i, j, window, near), b in zip(r["stats"], cases.PASTE_BOXES):
        assert window > 0 and near <= 1e-3 * window, (j, window, near)      # (a zero-width box still has a one-pixel-wide window)
        pm = 1.0 / (1.0 + np.exp(-r["logits"][j]))
        assert np.array_equal(r["masks"][i, j], _paste(pm, b, cases.PH, cases.PW))
    win = [s[2] for s in r["stats"]]
    assert win[1] == cases.PH * cases.PW and win[4] == 28 and win[3] < 2 * 41 and win[5] == 6
    assert not r["masks"][0, 7].any() and not r["masks"][1].any() and not r["rfi_mask"][1].any()
    assert r["masks"][0, :7].any((1, 2)).all() and np.array_equal(r["rfi_mask"][0], r["masks"][0].any(0))
