"""CPU-only: the case table of instance matching holds what it claims (shown with the NumPy restatement alone), the AP
arithmetic of ``evaluation.scores_from_matches`` on hand-worked cases and against the restatement, and every ValueError
``match_instances`` raises before a device call."""
import numpy as np
import pytest

import instance_match_cases as cases
import instance_match_ref as ref


@pytest.fixture(scope="module")
def table():
    c = cases.table()
    inter, iou = ref.mask_iou(c["det_masks"], c["det_count"], c["gt_masks"], c["gt_count"])
    thr = cases.TABLE_THRESHOLDS
    args = (iou, c["scores"], c["det_labels"], c["det_count"], c["gt_labels"], c["gt_count"], thr)
    return c, inter, iou, ref.match(*args, class_aware=True), ref.match(*args, class_aware=False)


def test_table_holds_what_it_claims(table):
    c, inter, iou, (dm, gm), (dm_any, gm_any) = table
    k25, k50, k75 = 0, 1, 2
    assert cases.TABLE_THRESHOLDS.tolist() == [0.25, 0.5, 0.75]
    # an IoU exactly equal to a threshold: 1 / 2 at t = 0.5, and it matches
    assert inter[0, 2, 2] == 1 and iou[0, 2, 2] == np.float32(0.5) and dm[0, k50, 2] == 2
    # two ground truths with equal IoU for one detection: the lowest slot
    assert iou[0, 3, 3] == iou[0, 3, 4] == np.float32(0.5) and dm[0, k50, 3] == 3 and gm[0, k50, 4] == -1
    # two detections with equal scores that want the same ground truth: the lower slot
    assert c["scores"][0, 2] == c["scores"][0, 6] and iou[0, 6, 2] == iou[0, 2, 2]
    assert gm[0, k50, 2] == 2 and dm[0, k50, 6] == -1
    # a detection whose best ground truth is taken falls to its second best
    assert iou[0, 1, 0] > iou[0, 1, 1] >= np.float32(0.25) and dm[0, k25, 0] == 0 and dm[0, k25, 1] == 1
    assert dm[0, k50, 1] == -1
    # matched at 0.5, unmatched at 0.75
    assert iou[0, 4, 5] == np.float32(3 / 5) and dm[0, k50, 4] == 5 and dm[0, k75, 4] == -1
    # a pair that matches only when class-agnostic
    assert iou[1, 0, 0] == 1 and c["det_labels"][1, 0] != c["gt_labels"][1, 0]
    assert dm[1, k50, 0] == -1 and gm[1, k50, 0] == -1 and dm_any[1, k50, 0] == 0 and gm_any[1, k50, 0] == 0
    # an empty detection mask and an empty truth mask: IoU 0 everywhere, 0 / 0 included
    assert not c["det_masks"][0, 5].any() and not c["gt_masks"][0, 6].any()
    assert not iou[0, 5].any() and not iou[0, :, 6].any() and (dm[0, :, 5] == -1).all() and (gm[0, :, 6] == -1).all()
    # identical masks
    assert np.array_equal(c["det_masks"][0, 0], c["gt_masks"][0, 0]) and iou[0, 0, 0] == 1 and (dm[0, :, 0] == 0).all()
    # an image without detections, one without truths
    assert c["det_count"][2] == 0 and c["gt_count"][2] == 2 and c["det_count"][3] == 2 and c["gt_count"][3] == 0
    assert (dm[2:] == -1).all() and (gm[2:] == -1).all() and not iou[2:].any()
    # mask bytes other than 0 or 1
    assert set(np.unique(c["det_masks"][1, 0])) == {0, 2} and set(np.unique(c["gt_masks"][1, 0])) == {0, 255}
    # garbage behind the counts, which would match if it were read
    D, G = c["det_masks"].shape[1], c["gt_masks"].shape[1]
    for i in range(4):
        nd, ng = int(c["det_count"][i]), int(c["gt_count"][i])
        assert nd < D and ng < G
        assert (c["det_masks"][i, nd:] == 255).all() and (c["gt_masks"][i, ng:] == 255).all() and (c["scores"][i, nd:] == 5).all()
        assert not iou[i, nd:].any() and not iou[i, :, ng:].any() and not inter[i, nd:].any()
        assert (dm[i, :, nd:] == -1).all() and (gm[i, :, ng:] == -1).all()
    # the table's mask extents reach the second word column
    bits, area, extent = ref.pack(c["gt_masks"][0])
    assert bits.shape == (G, 6, 2) and extent[2].tolist() == [3, 1, 4, 2] and area[2] == 2 and extent[6].tolist() == [0, 0, 0, 0]


def test_restatement_of_packing():
    m = np.zeros((2, 3, 70), np.uint8)
    m[0, 1, 0], m[0, 1, 63], m[0, 2, 64], m[0, 2, 69] = 1, 2, 255, 7
    bits, area, extent = ref.pack(m)
    assert bits.dtype == np.uint64 and bits[0, 1].tolist() == [1 | (1 << 63), 0] and bits[0, 2].tolist() == [0, 1 | (1 << 5)]
    assert area.tolist() == [4, 0] and extent.tolist() == [[1, 0, 3, 2], [0, 0, 0, 0]]


def test_box_iou_restatement_is_float32_in_the_pinned_order():
    a = np.asarray([[[0.1, 0.2, 10.3, 7.7]]], np.float32)
    b = np.asarray([[[3.3, 1.1, 12.9, 9.4], [20, 20, 30, 30], [5, 5, 5, 5]]], np.float32)
    got = ref.box_iou(a, [1], b, [3])
    f = np.float32
    iw, ih = f(f(10.3) - f(3.3)), f(f(7.7) - f(1.1))
    inter = f(iw * ih)
    union = f(f(f(f(f(10.3) - f(0.1)) * f(f(7.7) - f(0.2))) + f(f(f(12.9) - f(3.3)) * f(f(9.4) - f(1.1)))) - inter)
    assert got.dtype == np.float32 and got[0, 0, 0] == f(inter / union) and got[0, 0, 1] == 0 and got[0, 0, 2] == 0
    z = np.zeros((1, 1, 4), np.float32)
    assert ref.box_iou(z, [1], z, [1])[0, 0, 0] == 0                    # union 0 -> 0, not NaN


# ---------------------------------------------------------------------------------------------- AP
def _summary(scores, labels, matched, n_gt, thr=(0.5,), names=None):
    from rfi_toolbox_amd.evaluation import scores_from_matches
    matched = np.asarray(matched, bool).reshape(len(thr), -1)
    got = scores_from_matches(scores, labels, matched, n_gt, thr, names)
    want = ref.summary(scores, labels, matched, n_gt, thr, names or [str(c) for c in range(len(n_gt))])
    assert ref.same(got, want), (got, want)
    return got


def test_ap_hand_worked():
    assert _summary([0.9, 0.8, 0.7], [1, 1, 1], [1, 1, 1], [0, 3])["AP"] == 1.0               # all correct
    s = _summary([0.9, 0.8], [1, 1], [0, 1], [0, 1])                                           # FP then TP on one truth
    assert s["AP"] == 0.5 and s["AR"] == 1.0 and s["AP50"] == 0.5 and np.isnan(s["AP75"])
    s = _summary([0.9, 0.8, 0.7], [1, 1, 1], [1, 0, 1], [0, 2])                                # TP, FP, TP on two truths
    assert abs(s["AP"] - 253 / 303) < 1e-12 and s["AR"] == 1.0
    s = _summary([0.9], [1], [1], [0, 2])                                                      # half of the truths found
    assert abs(s["AP"] - 51 / 101) < 1e-12 and s["AR"] == 0.5
    s = _summary([], [], [], [0, 2])                                                           # truths, no detections
    assert s["AP"] == 0.0 and s["AR"] == 0.0


def test_ap_class_without_ground_truth_is_nan_and_excluded():
    s = _summary([0.9, 0.8, 0.7], [1, 2, 1], [1, 0, 1], [0, 2, 0], names=("bg", "a", "b"))
    assert s["per_class"]["a"]["AP"] == 1.0 and np.isnan(s["per_class"]["b"]["AP"]) and np.isnan(s["per_class"]["b"]["AR"])
    assert s["per_class"]["b"] == {**s["per_class"]["b"], "n_gt": 0, "n_det": 1}
    assert s["AP"] == 1.0 and s["AR"] == 1.0                        # the mean leaves class b out
    none = _summary([0.5], [1], [0], [0, 0])
    assert np.isnan(none["AP"]) and np.isnan(none["AR"])


def test_ap_over_thresholds_and_stable_order():
    thr = (0.5, 0.75)
    s = _summary([0.9, 0.8], [1, 1], [[1, 1], [0, 1]], [0, 2], thr)
    ap75 = 51 * 0.5 / 101                                        # [FP, TP] of two truths: precision 0.5 up to recall 0.5, 0 beyond
    assert s["AP50"] == 1.0 and abs(s["AP75"] - ap75) < 1e-12 and abs(s["AP"] - (1 + ap75) / 2) < 1e-12
    # equal scores keep their arrival order: [TP, FP] and [FP, TP] differ
    a = _summary([0.5, 0.5], [1, 1], [1, 0], [0, 1])["AP"]
    b = _summary([0.5, 0.5], [1, 1], [0, 1], [0, 1])["AP"]
    assert a == 1.0 and b == 0.5


def test_permuting_detection_slots_changes_nothing(table):
    """distinct scores: the match, hence the summary, does not depend on the slot order"""
    c = cases.random_case(5, 2, 9, 7, (6, 70))
    c["scores"] = (np.arange(18, dtype=np.float32).reshape(2, 9) + 1) / np.float32(32)         # distinct
    thr = ref.default_thresholds()

    def run(c):
        _, iou = ref.mask_iou(c["det_masks"], c["det_count"], c["gt_masks"], c["gt_count"])
        return ref.match(iou, c["scores"], c["det_labels"], c["det_count"], c["gt_labels"], c["gt_count"], thr)

    dm, gm = run(c)
    p = c.copy()
    for i in range(2):
        k = int(c["det_count"][i])
        perm = np.random.default_rng(i).permutation(k)
        for key in ("det_masks", "det_boxes", "scores", "det_labels"):
            p[key] = p[key].copy()
            p[key][i, :k] = c[key][i, :k][perm]
        dm2, gm2 = run(p)
        assert np.array_equal(dm2[i][:, :k], dm[i][:, :k][:, perm])
        back = np.where(gm2[i] >= 0, perm[np.clip(gm2[i], 0, max(k - 1, 0))] if k else -1, -1)
        assert np.array_equal(back, gm[i])
    d1, t1 = cases.lists_of(c)
    d2, t2 = cases.lists_of(p)
    assert ref.same(ref.score(d1, t1, 4), ref.score(d2, t2, 4))


def test_scorer_records_agree_with_the_restatement(table):
    """DetectionScorer's bookkeeping (records from det_match, counts per class) without a GPU: fed with the restatement's
    match through the same arrays ``update`` downloads."""
    from rfi_toolbox_amd.evaluation import scores_from_matches
    c = cases.random_case(8, 3, 12, 9, (6, 70))
    thr = ref.default_thresholds()
    dets, tgts = cases.lists_of(c)
    want = ref.score(dets, tgts, 4, thr)
    _, iou = ref.mask_iou(c["det_masks"], c["det_count"], c["gt_masks"], c["gt_count"])
    dm, _ = ref.match(iou, c["scores"], c["det_labels"], c["det_count"], c["gt_labels"], c["gt_count"], thr)
    valid = np.arange(12)[None] < c["det_count"][:, None]
    gvalid = np.arange(9)[None] < c["gt_count"][:, None]
    got = scores_from_matches(c["scores"][valid], c["det_labels"][valid], np.stack([dm[:, t][valid] >= 0 for t in range(10)]),
                              np.bincount(c["gt_labels"][gvalid], minlength=4), thr)
    assert ref.same(got, want)
    assert 0.0 < got["AP"] < 1.0 and got["per_class"]["1"]["n_det"] > 0


# ---------------------------------------------------------------------------------------------- argument checks
def test_value_errors_before_any_device_call(table):
    from rfi_toolbox_amd.components import InstanceTargets
    from rfi_toolbox_amd.evaluation import DetectionScorer, match_instances, score_detections
    c = table[0]
    dets, tgts = cases.lists_of(c)
    z = np.zeros(4, np.int32)
    no_masks = InstanceTargets(cases.TABLE_SHAPE, c["gt_boxes"], c["gt_labels"], c["gt_count"], z, z, np.zeros_like(c["gt_labels"]), None,
                               c["gt_count"], z, z)
    with pytest.raises(ValueError, match="instance_masks=False"):
        match_instances(dets, no_masks)
    with pytest.raises(ValueError, match="'masks'"):
        match_instances([{k: v for k, v in d.items() if k != "masks"} for d in dets], tgts)
    with pytest.raises(ValueError, match="planes"):
        match_instances(dets, [{**t, "masks": np.zeros((len(t["boxes"]), 6, 64), np.uint8)} for t in tgts])
    with pytest.raises(ValueError, match="images"):
        match_instances(dets[:3], tgts)
    for bad in ([0.0, 0.5], [0.5, 1.5], [np.nan], [np.inf], [-0.5], [], [[0.5]], np.linspace(0.1, 1, 33)):
        with pytest.raises(ValueError, match="iou_thresholds"):
            match_instances(dets, tgts, bad)
        with pytest.raises(ValueError, match="iou_thresholds"):
            DetectionScorer(4, bad)
    for bad in (np.nan, np.inf, -np.inf):
        d = [dict(x) for x in dets]
        d[0]["scores"] = d[0]["scores"].copy()
        d[0]["scores"][2] = bad
        with pytest.raises(ValueError, match="finite"):
            match_instances(d, tgts, kind="box")
    with pytest.raises(ValueError, match="kind"):
        match_instances(dets, tgts, kind="pixel")
    with pytest.raises(ValueError, match="at most 256"):
        match_instances([{"boxes": np.zeros((257, 4)), "scores": np.zeros(257), "labels": np.ones(257)}] * 4, tgts, kind="box")
    with pytest.raises(ValueError, match="num_classes"):
        score_detections(dets, tgts)
    with pytest.raises(ValueError):
        match_instances("detections", tgts)


def test_empty_inputs_need_no_device(table):
    from rfi_toolbox_amd.evaluation import DetectionScorer, match_instances
    m = match_instances([], []).numpy()
    assert m["iou"].shape == (0, 0, 0) and m["det_match"].shape == (0, 10, 0) and m["inter"].dtype == np.int32
    S = cases.TABLE_SHAPE
    none = {"boxes": np.zeros((0, 4), np.float32), "scores": np.zeros(0, np.float32), "labels": np.zeros(0, np.int64), "masks": np.zeros((0,) + S, bool)}
    two = {"boxes": np.asarray([[0, 0, 2, 2], [1, 1, 3, 3]], np.float32), "labels": np.asarray([1, 2]), "masks": np.ones((2,) + S, np.uint8)}
    m = match_instances([none, none], [two, two], [0.5, 0.75]).numpy()          # D = 0 everywhere
    assert m["iou"].shape == (2, 0, 2) and m["inter"].shape == (2, 0, 2) and m["det_match"].shape == (2, 2, 0)
    assert m["gt_match"].shape == (2, 2, 2) and (m["gt_match"] == -1).all()
    det = {**two, "scores": np.asarray([0.9, 0.8], np.float32)}
    no_gt = {"boxes": np.zeros((0, 4), np.float32), "labels": np.zeros(0, np.int64), "masks": np.zeros((0,) + S, np.uint8)}
    m = match_instances([det], [no_gt], kind="box")                               # G = 0 everywhere
    assert m.inter is None and m.numpy()["det_match"].shape == (1, 10, 2) and (m.numpy()["det_match"] == -1).all()
    s = DetectionScorer(3, class_names=("bg", "a", "b"))
    s.update([none, none], [two, two])
    s.update([det], [no_gt])
    out = s.summary()                                                             # two truths per class, two false alarms
    assert out["AP"] == 0.0 and out["AR"] == 0.0 and out["per_class"]["a"] == {"AP": 0.0, "AP50": 0.0, "AR": 0.0, "n_gt": 2, "n_det": 1}
    p, r, sc = s.pr_curve("a", 0.5)
    assert p.tolist() == [0.0] and r.tolist() == [0.0] and sc.tolist() == [np.float32(0.9)]
