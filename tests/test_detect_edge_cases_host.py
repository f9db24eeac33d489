"""No GPU: pins the tables of tests/detect_edge_cases.py -- every property test_gpu_detect_edges.py relies on is asserted here
(the saturated logits' coverage, the exact smooth-L1 residuals, the exactness of every IoU of group C and what the oracle makes of
the ties, the equality of the float32 and float64 sample coordinates of the boundary RoIs, the clearance of every other sample,
the sizes that reach a second grid trip, the exact mask averages), and the float64 references are checked against independent
statements (detection_ref's loops, torch autograd)."""
import numpy as np
import pytest
import torch

import detect_edge_cases as D
from oracle import detection_ref

F32, F64, U24 = np.float32, np.float64, D.U24


# ------------------------------------------------------------------------------------------------------------ A
def test_case_ids_are_unique_and_cover_the_factors():
    for cases in (D.RPN_CASES, D.FRC_CASES, D.ROI_CASES, D.ML_CASES):
        assert len({c.id for c in cases}) == len(cases)
    assert {c.A for c in D.RPN_CASES} == {4, 12} and {c.K1 for c in D.FRC_CASES} == {2, 5, 6}
    assert {c.P * c.A for c in D.RPN_CASES} == {37 * 4, 37 * 12, 65601 * 4} and 65601 * 4 > 1024 * 256
    assert {c.R for c in D.FRC_CASES} == {1, 37, 262400} and 262400 > 1024 * 256
    assert all(c.K1 == 2 for c in D.FRC_CASES if c.R == 262400)
    assert {c.beta for c in D.RPN_CASES} == {c.beta for c in D.FRC_CASES} == {1.0 / 9, 0.125} and F32(0.125) == 0.125
    for A in (4, 12):
        assert {(c.logits, c.labels) for c in D.RPN_CASES if c.A == A and c.P == 37} == {(r, l) for r in D.RANGES for l in D.RPN_LABELS}
        assert {c.ns for c in D.RPN_CASES if c.A == A} >= set(D.NS)


@pytest.mark.parametrize("case", [c for c in D.RPN_CASES if c.ns == "count" or c.P > 37], ids=lambda c: c.id)
def test_rpn_inputs(case):
    head, lab, tg, ns, rows, want = D.rpn_inputs(case)
    n = case.P * case.A
    count = int((lab >= 0).sum())
    assert ns == {"zero": 0, "one": 1, "count": count, "count7": 7 * count}[case.ns] and 7 * count < 2 ** 24
    assert {"none": count == 0, "all_pos": (lab == 1).all(), "all_neg": (lab == 0).all(), "one_pos": (lab == 1).sum() == 1 and count == n,
            "random": min((lab == v).sum() for v in (-1, 0, 1)) > 0}[case.labels]
    if case.logits == "saturated":
        lo, hi, near, mx, finite = D.coverage(head[:, :case.A])
        assert lo >= 0.10 and hi >= 0.10 and near > 0 and mx == 80.0 and finite, (lo, hi, near, mx)
    # the float32 subtraction head - target gives exactly the crafted residuals
    d = head[:, case.A:].reshape(n, 4)
    assert np.array_equal((d[rows] - tg[rows]).astype(F32), want) and want.dtype == F32
    if len(rows) >= 3:
        assert set(D.residuals(case.beta).tolist()) <= set(want.ravel().tolist())
    b = F32(case.beta)
    assert list(D.residuals(case.beta)[:6]) == [b, -b, np.nextafter(b, F32(0)), -np.nextafter(b, F32(0)), np.nextafter(b, F32(1)), -np.nextafter(b, F32(1))]


@pytest.mark.parametrize("case", [c for c in D.FRC_CASES if c.beta == 0.125], ids=lambda c: c.id)
def test_fastrcnn_inputs(case):
    head, lab, tg, rows, want = D.frc_inputs(case)
    R, K1 = case.R, case.K1
    x, d = head[:, :K1].astype(F64), head[:, K1:].reshape(R, K1, 4)
    assert lab.min() >= 0 and lab.max() < K1
    assert {"all_bg": (lab == 0).all(), "all_fg": (lab > 0).all(), "one_fg": (lab > 0).sum() == 1,
            "random": R < 37 or len(set(lab)) == K1}[case.labels]
    assert np.array_equal((d[rows, lab[rows]] - tg[rows]).astype(F32), want)
    if case.logits == "saturated":
        own = x[np.arange(R), lab]
        others = np.where(np.arange(K1)[None, :] == lab[:, None], np.nan, x)
        largest, smallest = own > np.nanmax(others, 1), own < np.nanmin(others, 1) - 80.0
        assert largest[0::4].all() and smallest[1::4].all() and largest.any() and (R == 1 or smallest.any())
        if R * K1 >= 64:
            lo, hi, near, mx, finite = D.coverage(x)
            assert lo >= 0.10 and hi >= 0.10 and near > 0 and mx == 80.0 and finite, (lo, hi, near, mx)


def test_rpn_reference_against_the_oracle_and_its_restatement():
    """the closed form equals oracle/detection_ref.rpn_loss where that is well conditioned (default logits, the label count as the
    normaliser), and the float32 restatement stays within a few float32 steps of it everywhere"""
    worst = 0.0
    for case in D.RPN_CASES:
        if case.P > 37:
            continue
        head, lab, tg, ns, _, _ = D.rpn_inputs(case)
        (lo, lb, g), e_ref, dl = D.loss_figures(D.rpn_ref, head, lab, tg, case.A, case.beta, ns)
        assert np.isfinite(g).all() and e_ref <= 8 * U24 * max(np.abs(g).max(), 1e-30), case.id
        assert dl[0] <= D.loss_bound(lo) and dl[1] <= D.loss_bound(lb), case.id
        worst = max(worst, e_ref / (U24 * max(np.abs(g).max(), 1e-30)))
        if case.ns == "count" and case.logits == "default":
            o = detection_ref.rpn_loss(head, lab, tg, case.A, float(F32(case.beta)))
            assert abs(o[0] - lo) <= 1e-12 * max(1, lo) and abs(o[1] - lb) <= 1e-12 * max(1, lb)
            np.testing.assert_allclose(g, o[2], rtol=1e-11, atol=1e-14)
    assert worst > 0.25                                   # (a restatement that IS the reference would measure nothing)


def test_fastrcnn_reference_against_autograd():
    for case in D.FRC_CASES:
        if case.R != 37 or case.logits != "default":
            continue
        head, lab, tg, _, _ = D.frc_inputs(case)
        (lc, lb, g), e_ref, _ = D.loss_figures(D.frc_ref, head, lab, tg, case.beta)
        h = torch.tensor(head, dtype=torch.float64, requires_grad=True)
        K1, R = case.K1, case.R
        lab_t = torch.tensor(lab, dtype=torch.long)
        cls = torch.nn.functional.cross_entropy(h[:, :K1], lab_t, reduction="sum") / R
        own = h[:, K1:].reshape(R, K1, 4)[torch.arange(R), lab_t]
        e = (own - torch.tensor(tg, dtype=torch.float64))[lab_t > 0]
        beta = float(F32(case.beta))
        box = torch.where(e.abs() < beta, 0.5 * e * e / beta, e.abs() - 0.5 * beta).sum() / R
        (cls + box).backward()
        assert abs(cls.item() - lc) <= 1e-12 * max(1, lc) and abs(box.item() - lb) <= 1e-12 * max(1, lb), case.id
        np.testing.assert_allclose(g, h.grad.numpy(), rtol=1e-10, atol=1e-14)
        assert e_ref <= 8 * U24 * np.abs(g).max()


# ------------------------------------------------------------------------------------------------------------ B
def test_decode_table():
    d = D.decode_deltas()
    assert D.CLAMP == F32(np.log(1000.0 / 16)) and len(d) % len(D.DECODE_ANCHORS) == 0
    for v in (D.CLAMP, np.nextafter(D.CLAMP, F32(9)), np.nextafter(D.CLAMP, F32(0)), F32(9), F32(-80), F32(0)):
        assert (d[:, 2] == v).any() and (d[:, 3] == v).any()
    assert (d == 0).all(1).sum() == len(D.DECODE_ANCHORS)
    b = detection_ref.decode_boxes(D.DECODE_ANCHORS, d)
    H, W = D.CLIP
    assert (b[:, 2] < 0).any() and (b[:, 0] > W).any() and (b[:, 3] < 0).any() and (b[:, 1] > H).any()       # wholly outside, each side
    assert (np.exp(np.minimum(d[:, 2].astype(F64), 5)) * 160 < 1e-30).any()                                  # width 0
    for clip in (None, D.CLIP):
        e = np.abs(D.decode32(D.DECODE_ANCHORS, d, clip) - detection_ref.decode_boxes(D.DECODE_ANCHORS, d, clip)) / D.decode_steps(D.DECODE_ANCHORS, d)
        assert e.max() <= 4.0
    assert D.DECODE_LARGE > 4096 * 256 + 64 * 3 and D.DECODE_LARGE % len(D.DECODE_ANCHORS) == 0
    rows = D.DECODE_LARGE_ROWS
    assert (rows < 4096 * 256).sum() == 64 and (rows >= 4096 * 256).sum() == 64 and rows.max() < D.DECODE_LARGE


def test_roundtrip_boxes_match_one_to_one():
    a, g = D.roundtrip_boxes()
    lab, matched, t = detection_ref.anchor_match(a, g, 0.7, 0.3, True)
    assert (lab == 1).all() and np.array_equal(matched, np.arange(len(a)))
    e = np.abs(D.decode32(a, D.encode32(a, g)) - g.astype(F64)) / D.decode_steps(a, t)
    assert e.max() <= 4.0
    np.testing.assert_allclose(detection_ref.decode_boxes(a, t), g.astype(F64), rtol=0, atol=1e-9)          # the float64 round trip is exact


# ------------------------------------------------------------------------------------------------------------ C
def test_every_iou_of_the_tie_cases_is_exact_or_clear():
    anchors, ac, gt, gc, names = D.match_batch()
    on_total = 0
    for i, k in enumerate(names):
        ok, on, none = D.iou_exactness(anchors[i], gt[i])                      # (the rows behind the counts included)
        assert ok, k
        on_total += on
        assert (none > 0) == k.startswith("zero_area"), k
    assert on_total >= 8
    ok, on, none = D.iou_exactness(D.match_large_anchors(), np.asarray(D.MATCH_LARGE_GT))
    assert ok and on >= 6 and none > 0 and D.MATCH_LARGE_N > 256 * 256
    for thr in D.THRESHOLDS:
        for n in D.NMS_SIZES:
            b = D.nms_boxes(n, thr)
            ok, on, none = D.iou_exactness(b, b)
            assert ok and (n < 8 or on >= 2), (n, thr)
        sets, counts = D.nms_batched_sets(thr)
        assert sets.shape == (40, 256, 4) and set(counts) == {0, 1, 255, 256}
        assert all(D.iou_exactness(s, s)[0] for s in sets[:8])
    assert {hi for hi, _, _ in D.MATCH_SETTINGS} | {lo for _, lo, _ in D.MATCH_SETTINGS} <= set(D.THRESHOLDS)


def _match(name, hi, lo, lq):
    g, a = D.MATCH_IMAGES[name]
    return D.ref_anchor_match(np.asarray(a, F32), np.asarray(g, F32).reshape(-1, 4), hi, lo, lq)


def test_what_the_matcher_makes_of_the_ties():
    lab, mi, _ = _match("thresholds", 0.75, 0.25, False)
    assert list(lab) == [1, -1, -1, -1, 0, 0] and list(mi) == [0, -1, -1, -1, -1, -1]      # IoU == hi: 1; IoU == lo: -1
    assert list(_match("thresholds", 0.5, 0.25, False)[0]) == [1, 1, -1, 1, 0, 0]
    assert list(_match("thresholds", 0.75, 0.5, False)[0]) == [1, -1, 0, -1, 0, 0]
    lab, mi, _ = _match("identical_gts", 0.75, 0.25, True)
    assert list(lab) == [1, 1, -1, -1] and list(mi) == [0, 0, -1, -1]                      # the first of two identical boxes wins
    lab, mi, _ = _match("tied_anchor", 0.75, 0.25, False)
    assert lab[0] == 1 and mi[0] == 0 and mi[1] == 1 and mi[2] == -1                       # 0.75 with both: the first
    lab, mi, t = _match("low_quality_three", 0.75, 0.25, True)
    assert list(lab) == [1, 1, 1, 1, 0] and list(mi) == [0, 0, 0, 1, -1]                   # all three attain the best IoU 2/16
    assert list(_match("low_quality_three", 0.75, 0.25, False)[0]) == [0, 0, 0, 1, 0]
    lab, mi, _ = _match("lonely_gt", 0.75, 0.25, True)
    assert list(lab) == [1, -1, 0] and (mi != 0).all()                                     # a ground truth nothing overlaps: no positives
    lab, mi, t = _match("no_gt", 0.75, 0.25, True)
    assert (lab == 0).all() and (mi == -1).all() and (t == 0).all()
    for lq in (True, False):
        lab, mi, t = _match("zero_area", 0.75, 0.25, lq)
        assert list(lab) == [0, 0, 1, 0, -1, 0] and list(mi) == [-1, -1, 1, -1, -1, -1] and (t[[0, 1, 3]] == 0).all()
        lab, mi, t = _match("zero_area_only", 0.75, 0.25, lq)
        assert (lab == 0).all() and (mi == -1).all() and (t == 0).all() and np.isfinite(t).all()


def test_what_greedy_nms_makes_of_the_ties():
    for thr in D.THRESHOLDS:
        keep = set(D.ref_nms(D.nms_boxes(8, thr), thr).tolist())
        assert keep == {0, 1, 2, 4, 5, 7}                 # on thr: kept; b goes, so c stays; the second identical box goes; zero area stays
        for n in (129, 2000):
            b, keep = D.nms_boxes(n, thr), set(D.ref_nms(D.nms_boxes(n, thr), thr).tolist())
            for w in (64, 128):
                assert {i for i in (w - 1, w, w - 2, w + 2, w - 3, w - 4) if i < n} <= keep and not {w + 1, w + 3} & keep, (n, thr, w)
            assert n < 2000 or 0.2 < len(keep) / n < 0.98          # (the dense set: suppression is the rule, not the exception)


# ------------------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("case", D.ROI_CASES + [D.ROI_FWD_TRIP, D.ROI_BWD_TRIP], ids=lambda c: c.id)
def test_roi_case_samples(case):
    x, rois, dout = D.roi_inputs(case)
    a = (case.scale, case.PH, case.PW, case.sr, case.aligned)
    assert (np.diff(rois[:, 0]) >= 0).all() and np.log2(case.scale) == round(np.log2(case.scale))
    if case.kind == "boundary":
        _, pts = D.boundary_rois(case.H, case.W, case.scale, case.aligned)
        s32, s64 = D.roi_samples(rois, *a, F32), D.roi_samples(rois, *a, F64)
        for (_, y32, x32), (_, y64, x64), (py, px) in zip(s32, s64, pts):
            assert y32.shape == (1, 1) and y32[0, 0] == y64[0, 0] == py and x32[0, 0] == x64[0, 0] == px
        for L, col in ((case.H, 0), (case.W, 1)):
            assert set(D.edge_values(L)) <= set(pts[:, col])
            assert {-1.0, 0.0, L - 1.0, float(L)} <= set(D.edge_values(L)) and min(D.edge_values(L)) < -1 and max(D.edge_values(L)) > L
    else:
        assert D.samples_clear(rois, *a, case.H, case.W)
    if case.kind == "adaptive":
        assert all(y.shape[1] * x.shape[1] >= 9 for _, y, x in D.roi_samples(rois, *a, F32))
    if case.kind == "zero_size":
        w, h = rois[:, 3] - rois[:, 1], rois[:, 4] - rois[:, 2]
        assert ((w == 0) & (h > 0)).any() and ((h == 0) & (w > 0)).any() and ((w == 0) & (h == 0)).any() and ((w == 0) | (h == 0)).all()
        out = D.roi_align_np(x, rois, case.scale, (case.PH, case.PW), case.sr, True, F64)
        assert (np.abs(out).reshape(len(rois), -1).max(1) > 0).all()       # the forward samples every one of them
    if case.counts is not None:
        assert [int((rois[:, 0] == n).sum()) for n in range(case.N)] == list(case.counts)
    if case.kind == "counts":
        assert sorted(case.counts) == [0, 1, 128, 129, 300] and 0 in (case.counts[0], case.counts[-1])
    if case.kind == "shapes":
        _, y, xs = zip(*D.roi_samples(rois, *a, F64))
        inside = [((v >= -1) & (v <= L)).any() for v, L in zip(y, [case.H] * len(y))]
        assert not all(inside) and any(inside)


@pytest.mark.parametrize("case", D.ROI_CASES, ids=lambda c: c.id)
def test_roi_restatement_against_the_loops(case):
    x, rois, dout = D.roi_inputs(case)
    a = (case.scale, (case.PH, case.PW), case.sr, case.aligned)
    want = detection_ref.roi_align(x, rois, *a)
    got = D.roi_align_np(x, rois, *a, f=F64)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * max(1.0, np.abs(want).max()))
    wantb = detection_ref.roi_align_backward(dout, x.shape, rois, *a)
    gotb = D.roi_align_bwd_np(dout, x.shape, rois, case.scale, case.sr, case.aligned, F64)
    np.testing.assert_allclose(gotb, wantb, rtol=0, atol=1e-12 * max(1.0, np.abs(wantb).max()))
    lhs, rhs = float((want * dout).sum()), float((x.astype(F64) * wantb).sum())                  # the backward is the adjoint
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, np.abs(want * dout).sum())
    e = np.abs(D.roi_align_np(x, rois, *a, f=F32) - want).max()                                  # (a coordinate near L carries 2^-24 L)
    assert e <= 4 * U24 * max(case.H, case.W) * np.abs(x).max()


def test_grid_trip_sizes():
    c = D.ROI_FWD_TRIP
    per_row = c.PH * c.PW * c.C // 4
    assert sum(c.counts) * per_row > 8192 * 256 and all(r * per_row >= 8192 * 256 for r in D.ROI_FWD_TRIP_ROWS[-2:])
    assert D.ROI_FWD_TRIP_ROWS[0] == 0 and max(D.ROI_FWD_TRIP_ROWS) == sum(c.counts) - 1
    c = D.ROI_BWD_TRIP
    assert c.H * c.W * c.C // 4 > 4096 * 256 and (c.H, c.W, c.C) == (128, 132, 256) and sum(c.counts) == 20
    _, rois, _ = D.roi_inputs(c)
    last = (4096 * 256) // (c.C // 4) // c.W                                     # the first map row of the second trip
    assert (rois[:, 4] * c.scale > last + 1).any()


@pytest.mark.parametrize("case", D.ML_CASES, ids=lambda c: c.id)
def test_ml_case(case):
    feats, rois, lv, start, dout = D.ml_inputs(case)
    R = len(rois)
    assert list(np.diff(start)) == list(case.counts) and start[-1] == R and (np.diff(rois[:, 0]) >= 0).all()
    assert case.C % 4 == 0 and case.C <= 1024 and (case.C <= 8 or R <= 24) and lv.min() >= 0 and lv.max() <= 3
    for k in range(4):
        idx = np.flatnonzero(lv == k)
        h, w = feats[k].shape[1:3]
        assert (h, w) == (case.H0 >> k, case.W0 >> k) and D.samples_clear(rois[idx], D.ML_SCALE0 / (1 << k), case.P, case.P, case.sr, False, h, w)
    if case.levels == "mixed" and R >= 4:
        assert len(set(lv)) == 4
    if case.levels != "mixed":
        assert (lv == case.levels).all()
    if "level3_1x2" in case.id:
        assert feats[3].shape[1:3] == (1, 2) and (lv == 3).any()
    if case.id.endswith("trip"):
        assert case.H0 * case.W0 > 1024 * 4 and (rois[:, 4] * D.ML_SCALE0 > 4096 // case.W0 + 1).all()


def test_ml_cases_cover_the_lane_groups_and_counts():
    assert {c.C for c in D.ML_CASES} == {4, 8, 260, 1024}
    assert any(c.H0 != c.W0 for c in D.ML_CASES) and any(0 in c.counts for c in D.ML_CASES)
    assert sum(sorted(c.counts) == [0, 1, 128, 129, 300] and c.C == 8 for c in D.ML_CASES) == 2


# ------------------------------------------------------------------------------------------------------------ E
def test_mask_averages_are_exact_and_reach_the_threshold():
    m = D.mask_inputs()
    assert set(np.unique(m)) == {0, 1}
    rois = D.mask_exact_rois()
    assert np.array_equal(rois, np.round(rois)) and {float(v) for v in (rois[:, 3] - rois[:, 1]) / 4} == {1.0, 2.0}
    v = D.mask_averages(m, rois, 4)
    assert np.array_equal(v * 64, np.round(v * 64))                              # multiples of 1/64: exact in float32
    for q in (0.25, 0.5, 0.75):
        assert (v == q).sum() >= 3, q
    assert 0.2 < (v >= 0.5).mean() < 0.8


def test_random_mask_rois_stay_off_the_threshold():
    v = D.mask_averages(D.mask_inputs(), D.mask_random_rois(), 14)
    assert np.abs(v - 0.5).min() > 2.0 ** -20 and 0.1 < (v >= 0.5).mean() < 0.9
