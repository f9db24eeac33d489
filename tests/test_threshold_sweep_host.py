"""CPU-only: everything of evaluation/sweep.py that runs on the host -- the metric curves, best cut, average precision
and ROC AUC of a ThresholdSweep (driven by the counts of tests/threshold_sweep_ref.py) and the argument handling of
threshold_sweep that precedes the device call."""
import numpy as np
import pytest
from sklearn.metrics import average_precision_score, roc_auc_score

import threshold_sweep_ref as ref
from rfi_toolbox_amd.evaluation import ThresholdSweep, default_thresholds, sweep_from_counts, threshold_sweep
from rfi_toolbox_amd.evaluation.metrics import _dice, _f1, _iou, _precision, _recall
from rfi_toolbox_amd.evaluation.sweep import prepare_thresholds

SCALAR = {"iou": _iou, "precision": _precision, "recall": _recall, "f1": _f1, "dice": _dice}


def _sweep(p, t, thr, group_elems=None, group_shape=None):
    c = ref.sweep_counts(p, t, thr, group_elems)
    n_groups = c.shape[0]
    shape = () if group_elems is None else (group_shape or (n_groups,))
    return sweep_from_counts(thr, c.reshape(shape + c.shape[1:]), np.full(shape, p.size // n_groups, np.int64))


def _check_metrics(sw):
    m = sw.metrics()
    assert set(m) == set(SCALAR)
    for name, f in SCALAR.items():
        assert m[name].dtype == np.float64 and m[name].shape == sw.tp.shape
        for idx in np.ndindex(sw.tp.shape):
            want = f(int(sw.tp[idx]), int(sw.fp[idx]), int(sw.fn[idx]))
            assert m[name][idx] == want, (name, idx)


def test_metrics_equal_the_scalar_rules():
    thr = ref.thresholds(65)
    p, t = ref.scores(4097, thr, 1), ref.truth(4097, np.uint8, 1)
    sw = _sweep(p, t, thr)
    assert sw.tp.shape == (65,) and sw.tp.dtype == np.int64 and sw.group_shape == ()
    _check_metrics(sw)


def test_metrics_edge_cases():
    thr = np.array([0.25, 0.75], np.float32)
    zeros, ones = np.zeros(8, np.float32), np.ones(8, np.uint8)
    # nothing flagged, nothing true: every metric 1 except f1's own rule
    sw = _sweep(zeros, np.zeros(8, np.uint8), thr)
    assert sw.tp.tolist() == [0, 0] and sw.fp.tolist() == [0, 0] and sw.fn.tolist() == [0, 0]
    _check_metrics(sw)
    assert sw.metrics()["precision"].tolist() == [1.0, 1.0] and sw.metrics()["iou"].tolist() == [1.0, 1.0]
    # nothing flagged on a non-empty truth: precision 0, recall 0, f1 0
    sw = _sweep(zeros, ones, thr)
    _check_metrics(sw)
    assert sw.metrics()["precision"].tolist() == [0.0, 0.0] and sw.metrics()["f1"].tolist() == [0.0, 0.0]
    # everything flagged at the lower cut on an empty truth: recall 1 by rule, precision 0
    sw = _sweep(np.full(8, 0.5, np.float32), np.zeros(8, np.uint8), thr)
    _check_metrics(sw)
    assert sw.metrics()["recall"].tolist() == [1.0, 1.0] and sw.metrics()["precision"].tolist() == [0.0, 1.0]


def test_grouped_shapes_and_pooled():
    thr = ref.thresholds(7)
    p, t = ref.scores(2 * 3 * 35, thr, 2), ref.truth(2 * 3 * 35, np.float32, 2)
    sw = _sweep(p, t, thr, 35, (2, 3))
    assert sw.tp.shape == (2, 3, 7) and sw.count.shape == (2, 3) and sw.group_shape == (2, 3)
    _check_metrics(sw)
    pooled, whole = sw.pooled(), _sweep(p, t, thr)
    for a in ("tp", "fp", "fn"):
        assert np.array_equal(getattr(pooled, a), getattr(whole, a))
    assert int(pooled.count) == p.size and pooled.group_shape == ()
    thr_b, val_b = sw.best("iou")
    assert thr_b.shape == (2, 3) and val_b.shape == (2, 3)
    for idx in np.ndindex(2, 3):
        one = ThresholdSweep(thr, sw.tp[idx], sw.fp[idx], sw.fn[idx], sw.count[idx])
        assert one.best("iou") == (float(thr_b[idx]), float(val_b[idx]))
    assert sw.average_precision().shape == (2, 3) and sw.roc_auc().shape == (2, 3)


def test_best_breaks_ties_towards_the_lowest_threshold():
    # f1 curve with a flat maximum at 0.4 and 0.6, thresholds given unsorted with a duplicate
    thr = np.array([0.8, 0.6, 0.2, 0.4, 0.6], np.float32)
    counts = np.array([[2, 0, 6], [6, 2, 2], [8, 8, 0], [6, 2, 2], [6, 2, 2]], np.int64)
    sw = sweep_from_counts(thr, counts, 100)
    f1 = sw.metrics()["f1"]
    assert f1[1] == f1[3] == f1[4] == f1.max()
    assert sw.best() == (float(np.float32(0.4)), float(f1[3]))
    assert sw.best("f1") == sw.best()
    with pytest.raises(ValueError):
        sw.best("accuracy")


def _all_distinct_thresholds(p):
    vals = np.unique(p)
    return np.concatenate([[np.nextafter(vals[0], np.float32(-np.inf))], vals]).astype(np.float32)


@pytest.mark.parametrize("seed", [0, 1])
def test_average_precision_and_roc_auc_match_scikit_learn(seed):
    rng = np.random.default_rng(seed)
    n = 5000
    t = (rng.random(n) < 0.3).astype(np.uint8)
    p = (np.round(np.clip(rng.normal(0.35 + 0.3 * t, 0.2), 0, 1) * 200) / 200).astype(np.float32)   # 201 levels
    thr = _all_distinct_thresholds(p)
    sw = _sweep(p, t, thr)
    assert abs(sw.average_precision() - average_precision_score(t, p)) <= 1e-12
    assert abs(sw.roc_auc() - roc_auc_score(t, p)) <= 1e-12
    # the order in which the caller lists the thresholds does not matter
    perm = rng.permutation(thr.size)
    c = ref.sweep_counts(p, t, thr)[0]
    shuffled = sweep_from_counts(thr[perm], c[perm], n)
    assert shuffled.average_precision() == sw.average_precision() and shuffled.roc_auc() == sw.roc_auc()


def test_average_precision_and_roc_auc_per_group_and_one_class_groups():
    rng = np.random.default_rng(5)
    n = 600
    p = (rng.integers(0, 21, 3 * n) / 20).astype(np.float32)
    t = (rng.random(3 * n) < 0.4).astype(np.uint8)
    t[n:2 * n] = 0                     # group 1: no positives
    t[2 * n:] = 1                      # group 2: no negatives
    thr = _all_distinct_thresholds(p)
    sw = _sweep(p, t, thr, n)
    ap, auc = sw.average_precision(), sw.roc_auc()
    assert abs(ap[0] - average_precision_score(t[:n], p[:n])) <= 1e-12
    assert abs(auc[0] - roc_auc_score(t[:n], p[:n])) <= 1e-12
    assert np.isnan(ap[1:]).all() and np.isnan(auc[1:]).all()
    one = _sweep(p[n:2 * n], t[n:2 * n], thr)
    assert np.isnan(one.average_precision()) and np.isnan(one.roc_auc())


def test_threshold_handling():
    assert np.float32(0.5) in default_thresholds().tolist()
    d = default_thresholds()
    assert d.dtype == np.float32 and d.size == 99 and np.all(np.diff(d) > 0)
    assert np.array_equal(prepare_thresholds(None)[0], d)
    thr, uniq, inv = prepare_thresholds([0.7, 0.1, 0.7, 0.3, 0.1])
    assert thr.dtype == np.float32 and uniq.dtype == np.float32
    assert uniq.tolist() == [np.float32(0.1), np.float32(0.3), np.float32(0.7)]
    assert np.array_equal(uniq[inv], thr) and np.array_equal(thr, np.array([0.7, 0.1, 0.7, 0.3, 0.1], np.float32))
    # two float64 values that are one float32 are one threshold for the device
    assert prepare_thresholds([0.1, 0.1 + 1e-12])[1].size == 1
    p, t = np.zeros(4, np.float32), np.zeros(4, np.uint8)
    for bad in ([0.5, np.nan], [np.inf], [-np.inf, 0.5], [1e300], [], [[0.1, 0.2]]):
        with pytest.raises(ValueError):
            threshold_sweep(p, t, bad)
    with pytest.raises(ValueError):
        threshold_sweep(p, t, kind="sigmoid")


def test_shape_and_per_are_checked_before_the_device_is_touched():
    p = np.zeros((2, 3, 4), np.float32)
    with pytest.raises(ValueError):
        threshold_sweep(p, np.zeros((2, 3, 5), np.uint8))
    with pytest.raises(ValueError):
        threshold_sweep(p, np.zeros((2, 12), np.uint8))             # same size, another shape
    with pytest.raises(ValueError):
        threshold_sweep(p, np.zeros(24, np.uint8))
    t = np.zeros((2, 3, 4), np.uint8)
    for per in (-1, 4, 1.5, True):
        with pytest.raises(ValueError):
            threshold_sweep(p, t, per=per)
    with pytest.raises(ValueError):
        threshold_sweep(np.zeros((2, 3, 4), np.int32), t)           # scores are floating point
    big = np.zeros((65536, 1), np.float32)
    with pytest.raises(ValueError):
        threshold_sweep(big, np.zeros((65536, 1), np.uint8), per=1)  # more than 65535 groups


def test_an_empty_array_sweeps_to_zero_counts():
    sw = threshold_sweep(np.zeros((0, 4), np.float32), np.zeros((0, 4), np.uint8), [0.2, 0.8])
    assert sw.tp.tolist() == [0, 0] and sw.fn.tolist() == [0, 0] and int(sw.count) == 0
    assert sw.metrics()["iou"].tolist() == [1.0, 1.0]
