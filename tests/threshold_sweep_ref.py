"""NumPy restatement of rfi_threshold_sweep (include/rfi_hip.h): counts[g, k] = (tp, fp, fn) of ``p > thr[k]`` against
``truth != 0`` over group g, with p and thr compared in float32.  One plain comparison per threshold -- no histogram,
no suffix sums -- so it shares nothing with the device code but the definition."""
import numpy as np


def sweep_counts(p, truth, thr, group_elems=None):
    """int64 (n_groups, K, 3); ``group_elems=None``: one group"""
    p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1)
    pos = np.asarray(truth).reshape(-1) != 0
    thr = np.asarray(thr, dtype=np.float32).reshape(-1)
    if group_elems is None:
        group_elems = p.size
    p, pos = p.reshape(-1, group_elems), pos.reshape(-1, group_elems)
    out = np.zeros((p.shape[0], thr.size, 3), np.int64)
    with np.errstate(invalid="ignore"):
        for k, t in enumerate(thr):
            flag = p > t                                   # NaN > t is False: a NaN score is flagged nowhere
            out[:, k, 0] = (flag & pos).sum(axis=1)
            out[:, k, 1] = (flag & ~pos).sum(axis=1)
            out[:, k, 2] = (~flag & pos).sum(axis=1)
    return out


def thresholds(K, lo=-0.1, hi=1.1):
    """K strictly increasing float32 cuts from below 0 to above 1; for K >= 3 one of them is exactly 0"""
    thr = np.linspace(lo, hi, K, dtype=np.float64).astype(np.float32) if K > 1 else np.array([0.5], np.float32)
    if K >= 3:
        thr[np.argmin(np.abs(thr))] = 0.0
    assert np.all(np.diff(thr) > 0)
    return thr


def scores(n, thr, seed):
    """float32 scores in [-0.2, 1.2) laced with values exactly on thresholds, +-inf, NaN and -0.0"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.2, 1.2, n).astype(np.float32)
    on = rng.random(n) < 0.3
    p[on] = thr[rng.integers(0, thr.size, int(on.sum()))]
    special = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1.0], np.float32)
    at = rng.random(n) < 0.1
    p[at] = special[rng.integers(0, special.size, int(at.sum()))]
    return p


def truth(n, dtype, seed):
    """uint8 in {0, 1, 2, 255} or float32 in {0, 0.5, -1, -0.0}: non-zero == positive"""
    rng = np.random.default_rng(seed + 1000)
    vals = np.array([0, 1, 2, 255], np.uint8) if np.dtype(dtype) == np.uint8 else np.array([0.0, 0.5, -1.0, -0.0], np.float32)
    return vals[rng.integers(0, 4, n)]
