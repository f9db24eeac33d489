"""Confusion counts, metric curves and the best cut at EVERY threshold from one pass over the scores.

``threshold_sweep`` bins each score among the thresholds on the GPU (one histogram pass, ``rfi_threshold_sweep``) and
returns a ``ThresholdSweep``: integer (tp, fp, fn) per threshold -- exact, so equal to K calls of
``confusion_counts(p > t, true)`` bit for bit -- with the ratios formed on the host by the rules of ``metrics.py``.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from .._lib import MASK_CODES, VALUES_LOGITS, VALUES_PROBS, check, lib
from ..runtime import context_for, describe, operand

METRICS = ("iou", "precision", "recall", "f1", "dice")
MAX_THRESHOLDS = 1024          # per call of the library
MAX_GROUPS = 65535
_HIST_SLOTS = 1 << 25          # histogram words a call may ask for (256 MB): many groups sweep fewer thresholds a call


def default_thresholds():
    """0.01, 0.02, ..., 0.99 in float32; contains exactly ``np.float32(0.5)``."""
    return np.arange(1, 100, dtype=np.float32) / np.float32(100)


def prepare_thresholds(thresholds):
    """-> (thr, uniq, inverse): the caller's thresholds in float32, their sorted distinct values (what the device
    sweeps) and the map back, ``thr == uniq[inverse]``."""
    thr = default_thresholds() if thresholds is None else np.asarray(thresholds)
    if thr.ndim != 1 or thr.size == 0:
        raise ValueError(f"thresholds must be a non-empty 1-D sequence, got shape {thr.shape}")
    with np.errstate(over="ignore"):
        thr = thr.astype(np.float32)
    if not np.all(np.isfinite(thr)):
        raise ValueError("thresholds must be finite (in float32)")
    uniq, inverse = np.unique(thr, return_inverse=True)
    return thr, np.ascontiguousarray(uniq), inverse.reshape(-1)


def _ratio(num, den, empty):
    """num / den in float64 where den != 0, else ``empty``"""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    out = np.array(np.broadcast_to(np.asarray(empty, np.float64), den.shape))
    np.divide(num, den, out=out, where=den != 0)
    return out


@dataclass(frozen=True)
class ThresholdSweep:
    """(tp, fp, fn) of ``score > thresholds[k]`` for every k; ``tp`` / ``fp`` / ``fn`` are int64 of shape
    ``group_shape + (K,)`` in the order of ``thresholds`` (the caller's), ``count`` the elements of each group."""
    thresholds: np.ndarray
    tp: np.ndarray
    fp: np.ndarray
    fn: np.ndarray
    count: np.ndarray

    @property
    def group_shape(self):
        return tuple(self.tp.shape[:-1])

    def metrics(self):
        """dict of float64 arrays shaped like ``tp``; each element is ``metrics.py``'s ``_iou`` ... ``_dice`` of its counts."""
        tp, fp, fn = self.tp, self.fp, self.fn
        precision = _ratio(tp, tp + fp, np.where(fn == 0, 1.0, 0.0))
        recall = _ratio(tp, tp + fn, 1.0)
        return {"iou": _ratio(tp, tp + fp + fn, 1.0), "precision": precision, "recall": recall,
                "f1": _ratio(2 * (precision * recall), precision + recall, 0.0),
                "dice": _ratio(2 * tp, 2 * tp + fp + fn, 1.0)}

    def pooled(self):
        """the sweep of all groups taken together"""
        ax = tuple(range(self.tp.ndim - 1))
        return ThresholdSweep(self.thresholds, self.tp.sum(axis=ax), self.fp.sum(axis=ax), self.fn.sum(axis=ax),
                              np.asarray(self.count.sum(), np.int64))

    def best(self, metric="f1"):
        """(threshold, value) of the highest ``metric``; ties go to the lowest threshold.  Arrays of ``group_shape``
        for a grouped sweep."""
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
        order = np.argsort(self.thresholds, kind="stable")
        curve = self.metrics()[metric][..., order]
        at = np.argmax(curve, axis=-1)                           # the first maximum: the lowest threshold
        value = np.take_along_axis(curve, at[..., None], axis=-1)[..., 0]
        thr = self.thresholds[order][at]
        if self.tp.ndim == 1:
            return float(thr), float(value)
        return thr, value

    def _rates(self):
        """thresholds ascending: tp, fp (float64, group_shape + (K,)), positives P and negatives N (group_shape)"""
        order = np.argsort(self.thresholds, kind="stable")
        tp, fp = self.tp[..., order].astype(np.float64), self.fp[..., order].astype(np.float64)
        P = (self.tp[..., 0] + self.fn[..., 0]).astype(np.float64)
        N = np.asarray(self.count, np.float64) - P
        return tp, fp, P, N

    def average_precision(self):
        """sum_k (R_k - R_{k+1}) P_k over ascending thresholds, closed by a point of recall 0; P_k = 1 where nothing is
        flagged.  NaN for a group without positives or without negatives."""
        tp, fp, P, N = self._rates()
        ok = (P > 0) & (N > 0)
        rec = _ratio(tp, np.broadcast_to(P[..., None], tp.shape), 0.0)
        rec = np.concatenate([rec, np.zeros(rec.shape[:-1] + (1,))], axis=-1)
        prec = _ratio(tp, tp + fp, 1.0)
        ap = np.sum((rec[..., :-1] - rec[..., 1:]) * prec, axis=-1)
        ap = np.where(ok, ap, np.nan)
        return float(ap) if ap.ndim == 0 else ap

    def roc_auc(self):
        """trapezoid sum over (FPR_k, TPR_k), ascending thresholds, closed by the point (0, 0).  NaN for a group
        without positives or without negatives."""
        tp, fp, P, N = self._rates()
        ok = (P > 0) & (N > 0)
        zero = np.zeros(tp.shape[:-1] + (1,))
        tpr = np.concatenate([_ratio(tp, np.broadcast_to(P[..., None], tp.shape), 0.0), zero], axis=-1)
        fpr = np.concatenate([_ratio(fp, np.broadcast_to(N[..., None], fp.shape), 0.0), zero], axis=-1)
        auc = np.sum((fpr[..., :-1] - fpr[..., 1:]) * (tpr[..., :-1] + tpr[..., 1:]) / 2.0, axis=-1)
        auc = np.where(ok, auc, np.nan)
        return float(auc) if auc.ndim == 0 else auc


def sweep_from_counts(thresholds, counts, count):
    """A ``ThresholdSweep`` from ``counts`` of shape ``group_shape + (K, 3)`` (tp, fp, fn along the last axis)."""
    counts = np.asarray(counts, np.int64)
    thresholds = np.asarray(thresholds, np.float32)
    if counts.ndim < 2 or counts.shape[-1] != 3 or counts.shape[-2] != thresholds.size:
        raise ValueError(f"counts must be group_shape + ({thresholds.size}, 3), got {counts.shape}")
    return ThresholdSweep(thresholds, np.ascontiguousarray(counts[..., 0]), np.ascontiguousarray(counts[..., 1]),
                          np.ascontiguousarray(counts[..., 2]), np.asarray(count, np.int64))


def threshold_sweep(scores, true, thresholds=None, *, kind="probabilities", per=None, device=None):
    """Confusion counts of ``p > t`` against ``true`` (non-zero == positive) for every ``t`` of ``thresholds`` in one
    pass on the GPU.  ``p`` is ``scores`` (kind "probabilities") or its sigmoid as the library's kernels compute it
    (kind "logits").  ``thresholds=None``: 0.01 ... 0.99.  ``per=j``: one curve per index of the first ``j`` axes."""
    if kind not in ("probabilities", "logits"):
        raise ValueError(f"kind must be 'probabilities' or 'logits', got {kind!r}")
    thr, uniq, inverse = prepare_thresholds(thresholds)
    shape, dt, _, owner = describe(scores)
    floating = scores.dtype.is_floating_point if dt is None else dt.kind == "f"      # (None: a torch dtype NumPy lacks)
    if not floating or (owner is not None and dt != np.float32):
        raise ValueError(f"scores must be float32, got {scores.dtype if dt is None else dt}")
    tshape = describe(true)[0]
    if tshape != shape:
        raise ValueError(f"scores have shape {shape}, true has shape {tshape}")
    if per is None:
        group_shape = ()
    else:
        if isinstance(per, bool) or not isinstance(per, (int, np.integer)) or not 0 <= per <= len(shape):
            raise ValueError(f"per must be an integer in [0, {len(shape)}], got {per!r}")
        group_shape = shape[:int(per)]
    n_groups = int(np.prod(group_shape, dtype=np.int64))
    if n_groups > MAX_GROUPS:
        raise ValueError(f"{n_groups} groups: at most {MAX_GROUPS}")
    count = int(np.prod(shape, dtype=np.int64))
    counts = np.zeros((n_groups, uniq.size, 3), np.int64)
    group_elems = count // n_groups if n_groups else 0
    if count:
        ctx = context_for(device, scores, true)
        s = operand(scores, ctx, (np.float32,), "cast")
        t = operand(true, ctx, (np.uint8, np.float32), "nonzero")
        kmax = max(1, min(MAX_THRESHOLDS, _HIST_SLOTS // (2 * n_groups) - 1))
        for k0 in range(0, uniq.size, kmax):
            chunk = np.ascontiguousarray(uniq[k0:k0 + kmax])
            out = np.empty((n_groups, chunk.size, 3), np.int64)
            check(lib.rfi_threshold_sweep(ctx.handle, C.c_void_p(s.ptr), s.mem, VALUES_LOGITS if kind == "logits" else VALUES_PROBS,
                                          C.c_void_p(t.ptr), MASK_CODES[t.dtype], t.mem, count, group_elems, chunk.ctypes.data_as(C.c_void_p),
                                          chunk.size, out.ctypes.data_as(C.c_void_p)))
            counts[:, k0:k0 + chunk.size] = out
    counts = counts[:, inverse].reshape(group_shape + (thr.size, 3))
    return sweep_from_counts(thr, counts, np.full(group_shape, group_elems, np.int64))
