"""Segmentation metrics with the reference's signatures and edge-case rules
(rfi_toolbox/evaluation/metrics.py:25-172).  The three confusion counts (TP, FP, FN) are ONE
reduction on the GPU (uint8 or float32 input, non-zero == positive, metrics.py:36-37); the
ratios are formed on the host in Python floats exactly as the reference forms them."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .._lib import MASK_CODES, check, lib
from ..runtime import context_for, describe, operand


def confusion_counts(pred, true, device=None):
    """(tp, fp, fn) as Python ints."""
    pn, tn = (int(np.prod(describe(a)[0], dtype=np.int64)) for a in (pred, true))
    if pn != tn:
        raise ValueError(f"pred has {pn} elements, true has {tn}")
    ctx = context_for(device, pred, true)
    p, t = (operand(a, ctx, (np.uint8, np.float32), "nonzero") for a in (pred, true))
    tp, fp, fn = C.c_int64(), C.c_int64(), C.c_int64()
    check(lib.rfi_confusion_counts(ctx.handle, C.c_void_p(p.ptr), MASK_CODES[p.dtype], p.mem, C.c_void_p(t.ptr), MASK_CODES[t.dtype],
                                   t.mem, pn, C.byref(tp), C.byref(fp), C.byref(fn)))
    return tp.value, fp.value, fn.value


def _iou(tp, fp, fn):
    union = tp + fp + fn
    return 1.0 if union == 0 else tp / union


def _precision(tp, fp, fn):
    if tp + fp == 0:
        return 1.0 if fn == 0 else 0.0
    return tp / (tp + fp)


def _recall(tp, fp, fn):
    return 1.0 if tp + fn == 0 else tp / (tp + fn)


def _f1(tp, fp, fn):
    p, r = _precision(tp, fp, fn), _recall(tp, fp, fn)
    return 0.0 if p + r == 0 else 2 * (p * r) / (p + r)


def _dice(tp, fp, fn):
    return 1.0 if 2 * tp + fp + fn == 0 else (2 * tp) / (2 * tp + fp + fn)


def compute_iou(pred, true):
    return _iou(*confusion_counts(pred, true))


def compute_precision(pred, true):
    return _precision(*confusion_counts(pred, true))


def compute_recall(pred, true):
    return _recall(*confusion_counts(pred, true))


def compute_f1(pred, true):
    return _f1(*confusion_counts(pred, true))


def compute_dice(pred, true):
    return _dice(*confusion_counts(pred, true))


def evaluate_segmentation(pred, true):
    """dict with 'iou', 'precision', 'recall', 'f1', 'dice' (metrics.py:155-172)."""
    c = confusion_counts(pred, true)
    return {"iou": _iou(*c), "precision": _precision(*c), "recall": _recall(*c), "f1": _f1(*c),
            "dice": _dice(*c)}
