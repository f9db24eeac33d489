"""The callers either side of the hot path, with the reference scripts' semantics.

* ``train_rfi_model``  -- the loop of scripts/train_model.py:133-193: per epoch shuffle, one
  ``train_step`` per batch (BCE-with-logits + dice, clip 1.0, Adam with coupled L2), validation
  loss in eval mode averaged over batches (:157-167), stop on NaN (:170-172), checkpoint dict
  ``{epoch, model_state_dict, optimizer_state_dict, loss, args}`` whenever the validation loss
  improves (:174-184) and a final ``{model_state_dict, args}`` (:189-193).  Unlike the reference
  the checkpoint directory is created and ``resume_from`` actually resumes.
* ``evaluate_rfi_model`` -- scripts/evaluate_model.py:18-58: eval mode, per batch
  ``sigmoid > 0.5`` -> ``evaluate_segmentation``, then the MEAN OF THE PER-BATCH metrics
  (:54-56; not the metric of the pooled counts).
* ``Augmenter`` -- train_model.py:44-53,70-75 (``--augment``): HorizontalFlip, VerticalFlip, Rotate(15) and
  ShiftScaleRotate(0.05, 0.05, 10), each with p = 0.5, of a batch and its masks on the device
  (``rfi_augment_batch``).  Distribution-level parity: the same family of transforms with this project's own
  Philox stream, the data resampled ONCE through the composed transform (the reference interpolates per transform).
Data are TorchDataset-like (``.images`` NHWC float32, ``.labels`` uint8) or (images, labels) pairs.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np
import torch

from ._lib import AugmentConfig, check, lib
from .evaluation.metrics import _dice, _f1, _iou, _precision, _recall
from .runtime import as_pointer, context_for, is_torch


def _pair(ds):
    if hasattr(ds, "images"):
        return ds.images, ds.labels
    return ds


def _batches(n, batch_size, order=None):
    idx = np.arange(n) if order is None else order
    for i in range(0, n, batch_size):
        yield idx[i:i + batch_size]


_METRICS = {"iou": _iou, "precision": _precision, "recall": _recall, "f1": _f1, "dice": _dice}


def evaluate_rfi_model(model, dataset, batch_size=4, threshold=0.5, class_names=None):
    """dict of mean per-batch iou / precision / recall / f1 / dice (evaluate_model.py:54-56).

    A model with class-bit targets (``set_targets("class_bits")``) gives the same five metrics per class, each the mean
    of its per-batch values under the same rules: ``{"per_class": [{"name": ..., "iou": ..., ...}, ...], "macro": {...}}``
    with ``macro`` the mean over the classes; ``class_names`` (one per output channel) names the entries, else they
    are ``"class0"`` ..."""
    images, labels = _pair(dataset)
    by_class = getattr(model, "targets", "map") == "class_bits"
    if class_names is not None:
        if not by_class:
            raise ValueError("class_names belongs to a model with class-bit targets")
        class_names = [str(v) for v in class_names]
        if len(class_names) != model.out_channels:
            raise ValueError(f"class_names must name the {model.out_channels} output channels, got {len(class_names)}")
    was_training = model.training
    model.eval()
    per_batch = []                    # one row of counts per class and batch
    try:
        for sel in _batches(len(images), batch_size):
            c = np.asarray(model.eval_batch(images[sel], labels[sel], threshold), np.int64).reshape(-1, 3)
            per_batch.append([{k: f(*(int(v) for v in row)) for k, f in _METRICS.items()} for row in c])
    finally:
        model.train(was_training)
    if not per_batch:
        raise ValueError("empty dataset")
    classes = [{k: float(np.mean([b[j][k] for b in per_batch])) for k in _METRICS} for j in range(len(per_batch[0]))]
    if not by_class:
        return classes[0]
    names = class_names or [f"class{j}" for j in range(len(classes))]
    return {"per_class": [dict(name=nm, **m) for nm, m in zip(names, classes)],
            "macro": {k: float(np.mean([m[k] for m in classes])) for k in _METRICS}}


def sweep_rfi_model(model, dataset, batch_size=4, thresholds=None):
    """``evaluate_rfi_model`` at every threshold from one forward pass per batch.  Returns a dict: ``thresholds``
    (float32, the caller's order; None: 0.01 ... 0.99), ``mean_per_batch`` metric -> (K,) under the reference's rule
    (the mean of the per-batch metrics, evaluate_model.py:54-56 -- at a threshold of the sweep it equals
    ``evaluate_rfi_model(..., threshold=t)``), ``pooled`` the ``ThresholdSweep`` of all batches' counts together,
    ``best`` metric -> (threshold, value) under the per-batch rule, ties to the lowest threshold.  Raises while the model's
    ignore switch is on (``set_ignore``), as ``eval_sweep`` does: the pooled count is the size of the label array.  Sweep the
    valid pixels with ``evaluation.threshold_sweep(prob[valid], truth[valid])`` instead."""
    from .evaluation.sweep import prepare_thresholds, sweep_from_counts
    thr = prepare_thresholds(thresholds)[0]
    images, labels = _pair(dataset)
    was_training = model.training
    model.eval()
    counts = []
    try:
        for sel in _batches(len(images), batch_size):
            counts.append(model.eval_sweep(images[sel], labels[sel], thr))
    finally:
        model.train(was_training)
    if not counts:
        raise ValueError("empty dataset")
    rules = {"iou": _iou, "precision": _precision, "recall": _recall, "f1": _f1, "dice": _dice}
    mean = {name: np.array([float(np.mean([f(*(int(v) for v in c[k])) for c in counts])) for k in range(thr.size)])
            for name, f in rules.items()}
    order = np.argsort(thr, kind="stable")
    best = {}
    for name, curve in mean.items():
        at = order[int(np.argmax(curve[order]))]
        best[name] = (float(thr[at]), float(curve[at]))
    counts = np.stack(counts)
    pooled = sweep_from_counts(thr, counts.sum(axis=0), int(np.prod(np.shape(labels), dtype=np.int64)))
    return {"thresholds": thr, "mean_per_batch": mean, "pooled": pooled, "best": best}


def save_checkpoint(path, model, epoch=None, loss=None, args=None, optimizer_hyper=None):
    """The dict train_model.py:177-183 writes (or :190-193 when epoch is None)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    ck = {"model_state_dict": model.state_dict(), "args": args}
    if epoch is not None:
        ck.update(epoch=epoch, loss=loss, optimizer_state_dict=model.optimizer_state_dict(**(optimizer_hyper or {})))
    torch.save(ck, path)
    return path


def load_checkpoint(path, model, load_optimizer=True):
    ck = torch.load(path, map_location="cpu", weights_only=False)
    model.load_state_dict(ck["model_state_dict"] if "model_state_dict" in ck else ck)
    if load_optimizer and isinstance(ck, dict) and "optimizer_state_dict" in ck:
        model.load_optimizer_state_dict(ck["optimizer_state_dict"])
    return ck


class Augmenter:
    """The reference's training augmentation on the device.  ``aug(images, labels, call)`` warps a batch (n, H, W, C)
    float32 and its masks (n, H, W) uint8 into two new ``DeviceArray``s; sample i of call number ``call`` draws its
    transform from (seed, call, i) alone (semantics: include/rfi_hip.h), so equal arguments give equal bits."""

    _PROBS = ("p_hflip", "p_vflip", "p_rotate", "p_ssr")
    _LIMITS = ("rotate_limit", "shift_limit", "scale_limit", "ssr_rotate_limit")

    def __init__(self, seed=0, p_hflip=0.5, p_vflip=0.5, p_rotate=0.5, rotate_limit=15, p_ssr=0.5, shift_limit=0.05,
                 scale_limit=0.05, ssr_rotate_limit=10, device=None):
        if not isinstance(seed, (int, np.integer)) or isinstance(seed, bool) or not 0 <= seed < 2 ** 64:
            raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
        self.seed = int(seed)
        given = dict(p_hflip=p_hflip, p_vflip=p_vflip, p_rotate=p_rotate, rotate_limit=rotate_limit, p_ssr=p_ssr,
                     shift_limit=shift_limit, scale_limit=scale_limit, ssr_rotate_limit=ssr_rotate_limit)
        for k, v in given.items():
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                raise ValueError(f"{k} must be a finite number, got {v!r}")
            if k in self._PROBS and not 0.0 <= v <= 1.0:
                raise ValueError(f"{k} must be in [0, 1], got {v!r}")
            if k in self._LIMITS and v < 0:
                raise ValueError(f"{k} must be >= 0, got {v!r}")
            setattr(self, k, float(v))
        if np.float32(self.scale_limit) >= 1:
            raise ValueError(f"scale_limit must be < 1, got {scale_limit!r}")
        self.device = device

    def _config(self):
        return AugmentConfig(self.seed, self.p_hflip, self.p_vflip, self.p_rotate, self.rotate_limit, self.p_ssr,
                             self.shift_limit, self.scale_limit, self.ssr_rotate_limit)

    @staticmethod
    def _call(call):
        if not isinstance(call, (int, np.integer)) or isinstance(call, bool) or not 0 <= call < 2 ** 64:
            raise ValueError(f"call must be an integer in [0, 2^64), got {call!r}")
        return int(call)

    def params(self, n, h, w, call=0):
        """(gates (n, 4) int32 = hflip, vflip, rotate, ssr; inv (n, 6) float64 = the row-major 2 x 3 map from an output
        pixel to its source position) of the samples of call ``call``: the host evaluation of what the kernel draws."""
        call = self._call(call)
        if n < 0 or h < 1 or w < 1:
            raise ValueError(f"needs n >= 0 and h, w >= 1, got {(n, h, w)}")
        gates, inv = np.zeros((n, 4), np.int32), np.zeros((n, 6), np.float64)
        cfg = self._config()
        check(lib.rfi_augment_params(C.byref(cfg), call, n, h, w, gates.ctypes.data_as(C.POINTER(C.c_int32)),
                                     inv.ctypes.data_as(C.POINTER(C.c_double))))
        return gates, inv

    def __call__(self, images, labels, call=0):
        call = self._call(call)
        shape, lshape = tuple(images.shape), tuple(labels.shape)
        if len(shape) != 4 or not 1 <= shape[3] <= 16 or shape[1] < 1 or shape[2] < 1:
            raise ValueError(f"images must be (n, H, W, C) with 1 <= C <= 16, got shape {shape}")
        if lshape != shape[:3]:
            raise ValueError(f"labels shape {lshape} does not match images {shape}")
        n, h, w, c = shape
        ctx = context_for(self.device, images, labels)
        xp, xm, k1 = as_pointer(images, np.float32, ctx)
        yp, ym, k2 = as_pointer(labels, np.uint8, ctx)
        x_out, y_out = ctx.empty(shape, np.float32), ctx.empty(lshape, np.uint8)
        cfg = self._config()
        check(lib.rfi_augment_batch(ctx.handle, C.c_void_p(xp), xm, C.c_void_p(yp), ym, n, h, w, c, C.byref(cfg), call,
                                    C.c_void_p(x_out.ptr), C.c_void_p(y_out.ptr)))
        if any(is_torch(k) for k in (k1, k2)):
            ctx.synchronize()                 # before torch's allocator may hand the (possibly temporary) CUDA tensors out again
        del k1, k2
        return x_out, y_out

    def state_dict(self):
        """plain numbers (for a checkpoint's ``args``)"""
        return {"seed": self.seed, **{k: getattr(self, k) for k in self._PROBS + self._LIMITS}}

    @classmethod
    def from_state_dict(cls, state, device=None):
        return cls(device=device, **state)


def train_rfi_model(model, train_data, val_data=None, num_epochs=50, batch_size=4, lr=1e-4,
                    weight_decay=1e-5, checkpoint_dir=None, resume_from=None, args=None, log=print,
                    augment=False, augment_seed=0):
    """Returns the history [{epoch, train_loss, val_loss}].  Defaults = train_model.py:86-95.  augment=True
    (train_model.py --augment): training batch b of epoch e (both 0-based, e counted from 0 also when resuming) goes
    through ``Augmenter(seed=augment_seed)(x, y, call=(e << 32) | b)`` on the device; validation data never does."""
    aug = Augmenter(seed=augment_seed, device=getattr(getattr(model, "ctx", None), "device_index", None)) if augment else None
    tr_x, tr_y = _pair(train_data)
    start_epoch = 0
    if resume_from:
        start_epoch = int(load_checkpoint(resume_from, model).get("epoch", 0))
    hyper = dict(lr=lr, weight_decay=weight_decay)
    best, history = float("inf"), []
    for epoch in range(start_epoch, num_epochs):
        model.train()
        order = torch.randperm(len(tr_x)).numpy()            # DataLoader(shuffle=True), train_model.py:106
        if aug is None:
            losses = [model.train_step(tr_x[sel], tr_y[sel], **hyper) for sel in _batches(len(tr_x), batch_size, order)]
        else:
            losses = [model.train_step(*aug(tr_x[sel], tr_y[sel], call=(epoch << 32) | b), **hyper)
                      for b, sel in enumerate(_batches(len(tr_x), batch_size, order))]
        rec = {"epoch": epoch + 1, "train_loss": float(np.mean(losses)), "val_loss": None}
        if val_data is not None:
            va_x, va_y = _pair(val_data)
            model.eval()
            vl = [model.loss(va_x[sel], va_y[sel]) for sel in _batches(len(va_x), batch_size)]
            rec["val_loss"] = float(np.mean(vl))
            log(f"Epoch [{epoch + 1}/{num_epochs}] - Train Loss: {rec['train_loss']:.4f} - Val Loss: {rec['val_loss']:.4f}")
            if math.isnan(rec["val_loss"]):
                log("Validation loss is NaN, stopping training.")
                history.append(rec)
                break
            if rec["val_loss"] < best and checkpoint_dir:
                best = rec["val_loss"]
                save_checkpoint(os.path.join(checkpoint_dir, f"unet_rfi_epoch_{epoch + 1}.pt"), model, epoch + 1,
                                losses[-1], args, hyper)
        history.append(rec)
    if checkpoint_dir:
        save_checkpoint(os.path.join(checkpoint_dir, "unet_rfi_final.pt"), model, args=args)
    return history
