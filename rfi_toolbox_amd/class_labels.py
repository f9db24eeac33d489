"""Class-bit labels: up to eight boolean class masks of a pixel in the one label byte the data path already carries.

    labels = pack_class_masks(masks)                  # (n, K, H, W) bool -> (n, H, W) uint8, bit k = class k
    model = UNet(8, K, 32).set_targets("class_bits")  # the target of output channel k is (label >> k) & 1
    model.train_step(images, labels)

The byte goes through ``TorchDataset``, ``BatchWriter`` shards, ``RFIMaskDataset`` and ``training.Augmenter`` (a
nearest-neighbour copy of the byte) as any label map does.  ``core.family_masks`` makes such labels on the device for a
simulated batch.  Pure NumPy: nothing here needs the GPU.
"""
from __future__ import annotations

import numpy as np

MAX_CLASSES = 8


def pack_class_masks(masks, channel_axis=None):
    """``(..., K, H, W)`` or ``(..., H, W, K)`` class masks (non-zero == member), K <= 8 -> ``(..., H, W)`` uint8 with bit k
    set where class k is.  ``channel_axis``: -3 or -1; None takes -3 unless only the last axis is at most 8 long."""
    m = np.asarray(masks)
    if m.ndim < 3:
        raise ValueError(f"masks must be (..., K, H, W) or (..., H, W, K), got shape {m.shape}")
    if channel_axis is None:
        channel_axis = -3 if m.shape[-3] <= MAX_CLASSES or m.shape[-1] > MAX_CLASSES else -1
    if channel_axis not in (-3, -1):
        raise ValueError(f"channel_axis must be -3 or -1, got {channel_axis!r}")
    m = np.moveaxis(m != 0, channel_axis, -1)
    K = m.shape[-1]
    if not 1 <= K <= MAX_CLASSES:
        raise ValueError(f"1 to {MAX_CLASSES} classes fit a label byte, got {K}")
    weights = (1 << np.arange(K)).astype(np.uint8)
    return (m * weights).sum(axis=-1, dtype=np.uint8)


def unpack_class_bits(bits, num_classes, channel_axis=-3):
    """The inverse: ``(..., H, W)`` uint8 -> bool ``(..., K, H, W)`` (``channel_axis=-1``: ``(..., H, W, K)``) with
    ``[k] = (bits >> k) & 1``; bits at and above ``num_classes`` are dropped."""
    b = np.asarray(bits)
    if b.dtype != np.uint8 and b.dtype != np.bool_:
        raise ValueError(f"bits must be uint8, got {b.dtype}")
    if b.ndim < 2:
        raise ValueError(f"bits must be (..., H, W), got shape {b.shape}")
    K = int(num_classes)
    if not 1 <= K <= MAX_CLASSES:
        raise ValueError(f"num_classes must be in 1 .. {MAX_CLASSES}, got {num_classes!r}")
    if channel_axis not in (-3, -1):
        raise ValueError(f"channel_axis must be -3 or -1, got {channel_axis!r}")
    out = ((b.astype(np.uint8)[..., None] >> np.arange(K, dtype=np.uint8)) & 1).astype(np.bool_)
    return out if channel_axis == -1 else np.moveaxis(out, -1, -3)


# ---- the ignore bit (``model.set_ignore(True)``, RFI_LABEL_IGNORE in include/rfi_hip.h): bit 7 of the label byte takes the
# pixel out of the loss and out of the evaluation counts.  It rides in the byte, so everything that carries labels carries it
IGNORE = 0x80


def with_ignore(labels, ignore):
    """``labels`` (uint8 or bool, a map or class bits of at most 7 classes) with bit 7 set where ``ignore`` is non-zero.
    The low seven bits stay as they are: ``split_ignore`` gives both back."""
    b = np.asarray(labels)
    if b.dtype != np.uint8 and b.dtype != np.bool_:
        raise ValueError(f"labels must be uint8 or bool, got {b.dtype}")
    b = b.astype(np.uint8)
    if (b & IGNORE).any():
        raise ValueError("labels already use bit 7: the ignore bit needs labels below 0x80 (at most 7 classes)")
    ig = np.broadcast_to(np.asarray(ignore) != 0, b.shape)
    return b | (ig.astype(np.uint8) << 7).astype(np.uint8)


def split_ignore(labels):
    """``(labels & 0x7F, ignored)``: the label bytes without bit 7 and the bool mask of the pixels that had it"""
    b = np.asarray(labels)
    if b.dtype != np.uint8:
        raise ValueError(f"labels must be uint8, got {b.dtype}")
    return b & np.uint8(0x7F), (b & np.uint8(IGNORE)) != 0
