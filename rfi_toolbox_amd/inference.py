"""Whole-observation flag prediction: complex visibilities in, one flag per waterfall pixel out.

The reference's workflow (README Quick Start, steps 2-5) tiles an observation with
``Preprocessor.create_dataset(inference_mode=True)``, runs the model on the patches and hands flags of shape
``(baselines, pols, channels, times)`` to ``MSLoader.save_flags``; the step that puts the patch outputs back together
is left to the user.  ``predict_flags`` does all of it on the GPU in one call (``rfi_model_predict_flags``): the
tiling and channel extraction straight from the waterfall, the eval-mode forward in batches, and the inverse tiling
(``rfi_stitch_patches``), streaming the observation through in chunks of whole planes.  Patches made by any other
model -- a user's own torch network included -- are put back with ``Preprocessor.reconstruct_flags``.

Tiling and combining rules (include/rfi_hip.h, rfi_tiling): ``views`` 1, 2 or 4 select the views {0}, {0,1},
{0,1,2,3} of the plane (plane, plane[::-1,:], plane.T, plane.T[::-1,:]); along an axis of length L > ps the tile
origins are 0, s, ..., k*s with k = ceil((L - ps) / s), and ``edge="shift"`` moves the last one to L - ps so that no
tile holds padding; every pixel combines sigmoid(logit) -- or the model's probability when its head applies a
sigmoid -- of every tile that covers it, in ascending view / tile row / tile column order, by float32 mean or max,
and is flagged when that value is strictly greater than ``threshold``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import COMBINE_MAX, COMBINE_MEAN, COMPLEX_CODES, EDGE_PAD, EDGE_SHIFT, Tiling, check, lib
from .runtime import as_pointer, describe, is_torch, result_buffer, torch

_COMBINE = {"mean": COMBINE_MEAN, "max": COMBINE_MAX}
_EDGE = {"pad": EDGE_PAD, "shift": EDGE_SHIFT}


def _downsampling(model) -> int:
    """Factor the model's input side must be a multiple of (its pooling levels)."""
    depth = getattr(model, "depth", None)
    return 2 ** int(depth) if depth else 1


def check_tiling_args(patch_size, stride, views, combine, edge):
    """-> (ps, stride) after the argument checks that need no model."""
    if not isinstance(patch_size, (int, np.integer)) or patch_size <= 0:
        raise ValueError(f"patch_size must be a positive integer, got {patch_size!r}")
    ps = int(patch_size)
    s = ps if stride is None else stride
    if not isinstance(s, (int, np.integer)) or not 1 <= s <= ps:
        raise ValueError(f"stride must be an integer in [1, patch_size={ps}], got {stride!r}")
    if views not in (1, 2, 4):
        raise ValueError(f"views must be 1, 2 or 4, got {views!r}")
    if combine not in _COMBINE:
        raise ValueError(f"combine must be 'mean' or 'max', got {combine!r}")
    if edge not in _EDGE:
        raise ValueError(f"edge must be 'pad' or 'shift', got {edge!r}")
    return ps, int(s)


def tiling_count(channels, times, patch_size=128, stride=None, views=1, edge="pad") -> int:
    """Patches one (channels x times) plane is cut into (``rfi_tiling_count``; host only)."""
    ps, s = check_tiling_args(patch_size, stride, views, "mean", edge)
    n = C.c_int64()
    check(lib.rfi_tiling_count(int(channels), int(times), C.byref(Tiling(ps, s, _EDGE[edge], views)), C.byref(n)))
    return n.value


def predict_flags(model, data, patch_size=128, stride=None, views=1, combine="mean", threshold=0.5, batch_size=64,
                  edge="pad", return_probabilities=False):
    """Flags of a whole observation from a segmentation model.

    ``data``: complex64 / complex128 visibilities ``(B, P, C, T)`` or ``(P, C, T)``, a NumPy array or a torch tensor (a
    CUDA tensor stays on the device).  ``model``: a ``HipSegmenter`` with 3 input channels and 1 output channel (the
    U-Net family, ``SimpleCNN``, ``UNetResNet18(3, 1, ...)``), in any mode: the forward runs in eval mode and leaves
    ``model.training`` and the BatchNorm running buffers alone; its compute dtype applies.  Returns bool flags of
    ``data``'s shape (NumPy for NumPy or CPU-tensor input, a CUDA tensor for CUDA input) and, with
    ``return_probabilities``, the float32 combined probabilities as a second result.
    """
    from .models.unet import HipSegmenter

    ps, s = check_tiling_args(patch_size, stride, views, combine, edge)
    if not isinstance(batch_size, (int, np.integer)) or batch_size <= 0:
        raise ValueError(f"batch_size must be a positive integer, got {batch_size!r}")
    shape, dt = describe(data)[:2]
    complex_in = data.is_complex() if dt is None else dt.kind == "c"
    if dt is None or dt not in COMPLEX_CODES:
        dt = np.dtype(np.complex128)
    if not complex_in:
        raise ValueError("predict_flags takes complex visibilities; for real-valued input build the patches with "
                         "Preprocessor(data).create_dataset(..., inference_mode=True), run the model and put the "
                         "flags back with Preprocessor.reconstruct_flags")
    if len(shape) not in (3, 4):
        raise ValueError(f"data must be (B, P, C, T) or (P, C, T), got shape {shape}")
    if not isinstance(model, HipSegmenter):
        raise TypeError(f"predict_flags needs a rfi_toolbox_amd segmentation model, got {type(model).__name__}")
    if model.in_channels != 3 or model.out_channels != 1 or model._out_scale != 1:
        raise ValueError(f"predict_flags needs a model with 3 input channels and 1 output channel the size of its "
                         f"input, got {type(model).__name__} with {model.in_channels} -> {model.out_channels}")
    f = _downsampling(model)
    if ps % f:
        raise ValueError(f"patch_size {ps} is not a multiple of {f}, the downsampling factor of {type(model).__name__}")
    Cn, Tn = int(shape[-2]), int(shape[-1])
    n_planes = int(np.prod(shape[:-2], dtype=np.int64))
    ctx = model.ctx
    ptr, mem, keep = as_pointer(data, dt, ctx)
    flags, fp, omem = result_buffer(ctx, shape, np.uint8, "host", data)
    prob, pp, _ = result_buffer(ctx, shape, np.float32, "host", data) if return_probabilities else (None, None, None)
    if n_planes and Cn and Tn:
        check(lib.rfi_model_predict_flags(model._h, C.c_void_p(ptr), mem, COMPLEX_CODES[dt], n_planes, Cn, Tn,
                                          C.byref(Tiling(ps, s, _EDGE[edge], views)), int(batch_size), _COMBINE[combine],
                                          float(threshold), C.c_void_p(fp), omem, C.c_void_p(pp) if pp else None, omem))
    del keep
    flags = flags.view(torch.bool) if is_torch(flags) else flags.view(bool)
    return (flags, prob) if return_probabilities else flags
