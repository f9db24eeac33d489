"""Whole-observation flag prediction: complex visibilities in, one flag per waterfall pixel out.

The reference's workflow (README Quick Start, steps 2-5) tiles an observation with
``Preprocessor.create_dataset(inference_mode=True)``, runs the model on the patches and hands flags of shape
``(baselines, pols, channels, times)`` to ``MSLoader.save_flags``; the step that puts the patch outputs back together
is left to the user.  ``predict_flags`` does all of it on the GPU in one call (``rfi_model_predict_flags``): the
tiling and channel extraction straight from the waterfall, the eval-mode forward in batches, and the inverse tiling
(``rfi_stitch_patches``), streaming the observation through in chunks of whole planes.  Patches made by any other
model -- a user's own torch network included -- are put back with ``Preprocessor.reconstruct_flags``.

A model with 8 input channels (the reference's default: real and imaginary parts of RR, RL, LR, LL of a normalised
sample) goes through the same pipeline with another gather (``rfi_model_predict_flags_pol``, csrc/pol_gather.hip): one
kernel cuts the tiles, applies the views, stacks the four polarisations of a baseline and normalises with the
arithmetic of ``Normalizer.transform``; one plane of flags per baseline comes back.  ``tile_observation`` is that
gather alone and ``stitch_patches`` the inverse tiling alone, for users who run their own model on the tiles.

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

from ._lib import (COMBINE_MAX, COMBINE_MEAN, COMPLEX_CODES, DEVICE, EDGE_PAD, EDGE_SHIFT, VALUES_LOGITS,
                   VALUES_PROBS, Tiling, check, lib)
from .runtime import DeviceArray, check_out, context_for, describe, is_torch, operand, result_buffer, torch

__all__ = ["predict_flags", "tile_observation", "stitch_patches", "tiling_count", "check_tiling_args"]

_COMBINE = {"mean": COMBINE_MEAN, "max": COMBINE_MAX}
_EDGE = {"pad": EDGE_PAD, "shift": EDGE_SHIFT}
_SAMPLE_GROUP_BYTES = 256 << 20        # input a sample-scope normalizer takes statistics of at a time (whole baselines)
_SAMPLE_GROUP_MAX = 4096               # rfi_norm_statistics' populations per call


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


def _complex_input(data, what):
    """-> (shape, dtype the kernels get) of complex visibilities; ValueError for real data (touches no device)."""
    shape, dt = describe(data)[:2]
    complex_in = data.is_complex() if dt is None else dt.kind == "c"
    if dt is None or dt not in COMPLEX_CODES:
        dt = np.dtype(np.complex128)
    if not complex_in:
        raise ValueError(f"{what} takes complex visibilities; for real-valued input build the patches with "
                         "Preprocessor(data).create_dataset(..., inference_mode=True), run the model and put the "
                         "flags back with Preprocessor.reconstruct_flags")
    return tuple(int(v) for v in shape), dt


def _pol_shape(shape, what="data"):
    """(n_samples, C, T) of complex (B, 4, C, T) / (4, C, T) input for an 8-channel model."""
    if len(shape) not in (3, 4) or shape[-3] != 4:
        raise ValueError(f"a model with 8 input channels takes the 4 polarisations RR, RL, LR, LL: {what} must be "
                         f"(B, 4, C, T) or (4, C, T), got shape {tuple(shape)}")
    return (shape[0] if len(shape) == 4 else 1), shape[-2], shape[-1]


def _normalizer_form(normalizer):
    """-> ("pair", centre, scale) or ("sample", method); the checks that need no device."""
    from .preprocessing.normalization import Normalizer
    if normalizer is None:
        return "pair", 0.0, 1.0
    if not isinstance(normalizer, Normalizer):
        raise TypeError(f"normalizer must be a rfi_toolbox_amd Normalizer or None, got {type(normalizer).__name__}")
    if normalizer.scope == "dataset":
        if normalizer.centres is None:
            raise RuntimeError("predict_flags with an unfitted dataset-scope normalizer: call fit (or load_state_dict) first")
        return "pair", float(normalizer.centres[0]), float(normalizer.scales[0])
    if normalizer.method is None:
        return "pair", 0.0, 1.0
    return "sample", normalizer.method


def _sample_groups(n, sample_bytes):
    """[b0, b1) runs of whole baselines a sample-scope normalizer is applied to at a time."""
    g = max(1, min(_SAMPLE_GROUP_MAX, _SAMPLE_GROUP_BYTES // max(1, sample_bytes)))
    return [(b0, min(n, b0 + g)) for b0 in range(0, n, g)]


def _group_on_device(o, ctx, b0, b1, sample_shape):
    """Baselines [b0, b1) of the resolved operand `o` as a DeviceArray: a view of device input, one upload of host input."""
    shape = (b1 - b0,) + tuple(sample_shape)
    if o.mem == DEVICE:
        per = int(np.prod(sample_shape, dtype=np.int64)) * o.dtype.itemsize
        return DeviceArray.borrow(ctx, o.ptr + b0 * per, shape, o.dtype, o.keep)
    return ctx.to_device(o.keep.reshape((-1,) + tuple(sample_shape))[b0:b1])


def _sample_pairs(normalizer, group):
    """(len(group), 2) float64 (centre, scale) of every baseline of the DeviceArray `group` by its own statistics: what
    ``Normalizer(method, "sample").fit(group)`` keeps.  Raises ValueError on non-finite input."""
    from .preprocessing.normalization import sample_parameters
    stats = normalizer.statistics(group, quantiles=normalizer.method == "robust_scale")
    return np.ascontiguousarray([sample_parameters(normalizer.method, st) for st in stats], dtype=np.float64).reshape(-1, 2)


def _as_bool(flags):
    return flags.view(torch.bool) if is_torch(flags) else (flags if isinstance(flags, DeviceArray) else flags.view(bool))


def _flag_buffer(ctx, shape, out, like):
    """result_buffer for flags: bytes the kernels write, handed back as bool by _as_bool."""
    return result_buffer(ctx, shape, np.bool_ if out == "device" else np.uint8, out, like)


def _broadcast_pols(ctx, flags, shape):
    """(B, C, T) or (C, T) flags -> `shape` = (B, 4, C, T) or (4, C, T): every polarisation gets its baseline's flags."""
    if isinstance(flags, DeviceArray):
        res = ctx.empty(shape, flags.dtype)
        px = int(shape[-2]) * int(shape[-1])
        rows = flags.nbytes // px if px else 0
        for p in range(4 if rows else 0):
            check(lib.rfi_op_copy_rows(ctx.handle, C.c_void_p(flags.ptr), px, C.c_void_p(res.ptr + p * px), 4 * px, px, rows))
        return res
    if is_torch(flags):
        return flags.unsqueeze(-3).expand(*shape).contiguous()
    return np.ascontiguousarray(np.broadcast_to(np.expand_dims(flags, -3), shape))


def predict_flags(model, data, patch_size=128, stride=None, views=1, combine="mean", threshold=0.5, batch_size=64,
                  edge="pad", return_probabilities=False, normalizer=None, broadcast_pols=True, out="host"):
    """Flags of a whole observation from a segmentation model.

    ``data``: complex64 / complex128 visibilities, a NumPy array, a torch tensor (a CUDA tensor stays on the device) or
    a ``DeviceArray``.  ``model``: a ``HipSegmenter`` with 1 output channel the size of its input (the U-Net family,
    ``SimpleCNN``, ``UNetResNet18``), in any mode: the forward runs in eval mode and leaves ``model.training`` and the
    BatchNorm running buffers alone; its compute dtype applies.

    * 3 input channels: ``data`` is ``(B, P, C, T)`` or ``(P, C, T)``; every plane is flagged from its own amplitude
      gradient, log-amplitude and phase.  Returns bool flags of ``data``'s shape.
    * 8 input channels (the reference's default model): ``data`` is ``(B, 4, C, T)`` or ``(4, C, T)`` in the order RR,
      RL, LR, LL; the network sees the real and imaginary parts of the four polarisations of a tile, normalised by
      ``normalizer``: ``None`` (a float32 cast), a fitted ``Normalizer(scope="dataset")`` (its one pair), or a
      ``Normalizer(method, scope="sample")``, fitted or not, which normalises every baseline by the statistics of its
      own whole ``8 C T`` scalars (never per tile; a stored fit is ignored).  One flag per baseline pixel comes out:
      with ``broadcast_pols`` it is repeated over the four polarisations (``data``'s shape, what ``MSLoader.save_flags``
      takes), without it the flags are ``(B, C, T)`` / ``(C, T)``.  The probabilities are always per baseline.

    Tiling works on the last two axes as they are: a model trained on the simulator's ``(T, F)`` planes must be given
    observation planes in that orientation (``views=4`` covers both).  Results are NumPy arrays (for NumPy or CPU-tensor
    input), CUDA tensors (for CUDA input) or, with ``out="device"``, ``DeviceArray``s; with ``return_probabilities``
    the float32 combined probabilities are a second result.
    """
    from .models.unet import HipSegmenter

    ps, s = check_tiling_args(patch_size, stride, views, combine, edge)
    if not isinstance(batch_size, (int, np.integer)) or batch_size <= 0:
        raise ValueError(f"batch_size must be a positive integer, got {batch_size!r}")
    check_out(out)
    shape, dt = _complex_input(data, "predict_flags")
    if len(shape) not in (3, 4):
        raise ValueError(f"data must be (B, P, C, T) or (P, C, T), got shape {shape}")
    if not isinstance(model, HipSegmenter):
        raise TypeError(f"predict_flags needs a rfi_toolbox_amd segmentation model, got {type(model).__name__}")
    if model.in_channels not in (3, 8) or model.out_channels != 1 or model._out_scale != 1:
        raise ValueError(f"predict_flags needs a model with 3 or 8 input channels and 1 output channel the size of its "
                         f"input, got {type(model).__name__} with {model.in_channels} -> {model.out_channels}")
    pol = model.in_channels == 8
    if not pol and (normalizer is not None or not broadcast_pols):
        raise ValueError("normalizer and broadcast_pols=False belong to models with 8 input channels; a model with 3 "
                         "input channels normalises every patch itself and flags every plane")
    f = _downsampling(model)
    if ps % f:
        raise ValueError(f"patch_size {ps} is not a multiple of {f}, the downsampling factor of {type(model).__name__}")
    tiling = Tiling(ps, s, _EDGE[edge], views)
    args = (int(batch_size), _COMBINE[combine], float(threshold))
    if not pol:
        Cn, Tn = shape[-2], shape[-1]
        n_planes = int(np.prod(shape[:-2], dtype=np.int64))
        ctx = model.ctx
        o = operand(data, ctx, (dt,), "cast")
        flags, fp, omem = _flag_buffer(ctx, shape, out, data)
        prob, pp, _ = result_buffer(ctx, shape, np.float32, out, data) if return_probabilities else (None, None, None)
        if n_planes and Cn and Tn:
            check(lib.rfi_model_predict_flags(model._h, C.c_void_p(o.ptr), o.mem, COMPLEX_CODES[dt], n_planes, Cn, Tn,
                                              C.byref(tiling), *args, C.c_void_p(fp), omem, C.c_void_p(pp) if pp else None, omem))
        del o
        return (_as_bool(flags), prob) if return_probabilities else _as_bool(flags)

    n, Cn, Tn = _pol_shape(shape)
    form = _normalizer_form(normalizer)
    ctx = model.ctx
    o = operand(data, ctx, (dt,), "cast")
    base = shape[:-3] + (Cn, Tn)
    flags, fp, omem = _flag_buffer(ctx, base, out, data)
    prob, pp, _ = result_buffer(ctx, base, np.float32, out, data) if return_probabilities else (None, None, None)
    px = Cn * Tn

    def run(ptr, mem, b0, b1, centre, scale, pairs):
        check(lib.rfi_model_predict_flags_pol(model._h, C.c_void_p(ptr), mem, COMPLEX_CODES[dt], b1 - b0, Cn, Tn, C.byref(tiling),
                                              *args, centre, scale, None if pairs is None else pairs.ctypes.data_as(C.c_void_p),
                                              C.c_void_p(fp + b0 * px), omem, C.c_void_p(pp + 4 * b0 * px) if pp else None, omem))

    if n and px:
        if form[0] == "pair":
            run(o.ptr, o.mem, 0, n, form[1], form[2], None)
        else:           # every group: one upload (host input), its statistics, then the pipeline on the device copy
            for b0, b1 in _sample_groups(n, 4 * px * dt.itemsize):
                group = _group_on_device(o, ctx, b0, b1, (4, Cn, Tn))
                run(group.ptr, DEVICE, b0, b1, 0.0, 1.0, _sample_pairs(normalizer, group))
                del group
    del o
    flags = _as_bool(flags)
    if broadcast_pols:
        flags = _broadcast_pols(ctx, flags, shape)
    return (flags, prob) if return_probabilities else flags


def _patch_table(n, Cn, Tn, ps, s, views, edge):
    """The (N, 4) int32 table (unit, view, row0, col0) of rfi_tiling's patch order for n units of Cn x Tn."""
    def origins(L):
        if L <= ps:
            return [0]
        o = [i * s for i in range(-(-(L - ps) // s) + 1)]
        if edge == "shift":
            o[-1] = L - ps
        return o
    oc, ot = origins(Cn), origins(Tn)
    per = [(v, r0, c0) for v in range(views) for r0 in (ot if v >= 2 else oc) for c0 in (oc if v >= 2 else ot)]
    table = np.empty((n, len(per), 4), dtype=np.int32)
    table[:, :, 0] = np.arange(n, dtype=np.int32)[:, None]
    table[:, :, 1:] = np.asarray(per, dtype=np.int32).reshape(-1, 3)
    return table.reshape(-1, 4)


def tile_observation(data, patch_size, stride=None, views=1, edge="pad", normalizer=None, device=None):
    """The network input of every tile of an observation for an 8-channel model, for users who run their own model.

    ``data``: complex ``(B, 4, C, T)`` or ``(4, C, T)`` (NumPy, torch or ``DeviceArray``).  Returns a ``DeviceArray``
    ``(N, ps, ps, 8)`` float32, NHWC, channels RR.re, RR.im, RL.re, ... LL.im, the tiles in ``rfi_tiling`` order
    (baseline, view, tile row, tile column); ``normalizer`` as in ``predict_flags``; a pixel past a view's edge holds
    the normalised value of a zero visibility.  ``stitch_patches`` puts the outputs of these tiles back together."""
    ps, s = check_tiling_args(patch_size, stride, views, "mean", edge)
    shape, dt = _complex_input(data, "tile_observation")
    n, Cn, Tn = _pol_shape(shape)
    form = _normalizer_form(normalizer)
    ctx = context_for(device, data)
    table = _patch_table(n, Cn, Tn, ps, s, views, edge)
    res = ctx.empty((len(table), ps, ps, 8), np.float32)
    if not len(table) or not Cn * Tn:
        return res
    o = operand(data, ctx, (dt,), "cast", to_device=True)
    pairs = None
    if form[0] == "sample":
        pairs = np.concatenate([_sample_pairs(normalizer, _group_on_device(o, ctx, b0, b1, (4, Cn, Tn)))
                                for b0, b1 in _sample_groups(n, 4 * Cn * Tn * dt.itemsize)])
    centre, scale = (form[1], form[2]) if form[0] == "pair" else (0.0, 1.0)
    check(lib.rfi_norm_gather(ctx.handle, C.c_void_p(o.ptr), DEVICE, COMPLEX_CODES[dt], n, Cn, Tn,
                              table.ctypes.data_as(C.c_void_p), len(table), ps, centre, scale,
                              None if pairs is None else pairs.ctypes.data_as(C.c_void_p), C.c_void_p(res.ptr), DEVICE))
    del o
    return res


def stitch_patches(values, channels, times, patch_size, stride=None, views=1, edge="pad", combine="mean", threshold=0.5,
                   logits=True, return_probabilities=False):
    """Per-tile model outputs back to whole planes (``rfi_stitch_patches``): the inverse of ``tile_observation``'s and
    ``predict_flags``' tiling.

    ``values``: float32 ``(N, ps, ps)``, ``(N, ps, ps, 1)`` or ``(N, 1, ps, ps)`` in ``rfi_tiling`` order, logits (read
    as ``sigmoid``) or, with ``logits=False``, probabilities; ``N`` must be a whole number of ``channels x times``
    planes.  Returns bool flags ``(planes, channels, times)`` and, with ``return_probabilities``, the float32 combined
    values: ``DeviceArray``s for a ``DeviceArray``, CUDA tensors for a CUDA tensor, else NumPy arrays."""
    ps, s = check_tiling_args(patch_size, stride, views, combine, edge)
    shape = tuple(int(v) for v in describe(values)[0])
    if len(shape) == 4 and (shape[-1] == 1 or shape[1] == 1):
        shape = shape[:3] if shape[-1] == 1 else (shape[0],) + shape[2:]
    if len(shape) != 3 or shape[1:] != (ps, ps):
        raise ValueError(f"values must be (N, {ps}, {ps}), (N, {ps}, {ps}, 1) or (N, 1, {ps}, {ps}), got {describe(values)[0]}")
    Cn, Tn = int(channels), int(times)
    if Cn <= 0 or Tn <= 0:
        raise ValueError(f"channels and times must be positive, got {channels!r}, {times!r}")
    ppp = tiling_count(Cn, Tn, ps, s, views, edge)
    if shape[0] % ppp:
        raise ValueError(f"{shape[0]} patches are not a whole number of {Cn} x {Tn} planes of {ppp} patches each")
    n_planes = shape[0] // ppp
    ctx = context_for(None, values)
    o = operand(values, ctx, (np.float32,), "cast")
    out = "device" if isinstance(values, DeviceArray) else "host"
    flags, fp, omem = _flag_buffer(ctx, (n_planes, Cn, Tn), out, values)
    prob, pp, _ = result_buffer(ctx, (n_planes, Cn, Tn), np.float32, out, values) if return_probabilities else (None, None, None)
    if n_planes:
        check(lib.rfi_stitch_patches(ctx.handle, C.c_void_p(o.ptr), o.mem, VALUES_LOGITS if logits else VALUES_PROBS, n_planes,
                                     Cn, Tn, C.byref(Tiling(ps, s, _EDGE[edge], views)), _COMBINE[combine], float(threshold),
                                     C.c_void_p(fp), omem, C.c_void_p(pp) if pp else None, omem))
    del o
    return (_as_bool(flags), prob) if return_probabilities else _as_bool(flags)
