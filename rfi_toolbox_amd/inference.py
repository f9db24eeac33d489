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

from ._lib import (COMBINE_MAX, COMBINE_MEAN, COMPLEX_CODES, DEVICE, EDGE_PAD, EDGE_SHIFT, VALID_FLAGS_BASELINE, VALID_FLAGS_POL, VALUES_LOGITS,
                   VALUES_PROBS, Tiling, check, lib)
from .runtime import DeviceArray, check_out, context_for, describe, is_torch, operand, result_buffer, torch

__all__ = ["predict_flags", "tile_observation", "tile_labels", "stitch_patches", "tiling_count", "tiling_table", "check_tiling_args",
           "stitch_instances", "detect_observation"]

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


def tiling_table(n_units, channels, times, patch_size, stride=None, views=1, edge="pad") -> np.ndarray:
    """The (N, 4) int32 table (unit, view, row0, col0) of ``rfi_tiling``'s patch order for ``n_units`` planes of
    channels x times (``rfi_tiling_table``; host only)."""
    ps, s = check_tiling_args(patch_size, stride, views, "mean", edge)
    tiling = Tiling(ps, s, _EDGE[edge], views)
    Cn, Tn = int(channels), int(times)
    ppp = tiling_count(max(Cn, 1), max(Tn, 1), ps, s, views, edge)       # (an empty axis has one origin, like an axis of 1)
    table = np.empty((int(n_units) * ppp, 4), dtype=np.int32)
    check(lib.rfi_tiling_table(Cn, Tn, C.byref(tiling), int(n_units), table.ctypes.data_as(C.c_void_p), len(table)))
    return table


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


def _sample_pairs(normalizer, group, flags=None):
    """(len(group), 2) float64 (centre, scale) of every baseline of the DeviceArray `group` by its own statistics: what
    ``Normalizer(method, "sample").fit(group, flags=flags)`` keeps.  Without `flags` it raises ValueError on non-finite
    input; with them (the group's prior flags or "nonfinite") the invalid visibilities are left out."""
    from .preprocessing.normalization import sample_parameters
    stats = normalizer.statistics(group, quantiles=normalizer.method == "robust_scale", flags=flags)
    return np.ascontiguousarray([sample_parameters(normalizer.method, st) for st in stats], dtype=np.float64).reshape(-1, 2)


def _prior_flags(flags, shape, n, Cn, Tn):
    """-> (form, array or None) of the `flags` argument of an 8-channel call on data of `shape`: VALID_FLAGS_POL for
    flags of the data's shape, VALID_FLAGS_BASELINE for flags without the polarisation axis, (0, None) for "nonfinite".
    ValueError / TypeError otherwise; no device is touched."""
    if isinstance(flags, str):
        if flags != "nonfinite":
            raise ValueError(f"flags must be an array of prior flags or the string 'nonfinite', got {flags!r}")
        return VALID_FLAGS_POL, None
    got, fdt = describe(flags)[:2]
    got = tuple(int(v) for v in got)
    if fdt is None or fdt not in (np.dtype(np.uint8), np.dtype(np.bool_)):
        raise TypeError(f"flags must be uint8 or bool, not {fdt}")
    if got == tuple(shape):
        return VALID_FLAGS_POL, flags
    if got == tuple(shape[:-3]) + (Cn, Tn):
        return VALID_FLAGS_BASELINE, flags
    raise ValueError(f"flags must have the data's shape {tuple(shape)} (per polarisation) or {tuple(shape[:-3]) + (Cn, Tn)} (per "
                     f"baseline), got shape {got}")


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
                  edge="pad", return_probabilities=False, normalizer=None, broadcast_pols=True, out="host", flags=None, fill=0.0):
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
      A model with class-bit targets (``set_targets("class_bits")``) and K = 2 .. 8 output channels gives flags
      ``(B, K, C, T)`` / ``(K, C, T)``, one plane per class from the same tiling, combine rule and scalar ``threshold``,
      and probabilities of that shape; ``broadcast_pols`` does not apply to it and raises when passed as False.

    ``flags`` (8 input channels only): the observation's prior flags, uint8 or bool, of ``data``'s shape (per
    polarisation) or without the polarisation axis (per baseline: all four), e.g. ``MSLoader.load_flags()``; or the string
    ``"nonfinite"``.  A visibility is then invalid when its prior flag is set or its real or imaginary part is
    non-finite: it is left out of a sample-scope normalizer's statistics (``rfi_valid_statistics``) and enters the network
    as ``fill`` (float32, normalised units).  The probabilities are the model's on that input.  With ``broadcast_pols``
    and one output channel the returned flags are ``model_flags[b] | invalid[b, p]``: a prior-flagged or non-finite
    visibility comes back flagged.  With ``broadcast_pols=False``, or a class-bit model with K > 1, the returned flags
    are the model's alone.  With ``flags=None`` nothing changes: non-finite input raises ``ValueError`` with a
    sample-scope normalizer and spreads through the network's receptive field otherwise.

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
    pol = model.in_channels == 8
    K = model.out_channels
    by_class = pol and getattr(model, "targets", "map") == "class_bits"       # its channels are classes of their own
    if model.in_channels not in (3, 8) or not 1 <= K <= (8 if by_class else 1) or model._out_scale != 1:
        raise ValueError(f"predict_flags needs a model with 3 or 8 input channels and 1 output channel the size of its input, or "
                         f"with 8 input channels, class-bit targets and up to 8 output channels, got {type(model).__name__} "
                         f"with {model.in_channels} -> {K} and {getattr(model, 'targets', 'map')!r} targets")
    if K > 1 and not broadcast_pols:
        raise ValueError("broadcast_pols does not apply to a model with several output channels: its flags are (B, K, C, T)")
    if not pol and (normalizer is not None or not broadcast_pols):
        raise ValueError("normalizer and broadcast_pols=False belong to models with 8 input channels; a model with 3 "
                         "input channels normalises every patch itself and flags every plane")
    if not pol and flags is not None:
        raise ValueError("flags belong to models with 8 input channels; a model with 3 input channels takes no prior flags")
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
    valid = flags is not None
    fform, prior = _prior_flags(flags, shape, n, Cn, Tn) if valid else (0, None)
    ctx = model.ctx
    o = operand(data, ctx, (dt,), "cast")
    base = shape[:-3] + ((Cn, Tn) if K == 1 else (K, Cn, Tn))
    flags, fp, omem = _flag_buffer(ctx, base, out, data)
    prob, pp, _ = result_buffer(ctx, base, np.float32, out, data) if return_probabilities else (None, None, None)
    px = Cn * Tn
    opx = K * px                # output elements per sample

    def run(ptr, mem, b0, b1, centre, scale, pairs):
        check(lib.rfi_model_predict_flags_pol(model._h, C.c_void_p(ptr), mem, COMPLEX_CODES[dt], b1 - b0, Cn, Tn, C.byref(tiling),
                                              *args, centre, scale, None if pairs is None else pairs.ctypes.data_as(C.c_void_p),
                                              C.c_void_p(fp + b0 * opx), omem, C.c_void_p(pp + 4 * b0 * opx) if pp else None, omem))

    if valid:                   # the validity-aware pipeline: prior flags and non-finite values (rfi_model_predict_flags_valid)
        fo = None if prior is None else operand(prior, ctx, (np.uint8,))
        fshape = (Cn, Tn) if fform == VALID_FLAGS_BASELINE else (4, Cn, Tn)
        fpx = px if fform == VALID_FLAGS_BASELINE else 4 * px
        merge = broadcast_pols and K == 1
        merged, mp, _ = _flag_buffer(ctx, shape, out, data) if merge else (None, None, None)
        fill = float(np.float32(fill))

        def run_valid(ptr, mem, fptr, fmem, b0, b1, centre, scale, pairs):
            check(lib.rfi_model_predict_flags_valid(
                model._h, C.c_void_p(ptr), mem, COMPLEX_CODES[dt], b1 - b0, Cn, Tn, C.byref(tiling), *args, centre, scale,
                None if pairs is None else pairs.ctypes.data_as(C.c_void_p), C.c_void_p(fptr) if fptr else None, fmem, fform, fill,
                C.c_void_p(fp + b0 * opx), omem, C.c_void_p(pp + 4 * b0 * opx) if pp else None, omem,
                C.c_void_p(mp + 4 * b0 * px) if merge else None, omem))

        if n and px:
            if form[0] == "pair":
                run_valid(o.ptr, o.mem, fo.ptr if fo else None, fo.mem if fo else DEVICE, 0, n, form[1], form[2], None)
            else:
                for b0, b1 in _sample_groups(n, 4 * px * dt.itemsize):
                    group = _group_on_device(o, ctx, b0, b1, (4, Cn, Tn))
                    gflags = None if fo is None else _group_on_device(fo, ctx, b0, b1, fshape)
                    pairs = _sample_pairs(normalizer, group, "nonfinite" if gflags is None else gflags)
                    run_valid(group.ptr, DEVICE, gflags.ptr if gflags is not None else None, DEVICE, b0, b1, 0.0, 1.0, pairs)
                    del group, gflags
        del o, fo
        flags = _as_bool(merged if merge else flags)
        return (flags, prob) if return_probabilities else flags

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
    if broadcast_pols and K == 1:
        flags = _broadcast_pols(ctx, flags, shape)
    return (flags, prob) if return_probabilities else flags


def tile_observation(data, patch_size, stride=None, views=1, edge="pad", normalizer=None, device=None, flags=None, fill=0.0):
    """The network input of every tile of an observation for an 8-channel model, for users who run their own model.

    ``data``: complex ``(B, 4, C, T)`` or ``(4, C, T)`` (NumPy, torch or ``DeviceArray``).  Returns a ``DeviceArray``
    ``(N, ps, ps, 8)`` float32, NHWC, channels RR.re, RR.im, RL.re, ... LL.im, the tiles in ``rfi_tiling`` order
    (baseline, view, tile row, tile column); ``normalizer`` as in ``predict_flags``; a pixel past a view's edge holds
    the normalised value of a zero visibility.  ``stitch_patches`` puts the outputs of these tiles back together.

    ``flags`` and ``fill`` as in ``predict_flags``: invalid visibilities (prior flag set, or a non-finite part) are left
    out of a sample-scope normalizer's statistics and written as ``fill`` (``rfi_valid_gather``); the pixels past a
    view's edge stay what they are and count as valid."""
    ps, s = check_tiling_args(patch_size, stride, views, "mean", edge)
    shape, dt = _complex_input(data, "tile_observation")
    n, Cn, Tn = _pol_shape(shape)
    form = _normalizer_form(normalizer)
    fform, prior = _prior_flags(flags, shape, n, Cn, Tn) if flags is not None else (0, None)
    ctx = context_for(device, data)
    table = tiling_table(n, Cn, Tn, ps, s, views, edge)
    res = ctx.empty((len(table), ps, ps, 8), np.float32)
    if not len(table) or not Cn * Tn:
        return res
    o = operand(data, ctx, (dt,), "cast", to_device=True)
    fo = None if prior is None else operand(prior, ctx, (np.uint8,), to_device=True)
    fshape = (Cn, Tn) if fform == VALID_FLAGS_BASELINE else (4, Cn, Tn)
    pairs = None
    if form[0] == "sample":
        pairs = np.concatenate([_sample_pairs(normalizer, _group_on_device(o, ctx, b0, b1, (4, Cn, Tn)),
                                              None if flags is None else
                                              ("nonfinite" if fo is None else _group_on_device(fo, ctx, b0, b1, fshape)))
                                for b0, b1 in _sample_groups(n, 4 * Cn * Tn * dt.itemsize)])
    centre, scale = (form[1], form[2]) if form[0] == "pair" else (0.0, 1.0)
    if flags is None:
        check(lib.rfi_norm_gather(ctx.handle, C.c_void_p(o.ptr), DEVICE, COMPLEX_CODES[dt], n, Cn, Tn,
                                  table.ctypes.data_as(C.c_void_p), len(table), ps, centre, scale,
                                  None if pairs is None else pairs.ctypes.data_as(C.c_void_p), C.c_void_p(res.ptr), DEVICE))
    else:
        check(lib.rfi_valid_gather(ctx.handle, C.c_void_p(o.ptr), DEVICE, COMPLEX_CODES[dt], n, Cn, Tn,
                                   table.ctypes.data_as(C.c_void_p), len(table), ps, centre, scale,
                                   None if pairs is None else pairs.ctypes.data_as(C.c_void_p),
                                   None if fo is None else C.c_void_p(fo.ptr), DEVICE, fform, float(np.float32(fill)),
                                   C.c_void_p(res.ptr), DEVICE))
    del o, fo
    return res


def tile_labels(labels, patch_size, stride=None, views=1, edge="pad", invalid=None, invalid_rule="any", pad="ignore", device=None):
    """The label planes of an observation cut into the tiles ``tile_observation`` cuts the data into, for training with
    ``model.set_ignore(True)`` (``rfi_label_gather``).

    ``labels``: ``(B, C, T)`` or ``(C, T)`` uint8 or bool (NumPy, torch or ``DeviceArray``), a map or class bits, one
    plane per baseline.  ``invalid``: None, or non-zero where a visibility is invalid, per polarisation ``(B, 4, C, T)`` --
    ``preprocessing.invalid_map(data, flags)`` -- or per baseline ``(B, C, T)``; such a pixel's byte gets bit 7
    (``class_labels.IGNORE``).  ``invalid_rule``: a pixel is invalid when ``"any"`` or ``"all"`` of its four polarisations
    are.  ``pad``: what a pixel past a view's edge holds (``edge="pad"``): ``"ignore"`` 0x80, ``"zero"`` 0.  Returns a
    ``DeviceArray`` ``(N, ps, ps)`` uint8 in ``rfi_tiling`` order: row i is the label of ``tile_observation``'s row i."""
    ps, s = check_tiling_args(patch_size, stride, views, "mean", edge)
    if invalid_rule not in ("any", "all"):
        raise ValueError(f"invalid_rule must be 'any' or 'all', got {invalid_rule!r}")
    if pad not in ("ignore", "zero"):
        raise ValueError(f"pad must be 'ignore' or 'zero', got {pad!r}")
    shape, dt = describe(labels)[:2]
    shape = tuple(int(v) for v in shape)
    if dt is None or dt not in (np.dtype(np.uint8), np.dtype(np.bool_)):
        raise TypeError(f"labels must be uint8 or bool, not {dt}")
    if len(shape) not in (2, 3):
        raise ValueError(f"labels must be (B, C, T) or (C, T), got shape {shape}")
    n, Cn, Tn = (shape[0] if len(shape) == 3 else 1), shape[-2], shape[-1]
    form = VALID_FLAGS_POL
    if invalid is not None:
        got, idt = describe(invalid)[:2]
        got = tuple(int(v) for v in got)
        if idt is None or idt not in (np.dtype(np.uint8), np.dtype(np.bool_)):
            raise TypeError(f"invalid must be uint8 or bool, not {idt}")
        if got in ((n, 4, Cn, Tn), (n, 4, Cn * Tn)) or (len(shape) == 2 and got == (4, Cn, Tn)):
            form = VALID_FLAGS_POL
        elif got == shape or got == (n, Cn, Tn):
            form = VALID_FLAGS_BASELINE
        else:
            raise ValueError(f"invalid must be per polarisation {(n, 4, Cn, Tn)} or per baseline {(n, Cn, Tn)}, got shape {got}")
    ctx = context_for(device, labels, invalid)
    table = tiling_table(n, Cn, Tn, ps, s, views, edge)
    res = ctx.empty((len(table), ps, ps), np.uint8)
    if not len(table) or not Cn * Tn:
        return res
    o = operand(labels, ctx, (np.uint8,), to_device=True)
    io = None if invalid is None else operand(invalid, ctx, (np.uint8,), to_device=True)
    check(lib.rfi_label_gather(ctx.handle, C.c_void_p(o.ptr), DEVICE, n, Cn, Tn, None if io is None else C.c_void_p(io.ptr), DEVICE,
                               form, 1 if invalid_rule == "all" else 0, table.ctypes.data_as(C.c_void_p), len(table), ps,
                               0x80 if pad == "ignore" else 0, C.c_void_p(res.ptr), DEVICE))
    if any(is_torch(k.keep) or k.keep is not x for k, x in ((o, labels), (io, invalid)) if k is not None):
        ctx.synchronize()                 # (an uploaded or converted copy goes with this frame)
    del o, io
    return res


def stitch_patches(values, channels, times, patch_size, stride=None, views=1, edge="pad", combine="mean", threshold=0.5,
                   logits=True, return_probabilities=False):
    """Per-tile model outputs back to whole planes (``rfi_stitch_patches``): the inverse of ``tile_observation``'s and
    ``predict_flags``' tiling.

    ``values``: float32 ``(N, ps, ps)``, ``(N, ps, ps, 1)`` or ``(N, 1, ps, ps)`` in ``rfi_tiling`` order, logits (read
    as ``sigmoid``) or, with ``logits=False``, probabilities; ``N`` must be a whole number of ``channels x times``
    planes.  Returns bool flags ``(planes, channels, times)`` and, with ``return_probabilities``, the float32 combined
    values: ``DeviceArray``s for a ``DeviceArray``, CUDA tensors for a CUDA tensor, else NumPy arrays.

    ``values`` of ``(N, ps, ps, K)`` with K > 1 -- the channel-last output of a K-class model -- are stitched class by
    class: flags ``(planes, K, channels, times)``, and the probabilities likewise."""
    ps, s = check_tiling_args(patch_size, stride, views, combine, edge)
    shape = tuple(int(v) for v in describe(values)[0])
    K = None
    if len(shape) == 4 and (shape[-1] == 1 or shape[1] == 1):
        shape = shape[:3] if shape[-1] == 1 else (shape[0],) + shape[2:]
    elif len(shape) == 4 and shape[1:3] == (ps, ps):
        shape, K = shape[:3], shape[3]
    if len(shape) != 3 or shape[1:] != (ps, ps):
        raise ValueError(f"values must be (N, {ps}, {ps}), (N, {ps}, {ps}, K) or (N, 1, {ps}, {ps}), got {describe(values)[0]}")
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
    oshape = (n_planes, Cn, Tn) if K is None else (n_planes, K, Cn, Tn)
    flags, fp, omem = _flag_buffer(ctx, oshape, out, values)
    prob, pp, _ = result_buffer(ctx, oshape, np.float32, out, values) if return_probabilities else (None, None, None)
    if n_planes:
        check(lib.rfi_stitch_patches_classes(ctx.handle, C.c_void_p(o.ptr), o.mem, VALUES_LOGITS if logits else VALUES_PROBS,
                                             n_planes, K or 1, Cn, Tn, C.byref(Tiling(ps, s, _EDGE[edge], views)),
                                             _COMBINE[combine], float(threshold), C.c_void_p(fp), omem,
                                             C.c_void_p(pp) if pp else None, omem))
    del o
    return (_as_bool(flags), prob) if return_probabilities else _as_bool(flags)


# ---------------------------------------------------------------------------------------------- instances of a whole observation
_STITCH_BYTES = 1 << 30               # tile masks plus outputs of one chunk of detect_observation (predict_flags' bound)
_STITCH_MAX_SLOTS = 65536             # patches per plane x D: the ranking sorts one segment per plane


def _check_stitch_args(max_events, min_area, min_score, connectivity, out):
    if not isinstance(max_events, (int, np.integer)) or not 1 <= max_events <= 256:
        raise ValueError(f"max_events must be an integer in 1 .. 256, got {max_events!r}")
    if not isinstance(min_area, (int, np.integer)) or min_area < 1:
        raise ValueError(f"min_area must be an integer of at least 1, got {min_area!r}")
    if not isinstance(min_score, (int, float, np.integer, np.floating)) or not np.isfinite(min_score):
        raise ValueError(f"min_score must be a finite number, got {min_score!r}")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    check_out(out)


def _check_plane(channels, times, ps, s, views, edge, D):
    """-> (C, T, patches per plane) of a stitch; ValueError for a plane the kernels do not take."""
    if not isinstance(channels, (int, np.integer)) or not isinstance(times, (int, np.integer)) or channels <= 0 or times <= 0:
        raise ValueError(f"channels and times must be positive integers, got {channels!r}, {times!r}")
    Cn, Tn = int(channels), int(times)
    if Cn * Tn >= 1 << 31:
        raise ValueError(f"planes of fewer than 2^31 pixels, got {Cn} x {Tn}")
    ppp = tiling_count(Cn, Tn, ps, s, views, edge)
    if ppp * D > _STITCH_MAX_SLOTS:
        raise ValueError(f"{ppp} patches per plane x {D} detection slots exceed {_STITCH_MAX_SLOTS}: use a larger stride, fewer "
                         "views or a smaller max_det")
    return Cn, Tn, ppp


def _run_stitch(ctx, ptrs, n_planes, Cn, Tn, tiling, D, E, min_area, min_score, class_aware, connectivity, res, plane0=0):
    """rfi_stitch_instances on device pointers `ptrs` (boxes, scores, labels, counts, masks) into the result dict `res`
    from its plane `plane0` on."""
    off = lambda k, per: C.c_void_p(res[k].ptr + plane0 * per * res[k].dtype.itemsize)  # noqa: E731
    check(lib.rfi_stitch_instances(ctx.handle, *[C.c_void_p(p) for p in ptrs], n_planes, Cn, Tn, C.byref(tiling), D, E, int(min_area),
                                   float(min_score), 1 if class_aware else 0, int(connectivity), off("boxes", E * 4), off("scores", E),
                                   off("labels", E), off("counts", 1), off("rfi_mask", Cn * Tn),
                                   off("masks", E * Cn * Tn) if "masks" in res else None))


def _stitch_result(ctx, n_planes, E, Cn, Tn, instance_masks):
    res = {"boxes": ctx.empty((n_planes, E, 4), np.float32), "scores": ctx.empty((n_planes, E), np.float32),
           "labels": ctx.empty((n_planes, E), np.int32), "counts": ctx.empty((n_planes,), np.int32),
           "rfi_mask": ctx.empty((n_planes, Cn, Tn), np.uint8)}
    if instance_masks:
        res["masks"] = ctx.empty((n_planes, E, Cn, Tn), np.uint8)
    return res


def _events_to_host(res, n_planes):
    """The device dict of a stitch -> ``predict``'s list of dicts, one per plane."""
    cnt, boxes, scores, labels = (res[k].numpy() for k in ("counts", "boxes", "scores", "labels"))
    rfi = res["rfi_mask"].numpy().astype(bool)
    masks = res["masks"].numpy() if "masks" in res else None
    items = []
    for i in range(n_planes):
        k = int(cnt[i])
        o = {"boxes": boxes[i, :k].copy(), "scores": scores[i, :k].copy(), "labels": labels[i, :k].astype(np.int64)}
        if masks is not None:
            o["masks"] = masks[i, :k].astype(bool)
        o["rfi_mask"] = rfi[i]
        items.append(o)
    return items


def stitch_instances(detections, channels, times, patch_size, stride=None, views=1, edge="pad", max_events=64, min_area=1,
                     min_score=0.0, class_aware=True, connectivity=8, instance_masks=True, out="device"):
    """Per-tile detections back to whole planes (``rfi_stitch_instances``): one event per emitter, the instance
    counterpart of ``stitch_patches``, for tiles from any detector.

    ``detections``: the dict of ``MaskRCNN.detect(out="device")`` over the ``N`` tiles of whole ``channels x times``
    planes in ``rfi_tiling`` order (``DeviceArray``s, NumPy arrays or torch tensors; boxes ``(N, D, 4)`` xyxy in tile
    coordinates, scores, labels, counts, masks ``(N, D, ps, ps)``), or the list of dicts of ``predict``, padded and
    uploaded once.  The rules are pinned in include/rfi_hip.h ("instance stitch"): a slot with ``score >= min_score`` and
    at least ``min_area`` mask pixels inside the plane is a member; members of different tiles (with ``class_aware``: of
    one label) are linked when their masks share a pixel where the tiles overlap, or touch (``connectivity`` 8 or 4)
    where the tiles only abut; an event is a connected set of members with the OR of their masks, the union of their
    mapped boxes, their best score and its label.  The link test is boolean: two emitters of one class that touch across
    a seam, or cross inside an overlap, merge.

    ``out="device"``: a dict of ``DeviceArray``s in ``detect``'s layout, so ``match_instances`` and
    ``DetectionScorer.update`` take it unchanged -- boxes ``(P, max_events, 4)``, scores, labels (int32), counts ``(P,)``,
    rfi_mask ``(P, C, T)`` uint8 and, with ``instance_masks``, masks ``(P, max_events, C, T)`` uint8; events by
    descending score, zero behind ``counts``.  ``rfi_mask`` is the OR of all members, whether or not ``max_events`` cut
    their event: the flags do not depend on the cap.  ``out="host"``: ``predict``'s list of dicts, one per plane."""
    from .evaluation.detection import _detections
    ps, s = check_tiling_args(patch_size, stride, views, "mean", edge)
    _check_stitch_args(max_events, min_area, min_score, connectivity, out)
    side = _detections(detections)
    if side.masks is None:
        raise ValueError("stitch_instances needs the instance masks of the tiles (detect(instance_masks=True))")
    if tuple(side.shape) != (ps, ps):
        raise ValueError(f"the tile masks must be {ps} x {ps}, got {tuple(side.shape)}")
    D = max(1, side.slots)
    Cn, Tn, ppp = _check_plane(channels, times, ps, s, views, edge, D)
    if side.n % ppp:
        raise ValueError(f"{side.n} tiles are not a whole number of {Cn} x {Tn} planes of {ppp} patches each")
    n_planes, E = side.n // ppp, int(max_events)
    arrays = [side.boxes, side.scores, side.labels, side.count, side.masks]
    if side.slots == 0:          # (lists without a detection: one empty slot per tile)
        arrays = [np.zeros((side.n, 1, 4), np.float32), np.zeros((side.n, 1), np.float32), np.zeros((side.n, 1), np.int32),
                  np.zeros((side.n,), np.int32), np.zeros((side.n, 1, ps, ps), np.uint8)]
    ctx = context_for(None, *arrays)
    res = _stitch_result(ctx, n_planes, E, Cn, Tn, instance_masks)
    if n_planes:
        ops = [operand(a, ctx, (dt,), "cast", to_device=True)
               for a, dt in zip(arrays, (np.float32, np.float32, np.int32, np.int32, np.uint8))]
        _run_stitch(ctx, [o.ptr for o in ops], n_planes, Cn, Tn, Tiling(ps, s, _EDGE[edge], views), D, E, min_area, min_score,
                    class_aware, connectivity, res)
        if out == "host" or any(o.keep is not a for o, a in zip(ops, arrays)):
            ctx.synchronize()    # (uploaded copies are dropped on return)
        del ops
    return res if out == "device" else _events_to_host(res, n_planes)


def detect_observation(detector, data, patch_size=128, stride=None, views=1, edge="pad", normalizer=None, batch_size=64,
                       max_events=64, min_area=1, min_score=0.0, class_aware=True, connectivity=8, instance_masks=False,
                       out="host"):
    """The events of a whole observation from a ``MaskRCNN`` with 8 input channels: tile, detect, stitch.

    ``data``: complex ``(B, 4, C, T)`` or ``(4, C, T)`` visibilities in the order RR, RL, LR, LL, as in ``predict_flags``;
    ``normalizer`` has its three forms.  The observation is streamed through in chunks of whole baselines: the tiles
    of a chunk are cut and normalised on the GPU (``tile_observation``'s gather), ``detector.detect`` runs on them in
    batches of ``batch_size`` tiles, and one ``stitch_instances`` per chunk joins the pieces of every emitter (its
    rules, arguments and boolean-link limit apply).  Returns one plane of events per baseline in ``stitch_instances``'
    two forms.  ``rfi_mask`` does not depend on ``max_events``."""
    from .models.mask_rcnn import MaskRCNN
    ps, s = check_tiling_args(patch_size, stride, views, "mean", edge)
    _check_stitch_args(max_events, min_area, min_score, connectivity, out)
    if not isinstance(batch_size, (int, np.integer)) or batch_size <= 0:
        raise ValueError(f"batch_size must be a positive integer, got {batch_size!r}")
    if not isinstance(detector, MaskRCNN):
        raise TypeError(f"detect_observation needs a rfi_toolbox_amd MaskRCNN, got {type(detector).__name__}")
    if detector.backbone.in_channels != 8:
        raise ValueError(f"detect_observation needs a detector with 8 input channels, got {detector.backbone.in_channels}: run "
                         "a detector of another input on tiles of your own and join its detections with stitch_instances")
    shape, dt = _complex_input(data, "detect_observation")
    n, Cn, Tn = _pol_shape(shape)
    form = _normalizer_form(normalizer)
    bs, E, D = int(batch_size), int(max_events), int(detector.max_det)
    detector._check_detect(bs, ps, ps)
    Cn, Tn, ppp = _check_plane(Cn, Tn, ps, s, views, edge, D)
    px = Cn * Tn
    per_plane = ppp * D * (ps * ps + 24) + px * (1 + (E if instance_masks else 0)) + E * 24 + 4
    if per_plane > _STITCH_BYTES:
        raise ValueError(f"one {Cn} x {Tn} plane needs {per_plane} bytes of tile masks and outputs, more than {_STITCH_BYTES}: lower "
                         "max_events, pass instance_masks=False, or use a larger stride or a smaller max_det")
    chunk = max(1, min(n, _STITCH_BYTES // per_plane))
    tiling = Tiling(ps, s, _EDGE[edge], views)
    ctx = detector.backbone.ctx
    full = out == "device"                       # the device result holds every plane; the host form is read back per chunk
    res = _stitch_result(ctx, n if full else chunk, E, Cn, Tn, instance_masks)
    items = []
    if not n:
        return res if full else items
    o = operand(data, ctx, (dt,), "cast")
    nt = chunk * ppp
    tiles = {"boxes": ctx.empty((nt, D, 4), np.float32), "scores": ctx.empty((nt, D), np.float32),
             "labels": ctx.empty((nt, D), np.int32), "counts": ctx.empty((nt,), np.int32), "masks": ctx.empty((nt, D, ps, ps), np.uint8)}
    rows = {"boxes": D * 16, "scores": D * 4, "labels": D * 4, "counts": 4, "masks": D * ps * ps}
    x = ctx.empty((bs, ps, ps, 8), np.float32)
    for b0 in range(0, n, chunk):
        b1 = min(n, b0 + chunk)
        group = _group_on_device(o, ctx, b0, b1, (4, Cn, Tn))
        pairs = None
        if form[0] == "sample":
            go = operand(group, ctx, (dt,))
            pairs = np.concatenate([_sample_pairs(normalizer, _group_on_device(go, ctx, g0, g1, (4, Cn, Tn)))
                                    for g0, g1 in _sample_groups(b1 - b0, 4 * px * dt.itemsize)])
        centre, scale = (form[1], form[2]) if form[0] == "pair" else (0.0, 1.0)
        table = tiling_table(b1 - b0, Cn, Tn, ps, s, views, edge)
        for i0 in range(0, len(table), bs):
            k = min(bs, len(table) - i0)
            if k < bs:
                x.zero_()                        # the last batch is padded with zero tiles; their slots are not copied
            part = np.ascontiguousarray(table[i0:i0 + k])
            check(lib.rfi_norm_gather(ctx.handle, C.c_void_p(group.ptr), DEVICE, COMPLEX_CODES[dt], b1 - b0, Cn, Tn,
                                      part.ctypes.data_as(C.c_void_p), k, ps, centre, scale,
                                      None if pairs is None else pairs.ctypes.data_as(C.c_void_p), C.c_void_p(x.ptr), DEVICE))
            det = detector.detect(x, instance_masks=True, out="device")      # (valid until the next call: copied now)
            for key, w in rows.items():
                check(lib.rfi_op_copy_rows(ctx.handle, C.c_void_p(det[key].ptr), k * w, C.c_void_p(tiles[key].ptr + i0 * w), k * w, k * w, 1))
        _run_stitch(ctx, [tiles[key].ptr for key in ("boxes", "scores", "labels", "counts", "masks")], b1 - b0, Cn, Tn, tiling, D, E,
                    min_area, min_score, class_aware, connectivity, res, b0 if full else 0)
        if not full:
            items += _events_to_host(res, b1 - b0)
        del group
    del o
    return res if full else items
