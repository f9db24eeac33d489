"""A statistical baseline flagger on the GPU: SumThreshold with a masked smooth background fit and the
scale-invariant-rank (SIR) operator -- the core of the strategy observatories run today (Offringa et al. 2010, MNRAS
405, 155; Offringa, van de Gronde & Roerdink 2012, A&A 539, A95).  It is what a learned model is compared against:

    flags = sumthreshold_flags(vis)                      # vis (B, P, C, T) complex -> bool flags of vis.shape

The reference toolbox takes its statistical flaggers from CASA and has no code for this; the arithmetic is this
project's own and is pinned, operation by operation, in include/rfi_hip.h ("statistical baseline flagger").  Per
(C, T) plane: the magnitude as float32; then ``iterations`` rounds of [median and MAD of the residual over the
unflagged samples -> a ladder of ``levels`` thresholds chi_k = s chi_1 sigma / rho^k for window lengths 2^k -> one
SumThreshold pass along time and one along frequency per window length -> a new background from a masked Gaussian
smooth of the unflagged data], the sensitivity s halving its factor every round down to ``base_sensitivity``; then the
SIR operator with aggressiveness ``sir_eta`` along time and along frequency.  Everything between the upload and the
download happens on the device (csrc/sumthreshold.hip); there is no CPU path.

A Gaussian smooth cannot follow a bandpass that falls off steeply (the simulator's t^8 band edges): about a quarter of
such a plane gets flagged.  Divide the bandpass out first, as an observatory pipeline does.

The other statistical flaggers the reference names are here as well, in the style of CASA's flagdata modes and per
chunk of ``ntime`` time samples: ``tfcrop_flags`` (robust piecewise-polynomial fits along time and frequency after the
bandpass is divided out), ``rflag_flags`` (sliding-window rms along time and deviation from the mean spectrum, exact
medians) and ``extend_flags`` (csrc/casa_flaggers.hip; header section "CASA-style baseline flaggers").
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import COMPLEX_CODES, HOST, VALUE_CODES as _CODES, ExtendConfig, RflagConfig, SumThresholdConfig, TfcropConfig, check, lib
from .runtime import as_pointer, check_out, context_for, describe, is_torch, result_buffer, torch

MAX_AXIS = 1 << 20
MAX_WINDOW = 128


def gaussian_weights(sigma, half) -> np.ndarray:
    """The weight table of one smoothing direction, 2 half + 1 float64 values (the one place it is computed)."""
    sigma, half = float(sigma), int(half)
    return np.exp(-np.arange(-half, half + 1)**2 / (2 * sigma * sigma))


def sir_q(eta) -> int:
    """The integer the SIR operator works with: floor(eta 1024 + 0.5)."""
    return int(np.floor(np.float64(eta) * 1024.0 + 0.5))


# ---------------------------------------------------------------------------------------------- argument checks
def _check_planes(name, x):
    """-> (shape, number of planes) of a (..., C, T) stack."""
    shape = describe(x)[0]
    if len(shape) < 2:
        raise ValueError(f"{name} must have shape (..., C, T) with ndim >= 2, got shape {shape}")
    if not 1 <= shape[-2] <= MAX_AXIS or not 1 <= shape[-1] <= MAX_AXIS:
        raise ValueError(f"{name}: C and T must be in 1 .. 2^20, got {shape[-2]} x {shape[-1]}")
    return shape, int(np.prod(shape[:-2], dtype=np.int64))


def _check_flags(flags, shape):
    fshape, dt = describe(flags)[:2]
    if fshape != shape:
        raise ValueError(f"flags have shape {fshape}, the data {shape}")
    if dt is None or dt not in (np.dtype(np.bool_), np.dtype(np.uint8)):
        raise ValueError(f"flags must be bool or uint8, got {dt}")


def _axis(axis, ndim):
    if axis in (-1, ndim - 1):
        return 1
    if axis in (-2, ndim - 2):
        return 0
    raise ValueError(f"axis must name the time axis (-1) or the frequency axis (-2), got {axis!r}")


def _check_real(name, values):
    _, dt, _, owner = describe(values)
    if dt is None or dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"{name} must be float32 or float64, got {dt}")
    if owner is not None and dt != np.float32:
        raise ValueError(f"a device array of {name} must be float32")


def _doubles(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def _run_stage(fn, inputs, shape, planes, args, result_dtype, device):
    """The shared tail of the three stage functions: fn(context, pointer and memory kind of every (array, dtype) of
    `inputs`, planes, C, T, *args, result pointer, HOST) into a new NumPy array of `shape`."""
    out = np.empty(shape, result_dtype)
    if planes:
        ctx = context_for(device, *(x for x, _ in inputs))
        held = [as_pointer(x, dt, ctx) for x, dt in inputs]
        check(fn(ctx.handle, *(a for p, mem, _ in held for a in (C.c_void_p(p), mem)), planes, shape[-2], shape[-1], *args,
                 C.c_void_p(out.ctypes.data), HOST))
    return out


def _check_data(data, flags, out, codes):
    """-> (shape, number of planes, dtype) after the checks the flaggers share (`flags` may be None)."""
    shape, planes = _check_planes("data", data)
    dt = describe(data)[1]
    if dt is None or dt not in codes:
        raise ValueError(f"data must be one of {', '.join(str(c) for c in codes)}, got {dt}")
    if flags is not None:
        _check_flags(flags, shape)
    check_out(out)
    return shape, planes, dt


def _run_flagger(call, data, dt, flags, shape, planes, out, device):
    """The shared tail of the four flaggers: pointers, the result buffer of `out`, then call(ctx, data pointer and
    memory kind, prior pointer and kind, result pointer and kind)."""
    ctx = context_for(device, data, flags)
    dp, dm, k1 = as_pointer(data, dt, ctx)
    fp, fm, k2 = as_pointer(flags, np.uint8, ctx) if flags is not None else (None, HOST, None)
    res, rp, rm = result_buffer(ctx, shape, np.uint8, out, data)
    if planes:
        check(call(ctx, C.c_void_p(dp), dm, C.c_void_p(fp) if fp else None, fm, C.c_void_p(rp), rm))
    if out == "device":
        res._keep = (k1, k2)             # the inputs may still be read by work in flight: they live as long as the result
        return res
    if is_torch(res):
        ctx.synchronize()
        return res.view(torch.bool)
    return res.view(bool)


# ---------------------------------------------------------------------------------------------- the three stages
def sumthreshold_pass(values, flags, window, threshold, center=0.0, axis=-1, device=None) -> np.ndarray:
    """One SumThreshold pass: ``flags | (the samples of every window of `window` consecutive samples along `axis`
    whose unflagged values v - center sum to more than threshold times their number in absolute value)``.

    ``values`` (..., C, T) real, ``flags`` of the same shape; ``window`` a power of two up to 128 (a window longer than
    the line changes nothing); ``threshold`` and ``center`` scalars or one value per plane.  Returns NumPy bool.
    """
    shape, planes = _check_planes("values", values)
    _check_real("values", values)
    _check_flags(flags, shape)
    if not isinstance(window, (int, np.integer)) or not 1 <= window <= MAX_WINDOW or window & (window - 1):
        raise ValueError(f"window must be a power of two in 1 .. {MAX_WINDOW}, got {window!r}")
    ax = _axis(axis, len(shape))
    try:
        th = np.broadcast_to(np.asarray(threshold, np.float64).reshape(-1), (planes,))
        ce = np.broadcast_to(np.asarray(center, np.float64).reshape(-1), (planes,))
    except ValueError:
        raise ValueError(f"threshold and center must be scalars or hold one value per plane ({planes})") from None
    th, thp = _doubles(th)
    ce, cep = _doubles(ce)
    return _run_stage(lib.rfi_sumthreshold_pass, [(values, np.float32), (flags, np.uint8)], shape, planes,
                      (int(window), ax, thp, cep), np.uint8, device).view(bool)


def masked_gaussian_smooth(values, flags, weights_t, weights_f, device=None) -> np.ndarray:
    """The background fit: per sample the weighted mean of the unflagged samples around it, separable, time direction
    first; 0 where no unflagged sample lies under the window.  ``weights_t`` / ``weights_f``: tables of odd length
    (``gaussian_weights``).  Returns NumPy float32."""
    shape, planes = _check_planes("values", values)
    _check_real("values", values)
    _check_flags(flags, shape)
    wt, wf = np.asarray(weights_t, np.float64), np.asarray(weights_f, np.float64)
    for name, w in (("weights_t", wt), ("weights_f", wf)):
        if w.ndim != 1 or w.size % 2 != 1:
            raise ValueError(f"{name} must be a 1-d table of odd length, got shape {w.shape}")
    wt, wtp = _doubles(wt)
    wf, wfp = _doubles(wf)
    return _run_stage(lib.rfi_masked_smooth, [(values, np.float32), (flags, np.uint8)], shape, planes,
                      (wtp, wt.size // 2, wfp, wf.size // 2), np.float32, device)


def sir_operator(flags, eta, axis=-1, device=None) -> np.ndarray:
    """The scale-invariant rank operator along one axis: a sample ends flagged when it lies in an interval of which
    at least a share 1 - eta is flagged (eta rounded to a multiple of 1/1024).  Returns NumPy bool."""
    shape, planes = _check_planes("flags", flags)
    _check_flags(flags, shape)
    if not 0.0 <= float(eta) < 1.0:
        raise ValueError(f"eta must be in [0, 1), got {eta!r}")
    ax = _axis(axis, len(shape))
    return _run_stage(lib.rfi_sir_operator, [(flags, np.uint8)], shape, planes, (ax, min(sir_q(eta), 1023)), np.uint8,
                      device).view(bool)


# ---------------------------------------------------------------------------------------------- the pipeline
def make_config(iterations=3, levels=7, base_sensitivity=1.0, chi_1=6.0, rho=1.5, smooth_sigma=(2.5, 5.0),
                smooth_half=(10, 15), sir_eta=0.2):
    """-> (SumThresholdConfig, weights_t, weights_f) after the argument checks (no device call)."""
    if not isinstance(iterations, (int, np.integer)) or iterations < 1:
        raise ValueError(f"iterations must be an integer >= 1, got {iterations!r}")
    if iterations > 64:
        raise ValueError(f"iterations must be at most 64, got {iterations!r}")
    if not isinstance(levels, (int, np.integer)) or not 1 <= levels <= 8:
        raise ValueError(f"levels must be an integer in 1 .. 8, got {levels!r}")
    if not float(rho) > 1.0:
        raise ValueError(f"rho must be > 1, got {rho!r}")
    if not float(base_sensitivity) > 0.0 or not float(chi_1) > 0.0:
        raise ValueError("base_sensitivity and chi_1 must be > 0")
    try:
        (st, sf), (ht, hf) = smooth_sigma, smooth_half
    except (TypeError, ValueError):
        raise ValueError("smooth_sigma and smooth_half must be (time, frequency) pairs") from None
    if not (float(st) > 0.0 and float(sf) > 0.0):
        raise ValueError(f"smooth_sigma must be > 0 in both directions, got {smooth_sigma!r}")
    if not all(isinstance(h, (int, np.integer)) and 0 <= h <= MAX_AXIS for h in (ht, hf)):
        raise ValueError(f"smooth_half must hold integers in 0 .. 2^20, got {smooth_half!r}")
    if not 0.0 <= float(sir_eta) < 1.0:
        raise ValueError(f"sir_eta must be in [0, 1), got {sir_eta!r}")
    cfg = SumThresholdConfig(int(iterations), int(levels), float(base_sensitivity), float(chi_1), float(rho), int(ht), int(hf),
                             min(sir_q(sir_eta), 1023), 0)
    return cfg, gaussian_weights(st, ht), gaussian_weights(sf, hf)


def threshold_ladder(sigma, iteration, **config) -> np.ndarray:
    """chi_k, k = 0 .. levels - 1, of one iteration for a noise estimate ``sigma`` (``rfi_sumthreshold_ladder``: the
    function the device evaluates; host only)."""
    cfg, _, _ = make_config(**config)
    out = np.empty(cfg.levels, np.float64)
    check(lib.rfi_sumthreshold_ladder(C.byref(cfg), float(sigma), int(iteration), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def sumthreshold_flags(data, flags=None, iterations=3, levels=7, base_sensitivity=1.0, chi_1=6.0, rho=1.5,
                       smooth_sigma=(2.5, 5.0), smooth_half=(10, 15), sir_eta=0.2, out="host", device=None):
    """Flags of a whole observation from the SumThreshold baseline strategy (module docstring).

    ``data``: ``(..., C, T)``, every leading axis a batch of independent planes; complex64 / complex128 visibilities
    (their magnitude is flagged) or float32 / float64 magnitudes; a NumPy array, a torch CPU or CUDA tensor, or a
    ``DeviceArray``.  ``flags``: optional prior flags of the same shape, bool or uint8 (non-zero == flagged); they
    count as flagged throughout and stay set.  ``smooth_sigma`` / ``smooth_half``: (time, frequency) pairs.

    ``out="host"`` returns bool flags of ``data``'s shape, like ``predict_flags`` (a CUDA tensor for CUDA input, else
    NumPy); ``out="device"`` returns a uint8 ``DeviceArray`` and, with device-resident inputs, only enqueues work.
    """
    shape, planes, dt = _check_data(data, flags, out, _CODES)
    cfg, wt, wf = make_config(iterations, levels, base_sensitivity, chi_1, rho, smooth_sigma, smooth_half, sir_eta)
    wt, wtp = _doubles(wt)
    wf, wfp = _doubles(wf)

    def call(ctx, dp, dm, fp, fm, rp, rm):
        return lib.rfi_sumthreshold_flag(ctx.handle, dp, dm, _CODES[dt], fp, fm, planes, shape[-2], shape[-1], C.byref(cfg), wtp, wfp,
                                         rp, rm)
    return _run_flagger(call, data, dt, flags, shape, planes, out, device)


# ---------------------------------------------------------------------------------------------- CASA-style flaggers
_FITS = {"line": 0, "poly": 1}
_DIMENSIONS = {"freqtime": 0, "timefreq": 1, "time": 2, "freq": 3}
_INT_MAX = (1 << 31) - 1


def _ntime(ntime):
    """None (the whole axis) or an integer >= 1 -> the int32 the library takes."""
    if ntime is None:
        return _INT_MAX
    if isinstance(ntime, (bool, np.bool_)) or not isinstance(ntime, (int, np.integer)) or ntime < 1:
        raise ValueError(f"ntime must be None or an integer >= 1, got {ntime!r}")
    return int(min(ntime, _INT_MAX))


def _non_negative(name, v):
    v = float(v)
    if not 0.0 <= v < float("inf"):
        raise ValueError(f"{name} must be finite and >= 0, got {v!r}")
    return v


def _per_plane(name, v, planes, per, forms):
    """None or float64 (planes * per,) from a scalar, one value per plane or (planes, per) values."""
    if v is None:
        return None
    a = np.asarray(v, np.float64)
    if a.size == 1:
        return np.full(planes * per, a.reshape(()), np.float64)
    if a.size == planes * per and (per == 1 or a.ndim >= 2 or planes == 1):
        return np.ascontiguousarray(a.reshape(planes * per))
    if a.size == planes:
        return np.ascontiguousarray(np.repeat(a.reshape(planes), per))
    raise ValueError(f"{name} must be {forms}, got shape {a.shape}")


def tfcrop_flags(data, flags=None, ntime=None, timecutoff=4.0, freqcutoff=3.0, timefit="line", freqfit="poly", maxnpieces=7,
                 flagdimension="freqtime", out="host", device=None):
    """Flags from a TFCrop-style flagger (CASA flagdata ``mode="tfcrop"``): robust fits along time and frequency.

    ``data``, ``flags``, ``out`` and ``device`` as for ``sumthreshold_flags`` (complex input is flagged on its
    magnitude).  Every plane is cut along time into chunks of ``ntime`` samples (None: the whole axis), and nothing
    crosses a chunk boundary.  Per chunk the mean bandpass over the unflagged samples is fitted robustly along frequency
    and divided out; then every channel is fitted along time (``timefit``, ``timecutoff``) and every time sample along
    frequency (``freqfit``, ``freqcutoff``) in the order ``flagdimension`` ("freqtime": time first, "timefreq", "time",
    "freq").  A fit is "line" or "poly" (a line, then up to ``maxnpieces`` cubic pieces), iterated five times, each time
    rejecting the samples further than cutoff standard deviations of the residuals from it.  The arithmetic is pinned in
    include/rfi_hip.h ("CASA-style baseline flaggers") and is this project's own: results agree with CASA in kind, not
    bit for bit.  CASA's ``usewindowstats`` / ``halfwin`` are not built.  There is no CPU path."""
    shape, planes, dt = _check_data(data, flags, out, _CODES)
    for name, v in (("timefit", timefit), ("freqfit", freqfit)):
        if v not in _FITS:
            raise ValueError(f"{name} must be 'line' or 'poly', got {v!r}")
    if flagdimension not in _DIMENSIONS:
        raise ValueError(f"flagdimension must be one of {', '.join(_DIMENSIONS)}, got {flagdimension!r}")
    if isinstance(maxnpieces, (bool, np.bool_)) or not isinstance(maxnpieces, (int, np.integer)) or maxnpieces < 1:
        raise ValueError(f"maxnpieces must be an integer >= 1, got {maxnpieces!r}")
    cfg = TfcropConfig(_ntime(ntime), _FITS[timefit], _FITS[freqfit], int(min(maxnpieces, _INT_MAX)), _DIMENSIONS[flagdimension], 0,
                       _non_negative("timecutoff", timecutoff), _non_negative("freqcutoff", freqcutoff))

    def call(ctx, dp, dm, fp, fm, rp, rm):
        return lib.rfi_tfcrop_flag(ctx.handle, dp, dm, _CODES[dt], fp, fm, planes, shape[-2], shape[-1], C.byref(cfg), rp, rm)
    return _run_flagger(call, data, dt, flags, shape, planes, out, device)


def rflag_flags(data, flags=None, ntime=None, winsize=3, timedevscale=5.0, freqdevscale=5.0, timedev=None, freqdev=None,
                out="host", device=None):
    """Flags from an RFlag-style flagger (CASA flagdata ``mode="rflag"``), on the real and imaginary parts of complex
    visibilities (real input raises ``ValueError``).

    Per chunk of ``ntime`` samples (None: the whole axis).  Time analysis: per channel the rms of the unflagged samples
    in a sliding window of ``winsize`` (odd) samples; a sample is flagged when the rms of its window exceeds
    ``timedevscale`` times (median + median absolute deviation of the channel's rms values).  Spectral analysis: per time
    sample the deviation of every channel from the mean over the unflagged channels; a sample is flagged when it exceeds
    ``freqdevscale`` times (median + MAD over the chunk of the per-sample rms deviations).  Both read the same input
    flags and their results are ORed.  ``timedev`` replaces median + MAD of the time analysis (a scalar, one value per
    plane or ``(planes, C)`` values), ``freqdev`` that of the spectral analysis (a scalar or one value per plane).
    Medians are exact.  Unlike CASA, no polynomial is fitted to the per-channel thresholds across a spectral window.
    ``data``, ``flags``, ``out`` and ``device`` as for ``sumthreshold_flags``.  There is no CPU path."""
    shape, planes, dt = _check_data(data, flags, out, COMPLEX_CODES)
    if isinstance(winsize, (bool, np.bool_)) or not isinstance(winsize, (int, np.integer)) or winsize < 1 or winsize % 2 == 0:
        raise ValueError(f"winsize must be an odd integer >= 1, got {winsize!r}")
    cfg = RflagConfig(_ntime(ntime), int(min(winsize, _INT_MAX)), _non_negative("timedevscale", timedevscale),
                      _non_negative("freqdevscale", freqdevscale))
    td = _per_plane("timedev", timedev, planes, shape[-2], "a scalar, one value per plane or (planes, C) values")
    fd = _per_plane("freqdev", freqdev, planes, 1, "a scalar or one value per plane")
    tdp = td.ctypes.data_as(C.POINTER(C.c_double)) if td is not None else None
    fdp = fd.ctypes.data_as(C.POINTER(C.c_double)) if fd is not None else None

    def call(ctx, dp, dm, fp, fm, rp, rm):
        return lib.rfi_rflag_flag(ctx.handle, dp, dm, _CODES[dt], fp, fm, planes, shape[-2], shape[-1], C.byref(cfg), tdp, fdp, rp, rm)
    return _run_flagger(call, data, dt, flags, shape, planes, out, device)


def extend_flags(flags, ntime=None, growtime=50.0, growfreq=50.0, growaround=False, flagneartime=False, flagnearfreq=False,
                 out="host", device=None):
    """CASA flagdata ``mode="extend"`` on ``(..., C, T)`` bool or uint8 flags, per chunk of ``ntime`` samples and in this
    order, each step on the result of the one before: ``growaround`` (a sample with more than 4 of its 8 neighbours
    flagged), ``growtime`` (a channel flagged for more than that many per cent of the chunk is flagged for all of it; 100
    switches it off), ``growfreq`` (the same per time sample across the channels), ``flagneartime`` and ``flagnearfreq``
    (the samples one step from a flagged one).  ``out`` and ``device`` as for ``sumthreshold_flags``."""
    shape, planes = _check_planes("flags", flags)
    _check_flags(flags, shape)
    check_out(out)
    for name, v in (("growtime", growtime), ("growfreq", growfreq)):
        if not 0.0 <= float(v) <= 100.0:
            raise ValueError(f"{name} must be in 0 .. 100, got {v!r}")
    cfg = ExtendConfig(_ntime(ntime), int(bool(growaround)), int(bool(flagneartime)), int(bool(flagnearfreq)), float(growtime),
                       float(growfreq))

    def call(ctx, dp, dm, fp, fm, rp, rm):
        return lib.rfi_extend_flags(ctx.handle, dp, dm, planes, shape[-2], shape[-1], C.byref(cfg), rp, rm)
    return _run_flagger(call, flags, np.uint8, None, shape, planes, out, device)
