"""Flagging-quality statistics with the reference's signatures, dict keys and edge-case rules
(rfi_toolbox/evaluation/statistics.py:10-229).

The device computes the raw statistics of a whole array -- count, flagged count, mean, std, median, MAD and max of
ALL elements and of the UNFLAGGED elements -- in ONE call (``flag_statistics``, csrc/flag_stats.hip); the ratios,
``ffi``, ``calcquality`` and the dicts are formed here in Python floats with the reference's formulas.

Values follow NumPy: complex input means ``|z|`` by NumPy's complex-abs rule (L * sqrt(fma(S/L, S/L, 1))) in the
input's precision; float32 and complex64 input stay in float32 (median, ``|x - median|``, the mean of the two middle
values); median, MAD and max are exact; a NaN among a view's values makes its statistics NaN (``np.median``, not
``nanmedian``).  Mean and std are two-pass fp64 sums rounded to float32 at the end for float32-origin data, so they
are at least as accurate as NumPy's float32 pairwise sums (and usually more).
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from .._lib import C64, F32, FS_ALL, FS_CLEAN, FS_MEDIANS, HOST, U8, VALUE_CODES, FlagStats as _Raw, check, lib
from ..runtime import Context, context_for, describe, operand  # noqa: F401  (Context: the tests patch it through this module)

__all__ = ["FlagStats", "flag_statistics", "compute_mad", "compute_statistics", "compute_ffi", "compute_calcquality",
           "print_statistics_comparison"]

FlagStats = namedtuple("FlagStats", "count flagged size mean std median mad max float32")
FlagStats.__doc__ = """Statistics of one view.  count: elements in the view; flagged: flagged elements of the whole
input; size: elements of the input; mean, std, median, mad, max: Python floats (NaN for an empty view, for a view
holding a NaN, and for median/mad when not requested); float32: True for float32 / complex64 input."""

def _stats(data, flags, want, medians, device):
    shape, dt, _, owner = describe(data)
    if dt is None or not (dt in VALUE_CODES or dt.kind in "biu"):
        raise TypeError(f"data must be complex128, complex64, float64, float32, bool or integer, not {dt}")
    n = int(np.prod(shape, dtype=np.int64))
    if flags is not None:
        fshape, fdt = describe(flags)[:2]
        if fdt is None or fdt not in (np.dtype(np.uint8), np.dtype(np.bool_)):
            raise TypeError(f"flags must be bool or uint8, not {fdt}")
        fn = int(np.prod(fshape, dtype=np.int64))
        if fn != n:
            raise ValueError(f"flags has {fn} elements, data has {n}")
    if owner is not None and dt not in VALUE_CODES:
        data = data.numpy()                      # (nothing widens a device array in place: bool and integers come down)
    ctx = context_for(device, data, flags)
    d = operand(data, ctx, tuple(VALUE_CODES), "widen")   # NumPy's median / mean of bool and integer arrays work in float64
    f = operand(flags, ctx, (np.uint8,)) if flags is not None else None
    code = VALUE_CODES[d.dtype]
    a, c = _Raw(), _Raw()
    check(lib.rfi_flag_statistics(ctx.handle, C.c_void_p(d.ptr), d.mem, code, n, C.c_void_p(f.ptr) if f else None, f.mem if f else HOST,
                                  U8, want | (FS_MEDIANS if medians else 0), C.byref(a), C.byref(c)))
    f32 = code in (C64, F32)
    return tuple(FlagStats(int(r.count), int(r.flagged), int(n), float(r.mean), float(r.std), float(r.median),
                           float(r.mad), float(r.max), f32) for r in (a, c))


def flag_statistics(data, flags=None, *, medians=True, device=None):
    """(all, unflagged): the FlagStats of every element and of the unflagged elements, from one device call.

    data: NumPy array, torch CPU / CUDA tensor or DeviceArray of complex128, complex64, float64 or float32 (complex:
    |z|); bool and integer input is widened to float64.  flags: bool or uint8 of as many elements (non-zero ==
    flagged), or None.  medians=False skips the median and MAD (mean, std, max and counts only)."""
    return _stats(data, flags, FS_ALL | FS_CLEAN, medians, device)


def _statistics_dict(s, flagged):
    """compute_statistics' dict from a view; `flagged`: whether flags were given"""
    if s.count == 0:
        return {"mean": np.nan, "median": np.nan, "std": np.nan, "mad": np.nan, "count": 0, "flagged_fraction": 1.0}
    return {"mean": s.mean, "median": s.median, "std": s.std, "mad": s.mad, "count": s.count,
            "flagged_fraction": float(s.flagged / s.size) if flagged else 0.0}


def compute_mad(data):
    """Median absolute deviation of all elements (complex: of |z|), as a NumPy scalar of the data's precision."""
    s = _stats(data, None, FS_ALL, True, None)[0]
    return (np.float32 if s.float32 else np.float64)(s.mad)


def compute_statistics(data, flags=None):
    """dict with keys mean, median, std, mad, count, flagged_fraction of the unflagged elements."""
    s = _stats(data, flags, FS_CLEAN, True, None)[1]
    return _statistics_dict(s, flags is not None)


def _ffi(stats_before, stats_after):
    if np.isnan(stats_after["mad"]) or np.isnan(stats_after["std"]):
        return {"ffi": 0.0, "mad_reduction": 0.0, "std_reduction": 0.0, "flagged_fraction": 1.0}
    mad_reduction = 1.0 - (stats_after["mad"] / stats_before["mad"])
    std_reduction = 1.0 - (stats_after["std"] / stats_before["std"])
    flagged_penalty = stats_after["flagged_fraction"]
    ffi = (0.5 * mad_reduction + 0.5 * std_reduction) * (1.0 - 0.5 * flagged_penalty)
    return {
        "ffi": float(ffi),
        "mad_reduction": float(mad_reduction),
        "std_reduction": float(std_reduction),
        "flagged_fraction": float(flagged_penalty),
    }


def _before_after(data, flags):
    a, c = _stats(data, flags, FS_ALL | FS_CLEAN, True, None)
    return _statistics_dict(a, False), _statistics_dict(c, flags is not None)


def compute_ffi(data, flags):
    """Flagging Fidelity Index: dict with keys ffi, mad_reduction, std_reduction, flagged_fraction.
    A zero MAD or std before flagging raises ZeroDivisionError, as in the reference."""
    return _ffi(*_before_after(data, flags))


def compute_calcquality(data, flags, reference_data=None):
    """calcquality (lower is better) and its components a-d (reference statistics.py:101-196)."""
    if reference_data is None:
        ref, flag = _stats(data, flags, FS_ALL | FS_CLEAN, False, None)
    else:
        ref = _stats(reference_data, None, FS_ALL, False, None)[0]
        flag = _stats(data, flags, FS_CLEAN, False, None)[1]
    ref_stats, flag_stats = _statistics_dict(ref, False), _statistics_dict(flag, flags is not None)

    rmean = ref_stats["mean"]
    rstd = ref_stats["std"]
    fmean = flag_stats["mean"]
    fstd = flag_stats["std"]
    pflag = flag_stats["flagged_fraction"] * 100

    if np.isnan(fmean) or np.isnan(fstd) or rstd < 1e-10:
        return {
            "calcquality": np.inf,
            "sensitivity": np.inf,
            "mean_shift": np.inf,
            "std_shift": np.inf,
            "overflagging_penalty": np.inf,
            "flagged_pct": float(pflag),
            "components": {},
        }

    if ref.count == 0:
        raise ValueError("zero-size array to reduction operation maximum which has no identity")
    # np.max of the reference data is a NumPy scalar of its precision: with float32 data, maxdev, a and calcquality
    # are float32 arithmetic (NumPy's weak Python-float promotion), exactly as in the reference
    rmax = (np.float32 if ref.float32 else np.float64)(ref.max)
    maxdev = (rmax - rmean) / rstd
    fdiff = fmean - rmean
    sdiff = fstd - rstd

    a = abs(abs(maxdev) - 3)
    b = abs(fdiff) / rstd - 1
    c = abs(sdiff) / rstd
    d = max(0, (pflag - 70) / 10)

    calcquality = np.sqrt(a**2 + b**2 + c**2 + d**2)

    return {
        "calcquality": float(calcquality),
        "sensitivity": float(a),
        "mean_shift": float(b),
        "std_shift": float(c),
        "overflagging_penalty": float(d),
        "flagged_pct": float(pflag),
        "components": {
            "rmean": float(rmean),
            "rstd": float(rstd),
            "fmean": float(fmean),
            "fstd": float(fstd),
            "rmax": float(rmax),
            "maxdev": float(maxdev),
            "fdiff": float(fdiff),
            "sdiff": float(sdiff),
        },
    }


def print_statistics_comparison(data, flags):
    """Print before/after statistics and FFI (one device call)."""
    stats_before, stats_after = _before_after(data, flags)
    ffi_metrics = _ffi(stats_before, stats_after)

    print("\n" + "=" * 60)
    print("Statistics Comparison (Before/After Flagging)")
    print("=" * 60)

    print("\nBefore Flagging:")
    print(f"  Mean:   {stats_before['mean']:.4e}")
    print(f"  Median: {stats_before['median']:.4e}")
    print(f"  Std:    {stats_before['std']:.4e}")
    print(f"  MAD:    {stats_before['mad']:.4e}")
    print(f"  Count:  {stats_before['count']}")

    print(f"\nAfter Flagging ({stats_after['flagged_fraction']*100:.2f}% flagged):")
    print(f"  Mean:   {stats_after['mean']:.4e}")
    print(f"  Median: {stats_after['median']:.4e}")
    print(f"  Std:    {stats_after['std']:.4e}")
    print(f"  MAD:    {stats_after['mad']:.4e}")
    print(f"  Count:  {stats_after['count']}")

    print("\nFlagging Fidelity Index (FFI):")
    print(f"  FFI:            {ffi_metrics['ffi']:.4f}")
    print(f"  MAD Reduction:  {ffi_metrics['mad_reduction']:.4f}")
    print(f"  STD Reduction:  {ffi_metrics['std_reduction']:.4f}")
