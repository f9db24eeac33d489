"""NumPy restatement of the validity-aware 8-channel input (include/rfi_hip.h, "validity-aware 8-channel input"),
written from the rules:

* a visibility (one polarisation of one pixel) is INVALID when its prior flag is non-zero or its real or imaginary part
  is non-finite; prior flags are per polarisation (n, 4, T, F) or per baseline (n, T, F);
* the statistics are those of the valid scalars alone: the valid scalars are compacted, then np.min / np.max, the
  sorted array at rfi_norm_bracket's ranks for the population's own valid count, and math.fsum moments;
* the transform is normalize_ref.apply in fp64 with float32 `fill` written into both channels of an invalid visibility;
* the tiles are pol_tiling_ref's cut of the transformed planes: a pixel past a view's edge is the normalised 0 + 0j.

The parameter rules and the comparison helpers are normalize_ref's, the tile cutting pol_tiling_ref's.
"""
import math

import numpy as np

import normalize_ref as nref
import pol_tiling_ref as pref

NAN = float("nan")


def invalid_map(x, flags=None, layout=None):
    """(n, 4, T, F) bool: True where the visibility is invalid.  x: any accepted input; flags (n, 4, T, F), (n, T, F) or None."""
    v = nref.to_nchw(x, layout)
    bad = ~np.isfinite(v[:, 0::2]) | ~np.isfinite(v[:, 1::2])
    if flags is not None:
        f = np.asarray(flags) != 0
        bad = bad | (f[:, None] if f.ndim == 3 else f)
    return bad


def valid_scalars(x, bad, layout=None):
    """The valid scalars of x as one flat fp64 array (both scalars of every valid visibility)."""
    v = nref.to_nchw(x, layout)
    return v[np.repeat(~bad, 2, axis=1)]


def bracket(count, q):
    """rfi_norm_bracket: (lower rank, upper rank, fraction) of quantile q among `count` values, in fp64."""
    v = q * float(count - 1)
    f = math.floor(v)
    return int(f), min(int(f) + 1, count - 1), v - f


def stats(values):
    """The record of one population from its compacted valid scalars."""
    v = np.sort(np.asarray(values, dtype=np.float64).ravel())
    if v.size == 0:
        return {"count": 0, "min": NAN, "max": NAN, "mean": NAN, "var": NAN, "q": ((NAN, NAN),) * 3}
    mean, var = nref.moments(v)
    q = tuple((float(v[lo]), float(v[hi])) for lo, hi, _ in (bracket(v.size, p) for p in (0.5, 0.25, 0.75)))
    return {"count": int(v.size), "min": float(v[0]), "max": float(v[-1]), "mean": mean, "var": var, "q": q}


def sample_stats(x, flags=None, layout=None):
    bad = invalid_map(x, flags, layout)
    return [stats(valid_scalars(x[i:i + 1], bad[i:i + 1], layout)) for i in range(len(x))]


def dataset_stats(chunks, flags=None, layouts=None):
    flags = [None] * len(chunks) if flags is None else flags
    layouts = [None] * len(chunks) if layouts is None else layouts
    return stats(np.concatenate([valid_scalars(c, invalid_map(c, f, l), l) for c, f, l in zip(chunks, flags, layouts)]))


def sample_pairs(x, method, flags=None, layout=None):
    """One (centre, scale) or None (the all-zeros transform; also a sample with no valid scalar) per sample."""
    bad = invalid_map(x, flags, layout)
    out = []
    for i in range(len(x)):
        v = valid_scalars(x[i:i + 1], bad[i:i + 1], layout)
        out.append(None if v.size == 0 else ((0.0, 1.0) if method is None else nref.sample_params(v, method)))
    return out


def dataset_pair(x, method, flags=None, layout=None):
    """-> (attrs, pair or None) of normalize_ref.dataset_params over the valid scalars of x (None too with none valid)."""
    v = valid_scalars(x, invalid_map(x, flags, layout), layout)
    if v.size == 0:
        return None, None
    if method is None:
        return None, (0.0, 1.0)
    return nref.dataset_params([v.reshape(1, 1, 1, -1)], method)        # (any 4-D real array: the rules see its values only)


def transform(x, pairs, flags=None, fill=0.0, layout=None):
    """float32 (n, 8, T, F): sample i by pairs[i], `fill` at both channels of every invalid visibility."""
    v = nref.to_nchw(x, layout)
    bad = np.repeat(invalid_map(x, flags, layout), 2, axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.stack([nref.apply(s, p) for s, p in zip(v, pairs)])
    out[bad] = np.float32(fill)
    return out


def tile(data, pairs, ps, stride=None, views=1, edge="pad", flags=None, fill=0.0):
    """The network input of every tile: the restatement transform of the whole sample, then pol_tiling_ref's cut."""
    return pref.cut_channels(transform(pref.as_samples(data), pairs, flags, fill), pairs, ps, stride, views, edge)
