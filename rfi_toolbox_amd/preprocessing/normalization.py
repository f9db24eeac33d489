"""Input normalisation of 8-channel RFI data on the GPU.

The reference normalises in two places, and both are covered:

* ``scope="dataset"`` follows ``datasets.RFIMaskDataset`` (rfi_mask_dataset.py:99-156): dataset-wide ``global_min``,
  ``global_max``, ``mean``, ``std`` (population std ``+ 1e-8``) and, for ``robust_scale``, ``robust_median`` and
  ``robust_iqr`` (``q75 - q25 + 1e-8``); min-max gives zeros when ``max <= min``.
* ``scope="sample"`` follows ``scripts/normalize_rfi_data.py::normalize_array``: every sample by its own statistics,
  with scikit-learn's rules for near-constant features restated here from the returned scalars (scikit-learn is not
  imported): ``StandardScaler`` divides by 1 when ``var <= n eps var + (n mean eps)**2``, ``RobustScaler`` when
  ``q75 - q25 < 10 eps``.

The device computes, per population, min, max, the fp64 mean and population variance and the two bracketing order
statistics of the median and the quartiles (``rfi_norm_statistics``, csrc/dataset_norm.hip: exact radix selection,
deterministic sums); NumPy's interpolation between the brackets (``_lerp``) and the mean of the two middle values are
formed here in Python floats.  The transform ``float32((float64(x) - centre) / scale)`` runs on the device with the
layout conversion fused (``rfi_norm_apply``) and is stream-ordered: a ``DeviceArray`` in gives a ``DeviceArray`` out
with nothing copied to the host.  NumPy input is uploaded once and the result comes back as NumPy.

Accepted inputs: planar ``(n, 8, T, F)`` or channel-last ``(n, T, F, 8)`` float64 / float32, and complex128 /
complex64 ``(n, 4, T, F)`` in the order RR, RL, LR, LL (channels RR.re, RR.im, ... as ``save_example_pair_npy``).
For float32 / complex64 input the arithmetic is fp64 on the values widened to fp64, not NumPy's float32 arithmetic.

Prior flags and non-finite samples.  ``statistics``, ``fit``, ``transform``, ``fit_transform`` and ``normalize_array``
take ``flags``: prior flags of the visibilities, uint8 or bool (NumPy, torch or ``DeviceArray``), per polarisation
``(n, 4, T, F)`` or per baseline ``(n, T, F)`` (all four polarisations of a pixel); for a list of chunks a list of the
same length; or the string ``"nonfinite"``: no prior flags.  A visibility is then INVALID when its flag is set or its
real or imaginary part (channels ``2p``, ``2p + 1`` of real input) is non-finite.  The statistics are those of the
valid scalars alone (``rfi_valid_statistics``: ``count`` is the valid count, and the quantile brackets come from it); a
population without a valid scalar has ``count`` 0, NaN statistics and the pair ``(0.0, 0.0)``, the all-zeros transform.
``transform`` writes ``fill`` (float32, normalised units, default 0.0) into both channels of an invalid visibility and
today's expression everywhere else (``rfi_valid_apply``).  What ``transform`` calls invalid is decided from the array it
is given, so ``fit`` and ``transform`` may see different flags.

Deviation: with ``flags=None`` input holding a NaN or an infinity raises ``ValueError`` in ``fit``, as before
(scikit-learn skips NaN; the reference's simulated data never has one).  Measured data does: pass its ``FLAG`` column,
or ``flags="nonfinite"``.  ``invalid_map`` hands the same decision out as bytes, for ``inference.tile_labels`` to put
into the label tiles as the ignore bit of ``model.set_ignore(True)``.  Out of scope here: ``detect_observation``, the
3-channel ``Preprocessor`` path and ``RFIMaskDataset``, none of which takes ``flags``.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

__all__ = ["Normalizer", "normalize_array", "invalid_map", "METHODS"]

METHODS = ("global_min_max", "standardize", "robust_scale", None)
_EPS = float(np.finfo(np.float64).eps)
_SCALAR = {np.dtype(np.complex128): np.dtype(np.float64), np.dtype(np.complex64): np.dtype(np.float32),
           np.dtype(np.float64): np.dtype(np.float64), np.dtype(np.float32): np.dtype(np.float32)}


def _describe(x, layout=None):
    """-> (n, pixels, 'nchw' | 'nhwc', (T, F)) of an accepted input; ValueError / TypeError otherwise (host only)."""
    dt = np.dtype(x.dtype)
    shape = tuple(int(s) for s in x.shape)
    if dt not in _SCALAR:
        raise TypeError(f"data must be float64, float32, complex128 or complex64, not {dt}")
    if len(shape) != 4:
        raise ValueError(f"data must be (n, 8, T, F), (n, T, F, 8) or complex (n, 4, T, F), got shape {shape}")
    if layout not in (None, "nchw", "nhwc"):
        raise ValueError(f"layout must be 'nchw', 'nhwc' or None, got {layout!r}")
    if dt.kind == "c":
        if shape[1] != 4 or layout == "nhwc":
            raise ValueError(f"complex data must be (n, 4, T, F) (RR, RL, LR, LL), got shape {shape}")
        return shape[0], shape[2] * shape[3], "nchw", shape[2:]
    first, last = shape[1] == 8, shape[3] == 8
    if layout is None:
        if first and last:
            raise ValueError(f"shape {shape} is ambiguous: pass layout='nchw' or layout='nhwc'")
        layout = "nchw" if first else "nhwc"
    if not (first if layout == "nchw" else last):
        raise ValueError(f"data must have 8 channels ((n, 8, T, F) or (n, T, F, 8)), got shape {shape}")
    tf = shape[2:] if layout == "nchw" else shape[1:3]
    return shape[0], tf[0] * tf[1], layout, tf


def _flags_form(flags, n, tf, what="flags"):
    """-> VALID_FLAGS_POL / VALID_FLAGS_BASELINE of prior flags for `n` samples of planes `tf`, or None for
    ``"nonfinite"``; ValueError / TypeError otherwise (host only: no device is touched)."""
    from .._lib import VALID_FLAGS_BASELINE, VALID_FLAGS_POL
    from ..runtime import describe
    if isinstance(flags, str):
        if flags != "nonfinite":
            raise ValueError(f"{what} must be an array of prior flags or the string 'nonfinite', got {flags!r}")
        return None
    shape, dt = describe(flags)[:2]
    shape = tuple(int(v) for v in shape)
    if dt is None or dt not in (np.dtype(np.uint8), np.dtype(np.bool_)):
        raise TypeError(f"{what} must be uint8 or bool, not {dt}")
    tf = tuple(int(v) for v in tf)
    if shape == (n, 4) + tf:
        return VALID_FLAGS_POL
    if shape == (n,) + tf:
        return VALID_FLAGS_BASELINE
    raise ValueError(f"{what} must be per polarisation {(n, 4) + tf} or per baseline {(n,) + tf}, got shape {shape}")


def _invalid_map(ctx, src, desc, flags, form):
    """The (n, 4, pixels) uint8 invalid map (``rfi_valid_map``) of the device operand `src` described by `desc`; `flags`:
    prior flags in `form`, or None."""
    from .._lib import NORM_NCHW, NORM_NHWC, VALUE_CODES, check, lib
    from ..runtime import operand
    n, px, lay = desc[0], desc[1], desc[2]
    vmap = ctx.empty((n, 4, px), np.uint8)
    if n and px:
        fo = None if form is None else operand(flags, ctx, (np.uint8,), to_device=True)
        check(lib.rfi_valid_map(ctx.handle, C.c_void_p(src.ptr), VALUE_CODES[src.dtype], NORM_NHWC if lay == "nhwc" else NORM_NCHW,
                                n, px, None if fo is None else C.c_void_p(fo.ptr), form or 0, C.c_void_p(vmap.ptr), None, 0))
        if fo is not None and fo.keep is not flags:
            ctx.synchronize()                           # (an uploaded copy of the flags goes with this frame)
    return vmap


def invalid_map(data, flags=None, layout=None, device=None):
    """``DeviceArray`` ``(n, 4, T, F)`` uint8, 1 where a visibility of `data` is invalid: its prior flag is set or its real or
    imaginary part is non-finite (``rfi_valid_map``, what ``transform(flags=)`` and ``tile_observation(flags=)`` decide
    internally).  `data`: any input this module accepts (NumPy or ``DeviceArray``); `flags`: prior flags per
    polarisation or per baseline, None or ``"nonfinite"``: none.  ``inference.tile_labels(invalid=)`` takes the result."""
    from ..runtime import DeviceArray, context_for, operand
    if not isinstance(data, DeviceArray):
        data = np.asarray(data)
    n, px, lay, (T, F) = _describe(data, layout)
    form = None if flags is None else _flags_form(flags, n, (T, F))
    ctx = context_for(device, data, flags)
    src = operand(data, ctx, tuple(_SCALAR), to_device=True)
    vmap = _invalid_map(ctx, src, (n, px, lay), flags if form is not None else None, form)
    if src.keep is not data:
        ctx.synchronize()                               # (an uploaded copy of the data goes with this frame)
    vmap.shape = (n, 4, T, F)                           # (the same bytes: pixels = T F)
    return vmap


def _lerp(a, b, t):
    """NumPy's _lerp for scalars."""
    d = b - a
    return b - d * (1.0 - t) if t >= 0.5 else a + d * t


def bracket(count, q):
    """(lower rank, upper rank, fraction) of quantile q among `count` values (NumPy's default linear method)."""
    from .._lib import check, lib
    r = (C.c_int64 * 2)()
    f = C.c_double()
    check(lib.rfi_norm_bracket(int(count), float(q), r, C.byref(f)))
    return int(r[0]), int(r[1]), float(f.value)


def quantiles_from_brackets(count, q):
    """(median, q25, q75) from the record's brackets q[3][2], as np.median / np.percentile form them."""
    (mlo, mhi), (alo, ahi), (blo, bhi) = q
    median = mlo if count % 2 else (mlo + mhi) / 2.0
    return median, _lerp(alo, ahi, bracket(count, 0.25)[2]), _lerp(blo, bhi, bracket(count, 0.75)[2])


def dataset_parameters(method, st):
    """RFIMaskDataset's attributes and the (centre, scale) pair of `method` from one population's statistics `st`
    (a dict with count, min, max, mean, var, q).  scale 0.0 stands for the all-zeros transform."""
    if st["count"] == 0:                                # (no valid scalar: NaN statistics, the all-zeros transform)
        nan = float("nan")
        return {"global_min": nan, "global_max": nan, "mean": nan, "std": nan, "robust_median": nan if method == "robust_scale" else None,
                "robust_iqr": nan if method == "robust_scale" else None}, (0.0, 0.0)
    attrs = {"global_min": st["min"], "global_max": st["max"], "mean": st["mean"], "std": math.sqrt(st["var"]) + 1e-8,
             "robust_median": None, "robust_iqr": None}
    if method == "robust_scale":
        med, q25, q75 = quantiles_from_brackets(st["count"], st["q"])
        attrs["robust_median"], attrs["robust_iqr"] = med, q75 - q25 + 1e-8
        pair = (med, attrs["robust_iqr"])
    elif method == "global_min_max":
        pair = (st["min"], st["max"] - st["min"]) if st["max"] > st["min"] else (0.0, 0.0)
    elif method == "standardize":
        pair = (attrs["mean"], attrs["std"])
    else:
        pair = (0.0, 1.0)
    return attrs, pair


def sample_parameters(method, st):
    """normalize_array's (centre, scale) for one sample from its statistics (scikit-learn 1.7's constant-feature rules)."""
    n = st["count"]                                     # (with prior flags: the number of valid scalars)
    if n == 0:
        return 0.0, 0.0
    if method == "global_min_max":
        return (st["min"], st["max"] - st["min"]) if st["max"] > st["min"] else (0.0, 0.0)
    if method == "standardize":
        var, mean = st["var"], st["mean"]
        constant = var <= n * _EPS * var + (n * mean * _EPS) ** 2
        return mean, 1.0 if constant else math.sqrt(var)
    if method == "robust_scale":
        med, q25, q75 = quantiles_from_brackets(n, st["q"])
        scale = q75 - q25
        return med, 1.0 if scale < 10 * _EPS else scale
    return 0.0, 1.0


class Normalizer:
    """``Normalizer(method, scope).fit(x).transform(x, out="nhwc")``; see the module docstring.

    method: "global_min_max", "standardize", "robust_scale" or None (a float32 cast).  scope "dataset": one set of
    parameters from everything passed to ``fit`` (an array or a list of arrays, which need not be concatenated);
    the attributes ``global_min``, ``global_max``, ``mean``, ``std``, ``robust_median``, ``robust_iqr`` are the
    reference dataset's.  scope "sample": ``fit`` takes one array and keeps one (centre, scale) pair per sample in
    ``centres`` / ``scales``; ``transform`` then takes an array of as many samples."""

    def __init__(self, method="global_min_max", scope="dataset", device=None):
        if method not in METHODS:
            raise ValueError(f"Unsupported normalization method: {method}")
        if scope not in ("dataset", "sample"):
            raise ValueError(f"scope must be 'dataset' or 'sample', got {scope!r}")
        self.method, self.scope, self.device = method, scope, device
        self.global_min = self.global_max = self.mean = self.std = self.robust_median = self.robust_iqr = None
        self.centres = self.scales = None          # per sample (scope "sample") or one entry (scope "dataset")
        self._params_dev = None

    @staticmethod
    def _as_list(x):
        return list(x) if isinstance(x, (list, tuple)) else [x]

    def statistics(self, x_or_list, layout=None, quantiles=True, flags=None):
        """The raw per-population statistics (list of dicts) of what ``fit`` would see; raises on non-finite input.
        quantiles=False skips the order statistics (``q`` is NaN): 2 reads of the data instead of 6.
        flags: prior flags (one array, or a list like `x_or_list`) or "nonfinite": the statistics of the valid scalars
        (module docstring); non-finite input is then skipped, not refused."""
        from .._lib import F32, F64, VALID_SRC_COMPLEX, VALID_SRC_NHWC, VALID_SRC_PLANAR, NormStats, check, lib
        from ..runtime import DeviceArray, context_for, operand
        xs = [x if isinstance(x, DeviceArray) else np.asarray(x) for x in self._as_list(x_or_list)]
        if not xs:
            raise ValueError("fit needs at least one array")
        if self.scope == "sample" and len(xs) != 1:
            raise ValueError("scope='sample' fits one array at a time")
        desc = [_describe(x, layout) for x in xs]
        scalars = {_SCALAR[np.dtype(x.dtype)] for x in xs}
        if len(scalars) != 1:
            raise ValueError("all chunks must have the same precision (float64 / complex128 or float32 / complex64)")
        if sum(d[0] for d in desc) == 0:
            raise ValueError("fit needs at least one sample")
        scalar = scalars.pop()
        forms = None
        if flags is not None:
            fl = list(flags) if isinstance(flags, (list, tuple)) else [flags] * (len(xs) if isinstance(flags, str) else 1)
            if len(fl) != len(xs):
                raise ValueError(f"flags must match the data: {len(xs)} chunk(s) of data, {len(fl)} of flags")
            forms = [_flags_form(f, d[0], d[3], f"flags[{i}]" if len(fl) > 1 else "flags") for i, (f, d) in enumerate(zip(fl, desc))]
        ctx = context_for(self.device, *xs)
        devs = [operand(x, ctx, tuple(_SCALAR), to_device=True) for x in xs]      # kept alive until the call returns
        counts = [d[0] * d[1] * 8 for d in desc]
        n = len(devs)
        ptrs = (C.c_void_p * n)(*[d.ptr for d in devs])
        cnts = (C.c_int64 * n)(*counts)
        segment = desc[0][1] * 8 if self.scope == "sample" else 0
        pops = desc[0][0] if self.scope == "sample" else 1
        out = (NormStats * pops)()
        if forms is None:
            check(lib.rfi_norm_statistics(ctx.handle, ptrs, cnts, n, F32 if scalar == np.float32 else F64, segment,
                                          1 if quantiles else 0, out, pops))
        else:
            maps = [_invalid_map(ctx, s, d, f, form) for s, d, f, form in zip(devs, desc, fl, forms)]
            mptrs = (C.c_void_p * n)(*[m.ptr for m in maps])
            kinds = (C.c_int * n)(*[VALID_SRC_COMPLEX if np.dtype(x.dtype).kind == "c" else
                                    (VALID_SRC_NHWC if d[2] == "nhwc" else VALID_SRC_PLANAR) for x, d in zip(xs, desc)])
            pixels = (C.c_int64 * n)(*[max(1, d[1]) for d in desc])
            check(lib.rfi_valid_statistics(ctx.handle, ptrs, cnts, mptrs, kinds, pixels, n, F32 if scalar == np.float32 else F64,
                                           segment, 1 if quantiles else 0, out, pops))
            del maps
        del devs
        bad = sum(int(r.nonfinite) for r in out)
        if bad:
            raise ValueError(f"input holds {bad} non-finite value(s); normalisation needs finite data")
        return [{"count": int(r.count), "min": float(r.min), "max": float(r.max), "mean": float(r.mean), "var": float(r.var),
                 "q": tuple((float(r.q[j][0]), float(r.q[j][1])) for j in range(3))} for r in out]

    # ---- the surface
    def fit(self, x_or_list, layout=None, flags=None):
        stats = self.statistics(x_or_list, layout, quantiles=self.method == "robust_scale", flags=flags)
        if self.scope == "dataset":
            attrs, pair = dataset_parameters(self.method, stats[0])
            for k, v in attrs.items():
                setattr(self, k, v)
            pairs = [pair]
        else:
            pairs = [sample_parameters(self.method, st) for st in stats]
        self.centres = [float(p[0]) for p in pairs]
        self.scales = [float(p[1]) for p in pairs]
        self._params_dev = None
        return self

    def transform(self, x, out="nhwc", layout=None, flags=None, fill=0.0):
        """float32 (n, T, F, 8) for out="nhwc", (n, 8, T, F) for out="nchw": DeviceArray for DeviceArray input (stream-
        ordered, nothing synchronised), NumPy for NumPy input.  flags (prior flags or "nonfinite") and fill: both
        channels of an invalid visibility are written as float32 `fill` (module docstring); the call then synchronises,
        since the invalid map it builds is its own."""
        from .._lib import NORM_NCHW, NORM_NHWC, VALUE_CODES, check, lib
        from ..runtime import DeviceArray, context_for, operand
        if out not in ("nhwc", "nchw"):
            raise ValueError(f"out must be 'nhwc' or 'nchw', got {out!r}")
        if not isinstance(x, DeviceArray):
            x = np.asarray(x)
        n, px, lay, (T, F) = _describe(x, layout)
        if self.centres is None:
            raise RuntimeError("transform before fit (or load_state_dict)")
        if self.scope == "sample" and len(self.centres) != n:
            raise ValueError(f"fitted on {len(self.centres)} samples, asked to transform {n}")
        form = None
        if flags is not None:
            form = _flags_form(flags, n, (T, F))
            fill = float(np.float32(fill))
        on_device = isinstance(x, DeviceArray)
        ctx = context_for(self.device, x)
        src = operand(x, ctx, tuple(_SCALAR), to_device=True)
        dst = ctx.empty((n, T, F, 8) if out == "nhwc" else (n, 8, T, F), np.float32)
        params = None
        if self.scope == "sample":
            if self._params_dev is None or self._params_dev.ctx is not ctx:
                self._params_dev = ctx.to_device(np.stack([self.centres, self.scales], axis=1).astype(np.float64))
            params = C.c_void_p(self._params_dev.ptr)
        if flags is None:
            check(lib.rfi_norm_apply(ctx.handle, C.c_void_p(src.ptr), VALUE_CODES[src.dtype], NORM_NHWC if lay == "nhwc" else NORM_NCHW, n, px,
                                     self.centres[0], self.scales[0], params, C.c_void_p(dst.ptr),
                                     NORM_NHWC if out == "nhwc" else NORM_NCHW))
        elif n and px:
            vmap = _invalid_map(ctx, src, (n, px, lay), flags, form)
            check(lib.rfi_valid_apply(ctx.handle, C.c_void_p(src.ptr), VALUE_CODES[src.dtype], NORM_NHWC if lay == "nhwc" else NORM_NCHW,
                                      n, px, self.centres[0], self.scales[0], params, C.c_void_p(vmap.ptr), fill, C.c_void_p(dst.ptr),
                                      NORM_NHWC if out == "nhwc" else NORM_NCHW))
            if on_device:
                ctx.synchronize()                       # (the map is this call's own: it must outlive the kernel that reads it)
        if on_device:
            return dst
        return dst.numpy()                              # (the copy waits for the stream, so `src` may go now)

    def fit_transform(self, x, out="nhwc", layout=None, flags=None, fill=0.0):
        if self.scope == "dataset" and isinstance(x, (list, tuple)):
            raise ValueError("fit_transform takes one array; fit a list, then transform each chunk")
        return self.fit(x, layout, flags).transform(x, out, layout, flags, fill)

    def state_dict(self):
        """Plain Python floats and strings (fit for a checkpoint's ``args``)."""
        return {"method": self.method, "scope": self.scope, "global_min": self.global_min, "global_max": self.global_max,
                "mean": self.mean, "std": self.std, "robust_median": self.robust_median, "robust_iqr": self.robust_iqr,
                "centres": None if self.centres is None else list(self.centres),
                "scales": None if self.scales is None else list(self.scales)}

    def load_state_dict(self, state):
        if state["method"] not in METHODS:
            raise ValueError(f"Unsupported normalization method: {state['method']}")
        if state["scope"] not in ("dataset", "sample"):
            raise ValueError(f"scope must be 'dataset' or 'sample', got {state['scope']!r}")
        self.method, self.scope = state["method"], state["scope"]
        for k in ("global_min", "global_max", "mean", "std", "robust_median", "robust_iqr"):
            v = state.get(k)
            setattr(self, k, None if v is None else float(v))
        self.centres = None if state.get("centres") is None else [float(v) for v in state["centres"]]
        self.scales = None if state.get("scales") is None else [float(v) for v in state["scales"]]
        self._params_dev = None
        return self


def normalize_array(data, method="standardize", device=None, flags=None, fill=0.0):
    """``scripts/normalize_rfi_data.py::normalize_array`` for one (8, T, F) array, computed on the GPU.  Returns
    float32: what the reference's training loop sees after ``torch.tensor(..., dtype=torch.float32)``.
    flags: prior flags (4, T, F) or (T, F), or "nonfinite"; invalid visibilities are left out of the statistics and
    come back as `fill` (module docstring)."""
    if method not in METHODS:
        raise ValueError(f"Unsupported normalization method: {method}")
    data = np.asarray(data)
    if data.ndim != 3 or data.shape[0] != 8:
        raise ValueError(f"data must be (8, T, F), got shape {data.shape}")
    if flags is not None and not isinstance(flags, str):
        flags = np.asarray(flags)
        if flags.shape not in ((4,) + data.shape[1:], data.shape[1:]):
            raise ValueError(f"flags must be {(4,) + data.shape[1:]} or {data.shape[1:]}, got shape {flags.shape}")
        flags = flags[None]
    return Normalizer(method, scope="sample", device=device).fit_transform(data[None], out="nchw", layout="nchw", flags=flags,
                                                                           fill=fill)[0]
