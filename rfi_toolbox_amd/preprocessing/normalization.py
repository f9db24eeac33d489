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

Deviation: input holding a NaN or an infinity raises ``ValueError`` in ``fit`` (scikit-learn skips NaN; the
reference's data never has one).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

__all__ = ["Normalizer", "normalize_array", "METHODS"]

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
    n = st["count"]
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

    def statistics(self, x_or_list, layout=None, quantiles=True):
        """The raw per-population statistics (list of dicts) of what ``fit`` would see; raises on non-finite input.
        quantiles=False skips the order statistics (``q`` is NaN): 2 reads of the data instead of 6."""
        from .._lib import F32, F64, NormStats, check, lib
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
        ctx = context_for(self.device, *xs)
        devs = [operand(x, ctx, tuple(_SCALAR), to_device=True) for x in xs]      # kept alive until the call returns
        counts = [d[0] * d[1] * 8 for d in desc]
        n = len(devs)
        ptrs = (C.c_void_p * n)(*[d.ptr for d in devs])
        cnts = (C.c_int64 * n)(*counts)
        segment = desc[0][1] * 8 if self.scope == "sample" else 0
        pops = desc[0][0] if self.scope == "sample" else 1
        out = (NormStats * pops)()
        check(lib.rfi_norm_statistics(ctx.handle, ptrs, cnts, n, F32 if scalar == np.float32 else F64, segment,
                                      1 if quantiles else 0, out, pops))
        del devs
        bad = sum(int(r.nonfinite) for r in out)
        if bad:
            raise ValueError(f"input holds {bad} non-finite value(s); normalisation needs finite data")
        return [{"count": int(r.count), "min": float(r.min), "max": float(r.max), "mean": float(r.mean), "var": float(r.var),
                 "q": tuple((float(r.q[j][0]), float(r.q[j][1])) for j in range(3))} for r in out]

    # ---- the surface
    def fit(self, x_or_list, layout=None):
        stats = self.statistics(x_or_list, layout, quantiles=self.method == "robust_scale")
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

    def transform(self, x, out="nhwc", layout=None):
        """float32 (n, T, F, 8) for out="nhwc", (n, 8, T, F) for out="nchw": DeviceArray for DeviceArray input (stream-
        ordered, nothing synchronised), NumPy for NumPy input."""
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
        on_device = isinstance(x, DeviceArray)
        ctx = context_for(self.device, x)
        src = operand(x, ctx, tuple(_SCALAR), to_device=True)
        dst = ctx.empty((n, T, F, 8) if out == "nhwc" else (n, 8, T, F), np.float32)
        params = None
        if self.scope == "sample":
            if self._params_dev is None or self._params_dev.ctx is not ctx:
                self._params_dev = ctx.to_device(np.stack([self.centres, self.scales], axis=1).astype(np.float64))
            params = C.c_void_p(self._params_dev.ptr)
        check(lib.rfi_norm_apply(ctx.handle, C.c_void_p(src.ptr), VALUE_CODES[src.dtype], NORM_NHWC if lay == "nhwc" else NORM_NCHW, n, px,
                                 self.centres[0], self.scales[0], params, C.c_void_p(dst.ptr),
                                 NORM_NHWC if out == "nhwc" else NORM_NCHW))
        if on_device:
            return dst
        return dst.numpy()                              # (the copy waits for the stream, so `src` may go now)

    def fit_transform(self, x, out="nhwc", layout=None):
        if self.scope == "dataset" and isinstance(x, (list, tuple)):
            raise ValueError("fit_transform takes one array; fit a list, then transform each chunk")
        return self.fit(x, layout).transform(x, out, layout)

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


def normalize_array(data, method="standardize", device=None):
    """``scripts/normalize_rfi_data.py::normalize_array`` for one (8, T, F) array, computed on the GPU.  Returns
    float32: what the reference's training loop sees after ``torch.tensor(..., dtype=torch.float32)``."""
    if method not in METHODS:
        raise ValueError(f"Unsupported normalization method: {method}")
    data = np.asarray(data)
    if data.ndim != 3 or data.shape[0] != 8:
        raise ValueError(f"data must be (8, T, F), got shape {data.shape}")
    return Normalizer(method, scope="sample", device=device).fit_transform(data[None], out="nchw", layout="nchw")[0]
