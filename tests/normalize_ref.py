"""NumPy restatement of the two normalisation scopes (no scikit-learn), the expectation of the normalisation tests.

dataset scope = the reference's RFIMaskDataset (_calculate_normalization_params / _normalize_input); sample scope =
scripts/normalize_rfi_data.py::normalize_array with scikit-learn 1.7's StandardScaler / RobustScaler rules written out.
The moments are exact sums (``math.fsum``) rounded once; the order statistics are NumPy's.  Everything is fp64 on the
values widened to fp64 -- for float32 / complex64 input too, which is NOT NumPy's own float32 arithmetic -- and the
result is rounded once to float32.
"""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
METHODS = ("global_min_max", "standardize", "robust_scale")


def to_nchw(x, layout=None):
    """(n, 8, T, F) fp64 view of any accepted input: planar, channel-last or complex (n, 4, T, F)."""
    x = np.asarray(x)
    if x.dtype.kind == "c":
        n, p, T, F = x.shape
        out = np.empty((n, 8, T, F), dtype=np.float64)
        out[:, 0::2] = x.real
        out[:, 1::2] = x.imag
        return out
    if layout == "nhwc" or (layout is None and x.shape[1] != 8):
        x = x.transpose(0, 3, 1, 2)
    return x.astype(np.float64)


def moments(v):
    """(mean, population variance) of flat fp64 values from exact sums."""
    v = np.asarray(v, dtype=np.float64).ravel()
    mean = math.fsum(v) / v.size
    d = v - mean
    return mean, math.fsum(d * d) / v.size


def dataset_params(chunks, method):
    """-> (attrs dict as RFIMaskDataset, (centre, scale) or None for all zeros); chunks: list of arrays of any layout."""
    v = np.concatenate([np.asarray(to_nchw(c)).ravel() for c in chunks])
    mean, var = moments(v)
    attrs = {"global_min": float(v.min()), "global_max": float(v.max()), "mean": mean, "std": math.sqrt(var) + 1e-8,
             "robust_median": None, "robust_iqr": None}
    if method == "robust_scale":
        attrs["robust_median"] = float(np.median(v))
        attrs["robust_iqr"] = float(np.percentile(v, 75) - np.percentile(v, 25) + 1e-8)
        return attrs, (attrs["robust_median"], attrs["robust_iqr"])
    if method == "global_min_max":
        if attrs["global_max"] > attrs["global_min"]:
            return attrs, (attrs["global_min"], attrs["global_max"] - attrs["global_min"])
        return attrs, None
    if method == "standardize":
        return attrs, (mean, attrs["std"])
    return attrs, (0.0, 1.0)


def sample_params(x, method):
    """(centre, scale) or None (all zeros) of one sample, as normalize_array treats it."""
    v = np.asarray(x, dtype=np.float64).ravel()
    n = v.size
    if method == "global_min_max":
        lo, hi = float(v.min()), float(v.max())
        return (lo, hi - lo) if hi > lo else None
    if method == "standardize":
        mean, var = moments(v)
        constant = var <= n * EPS * var + (n * mean * EPS) ** 2
        return mean, (1.0 if constant else math.sqrt(var))
    if method == "robust_scale":
        scale = float(np.percentile(v, 75) - np.percentile(v, 25))
        return float(np.median(v)), (1.0 if scale < 10 * EPS else scale)
    return 0.0, 1.0


def apply(x_nchw, pair):
    x = np.asarray(x_nchw, dtype=np.float64)
    if pair is None:
        return np.zeros(x.shape, dtype=np.float32)
    return ((x - pair[0]) / pair[1]).astype(np.float32)


def normalize_dataset(chunks, method):
    """-> (attrs, list of float32 (n, 8, T, F) outputs, one per chunk)"""
    attrs, pair = dataset_params(chunks, method)
    return attrs, [apply(to_nchw(c), pair) for c in chunks]


def normalize_samples(x, method, layout=None):
    """float32 (n, 8, T, F): every sample by its own statistics."""
    x = to_nchw(x, layout)
    return np.stack([apply(s, sample_params(s, method)) for s in x])


def ulp_diff_f32(a, b):
    """element-wise distance in float32 units in the last place (both finite float32 arrays of one shape)"""
    def key(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


# ---- the tolerances of the normalisation tests (the same for restatement vs golden and device vs golden)
REL_MOMENT = 1e-12          # mean, std: NumPy's pairwise sums sat 3e-16 / 1e-16 away from the exact sums
MAX_SHARE = 1e-3            # standardize outputs: share of elements that may differ at all (each by <= 1 float32 ulp)


def check_outputs(got, want, method, label=""):
    """min-max and robust outputs: bit-equal float32.  standardize: every element within 1 float32 ulp, at most a
    share of 1e-3 differing at all; prints the count of differing elements."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (label, got.dtype, got.shape, want.shape)
    if method != "standardize":
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (label, method, int((got != want).sum()))
        return 0
    d = ulp_diff_f32(got, want)
    differing = int((d != 0).sum())
    print(f"{label} standardize: {differing} of {d.size} float32 elements differ (max {int(d.max())} ulp)")
    assert int(d.max()) <= 1, (label, int(d.max()))
    assert differing <= MAX_SHARE * d.size, (label, differing, d.size)
    return differing


def check_attrs(got, want, method, label=""):
    """global_min, global_max, robust_median, robust_iqr bit-equal; mean, std within 1e-12 relative"""
    for k in ("global_min", "global_max"):
        assert got[k] == want[k], (label, k, got[k], want[k])
    for k in ("mean", "std"):
        assert abs(got[k] - want[k]) <= REL_MOMENT * abs(want[k]), (label, k, got[k], want[k])
    for k in ("robust_median", "robust_iqr"):
        if method == "robust_scale":
            assert got[k] == want[k], (label, k, got[k], want[k])
        else:
            assert got[k] is None and want[k] is None, (label, k)


def golden_attrs(expected, prefix, method):
    """the reference dataset's attributes as recorded by tests/golden/make_normalization_golden.py"""
    out = {k: float(expected[f"{prefix}{method}.{k}"]) for k in ("global_min", "global_max", "mean", "std")}
    has = bool(expected[f"{prefix}{method}.has_robust"])
    for k in ("robust_median", "robust_iqr"):
        out[k] = float(expected[f"{prefix}{method}.{k}"]) if has else None
    return out
