"""The inputs of the validity-aware tests (test_valid_path_host.py, test_gpu_valid_path.py): observations with about
10 % random prior flags and planted non-finite values, in every source form, and the planted populations at which the
statistics kernel can go wrong.  NumPy only."""
import numpy as np

import normalize_ref as nref

SHAPE = (40, 52)            # 4 * 40 * 52 * 2 = 16640 scalars a sample: two 8192-scalar sum tiles and a ragged third
SHAPE2 = (77, 50)
KINDS = ("c128", "c64", "f64_nchw", "f32_nhwc")
SUM_TILE = 8192


def observation(shape=SHAPE, dtype=np.complex128, seed=0, n=3):
    """(n, 4, C, T): noise with a few bright channels and a burst, every baseline on its own scale and offset."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 4) + tuple(shape)) + 1j * rng.standard_normal((n, 4) + tuple(shape))
    C_, T_ = shape
    d[..., C_ // 3: C_ // 3 + 3, :] *= 40.0
    d[..., :, T_ // 2: T_ // 2 + 2] *= 25.0
    d *= np.resize([1.0, 7.5, 0.02], n).reshape(n, 1, 1, 1)
    d += np.resize([0.5, 3.0 - 2.0j, 0.01j], n).reshape(n, 1, 1, 1)
    return d.astype(dtype)


def plant_nonfinite(data, seed=1, each=5):
    """A copy with, in every sample: NaN in real parts only, +inf in imaginary parts only, -inf in real parts."""
    rng = np.random.default_rng(seed)
    d = data.copy()
    per = d[0].size
    for i in range(len(d)):
        at = rng.choice(per, 3 * each, replace=False)
        flat = d[i].reshape(-1)
        flat[at[:each]] = np.nan + 1j * flat[at[:each]].imag
        flat[at[each:2 * each]] = flat[at[each:2 * each]].real + 1j * np.inf
        flat[at[2 * each:]] = -np.inf + 1j * flat[at[2 * each:]].imag
    return d


def prior_flags(data_shape, seed=2, per_baseline=False, share=0.1):
    shape = (data_shape[0],) + tuple(data_shape[2:]) if per_baseline else tuple(data_shape)
    return (np.random.default_rng(seed).random(shape) < share).astype(np.uint8)


def as_kind(z, kind):
    """complex (n, 4, T, F) -> (array in the source form `kind`, its layout argument)"""
    if kind == "c128":
        return z.astype(np.complex128), None
    if kind == "c64":
        return z.astype(np.complex64), None
    planar = nref.to_nchw(z).astype(np.float32 if kind.startswith("f32") else np.float64)
    if kind.endswith("nhwc"):
        return np.ascontiguousarray(planar.transpose(0, 2, 3, 1)), "nhwc"
    return planar, "nchw"


def working(kind="c128", per_baseline=False, shape=SHAPE, seed=0):
    """-> (x in `kind`, layout, prior flags): the case mix of the GPU tests"""
    z = plant_nonfinite(observation(shape, np.complex128, seed), seed + 1)
    x, layout = as_kind(z, kind)
    return x, layout, prior_flags(z.shape, seed + 2, per_baseline)


PLANTED = ("none_valid", "one", "two", "three", "even", "odd", "tile_invalid", "extremes_flagged", "all_equal")


def planted(dtype=np.complex128, seed=7):
    """-> (data (9, 4, 40, 52), per-polarisation flags): one population per name in PLANTED, by valid VISIBILITIES (a
    visibility is two scalars, so the valid scalar count is always even): none, 1, 2, 3, 1000 and 1001 (scalar counts
    whose quartile ranks fall on and between elements), one whole 8192-scalar sum tile invalid, the visibilities holding
    the minimum and the maximum scalar flagged, and every valid scalar equal."""
    n = len(PLANTED)
    d = observation(SHAPE, np.complex128, seed, n).astype(dtype)
    f = np.zeros(d.shape, dtype=np.uint8)
    rng = np.random.default_rng(seed + 1)
    per = d[0].size
    for i, keep in ((0, 0), (1, 1), (2, 2), (3, 3), (4, 1000), (5, 1001)):
        fi = np.ones(per, dtype=np.uint8)
        fi[rng.choice(per, keep, replace=False)] = 0
        f[i] = fi.reshape(d[0].shape)
    d[0].reshape(-1)[::7] = np.nan                                   # (what is invalid may hold anything)
    f[6].reshape(-1)[SUM_TILE // 2: SUM_TILE] = 1                    # scalars 8192 .. 16383: the second sum tile
    s = nref.to_nchw(d[7:8])[0]                                      # (8, T, F)
    for idx in (np.unravel_index(np.argmin(s), s.shape), np.unravel_index(np.argmax(s), s.shape)):
        f[7, idx[0] // 2, idx[1], idx[2]] = 1
    f[8] = rng.random(d[8].shape) < 0.5
    d[8][f[8] == 0] = 2.0 + 2.0j
    return d, f
