"""The cases of test_gpu_preprocess_kernels.py, as plain data and NumPy, importable without a GPU:
test_preprocess_cases_host.py proves on the CPU that the table covers what it claims and that the criteria can fail.

Three tables:

* CASES -- the channel kernels prep_pass1 / prep_pass2: shape x dtype x a group of three patches, one content kind per
  patch.  The shapes are read off launch_preprocess's pixels-per-block formula (``npb`` below, restated from
  csrc/preprocess.hip): a block owns ``npb`` consecutive pixels of a patch and reads the row above them as its halo, so
  what can go wrong sits on the seams between blocks.
* planted_patch -- 64 x 64 patches with four pixels planted on and one ulp beyond the MAD thresholds, for the order
  statistics behind rfi_mad_flags / rfi_preprocess_real.
* median_stack -- 8-patch stacks for the radix-selection median on its own (rfi_op_patch_median).
"""
import warnings
import zlib
from collections import namedtuple

import numpy as np

from oracle import preprocess_ref

# ---------------------------------------------------------------------------------------------- the block layout

def npb(pw, esz):
    """Pixels per workgroup of prep_pass1 for rows of ``pw`` pixels, esz = 8 (64-bit input) or 4 (32-bit input):
    at least four rows, capped by the 64 KiB of LDS that hold the halo row and the block's own pixels."""
    return min(max(2048, 4 * pw), 64 * 1024 // esz - pw)


def esz_of(dtype):
    return 8 if np.dtype(dtype) in (np.dtype(np.complex128), np.dtype(np.float64)) else 4


def seam_classes(ph, pw, esz):
    """What kind of block seams a shape has: the set the host test wants covered."""
    n, per = npb(pw, esz), ph * pw
    blocks = -(-per // n)
    out = set()
    if blocks == 1:
        out.add("single-block")
    else:
        out.add("row-aligned" if n % pw == 0 else "mid-row")
        if per % n:
            out.add("ragged-last")
        if n > 2 * pw and n % pw:
            out.add("block-over-two-rows")
    if pw > 2048:
        out.add("wide-row")
    if n < max(2048, 4 * pw):
        out.add("cap-active")
    if per < 64:
        out.add("under-one-wave")
    return out


SHAPES = [(128, 128), (256, 256),            # the default sizes: 8 / 32 blocks, seams on row boundaries
          (80, 96), (257, 33),               # 2048 % pw != 0: blocks start mid-row, ragged last block
          (3, 2500),                         # pw > 2048; 64-bit: npb capped at 5692, a seam mid-row; 32-bit: one block
          (4096, 1), (1, 4096),              # every d1 = 0; every d0 = 0 and the longest 64-bit row accepted
          (1, 1), (2, 2)]                    # flat by construction; fewer pixels than one wave
DTYPES = [np.complex128, np.complex64, np.float64, np.float32]
DTYPE_TAG = {np.complex128: "c128", np.complex64: "c64", np.float64: "f64", np.float32: "f32"}

# one content kind per patch; the groups differ between complex and real input
GROUPS_COMPLEX = {"A": ("wide", "zeros", "const"),
                  "B": ("phase-pi", "nonfinite-interior", "nonfinite-seam"),
                  "C": ("all-nan", "zero0j", "wide")}
GROUPS_REAL = {"A": ("wide", "zeros", "const"),
               "B": ("lowc-1e-2", "nonfinite-interior", "nonfinite-seam"),
               "C": ("all-nan", "lowc-1e-4", "wide")}

Case = namedtuple("Case", "id shape dtype group kinds")
CASES = []
for _shape in SHAPES:
    for _dt in DTYPES:
        _groups = GROUPS_COMPLEX if np.dtype(_dt).kind == "c" else GROUPS_REAL
        for _g, _kinds in _groups.items():
            CASES.append(Case(f"{_shape[0]}x{_shape[1]}-{DTYPE_TAG[_dt]}-{_g}", _shape, _dt, _g, _kinds))


def nonfinite_positions(kind, ph, pw, esz):
    """(flat index of the NaN pixel or None, of the +-inf pixel or None) for the two non-finite kinds.
    interior: both well inside the first block.  seam: the NaN in the halo row of the second block (the last row the first
    block owns), the infinity on the first row of the last block; with one block, on the patch's first row."""
    n, per = npb(pw, esz), ph * pw
    blocks = -(-per // n)
    if per == 1:
        return (0, None) if kind == "nonfinite-interior" else (None, 0)
    if kind == "nonfinite-interior":
        own = min(n, per)
        a = own // 2 + pw // 2
        b = a + 2 * pw + 3
        if not (pw < a and b + pw < own):
            a, b = per // 3, (2 * per) // 3
        return a, b
    if blocks == 1:
        return min(1, per - 1), min(3, per - 1) if per > 2 else 0
    nan_at = n - pw + min(1, pw - 1)
    inf_at = (blocks - 1) * n + (min(2, pw - 1) if pw > 1 else 1)
    return nan_at, min(inf_at, per - 1)


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


def make_patch(kind, shape, dtype, seed):
    """One (ph, pw) patch of ``dtype`` with the named content."""
    ph, pw = shape
    dt = np.dtype(dtype)
    cplx = dt.kind == "c"
    real = np.float32 if dt.itemsize == (8 if cplx else 4) else np.float64
    rng = np.random.default_rng(seed)
    amp = 10.0 ** rng.uniform(-12, 6, size=shape)          # channel 1 of complex input clips at both ends
    if kind == "zeros":                                     # exact zeros: la = -10
        amp[rng.random(shape) < 0.3] = 0.0
    if kind == "const":
        amp[...] = 10.0 ** rng.uniform(-2, 3)
    if kind.startswith("lowc"):                             # low contrast around a non-zero mean log-amplitude (3)
        amp = 1000.0 * (1.0 + float(kind[5:]) * rng.normal(size=shape))
    if cplx:
        ang = rng.uniform(-np.pi, np.pi, size=shape)
        if kind == "const":
            ang[...] = 0.7
        z = (amp * np.exp(1j * ang)).astype(dt)
        if kind == "phase-pi":                              # re < 0 with im = +0.0 (phase pi, channel 2 = 1) and -0.0 (-pi, 0)
            which = rng.integers(0, 3, size=shape)
            neg = (-amp).astype(real)
            z.real[which > 0] = neg[which > 0]
            z.imag[which == 1] = 0.0
            z.imag[which == 2] = -0.0
        if kind == "zero0j":
            z[rng.random(shape) < 0.5] = 0
            z.flat[0] = 0
        x = z
    else:
        x = (amp * rng.choice([-1.0, 1.0], size=shape)).astype(dt) if not kind.startswith("lowc") else amp.astype(dt)
    if kind == "all-nan":
        x[...] = np.nan
    if kind.startswith("nonfinite"):
        a, b = nonfinite_positions(kind, ph, pw, esz_of(dt))
        sign = -1.0 if seed & 1 else 1.0
        if b is not None:
            x.flat[b] = sign * np.inf
        if a is not None:
            x.flat[a] = complex(np.nan, 1.0) if cplx else np.nan
    return x


def make_patches(case):
    return np.stack([make_patch(k, case.shape, case.dtype, _seed(case.id, i, k)) for i, k in enumerate(case.kinds)])


# ---------------------------------------------------------------------------------------------- the image criterion
ATOL_64 = 2e-6            # the project's bound for this kernel on 64-bit input (test_gpu_preprocess_metrics.py)


def reference_images(patches):
    """-> (float64-oracle images, float32-oracle images or None for 64-bit input), as create_dataset stores them."""
    p = np.asarray(patches)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)              # all-NaN patches, inf - inf
        want64 = preprocess_ref.images_of(preprocess_ref.channels(p))
        want32 = preprocess_ref.images_of(preprocess_ref.channels_f32(p)) if esz_of(p.dtype) == 4 else None
    return want64, want32


def _maxerr(a, b):
    """max |a - b| per channel over the positions where b is a number"""
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    d = np.where(np.isnan(b), 0.0, d).reshape(-1, 3)
    return d.max(axis=0) if len(d) else np.zeros(3)


def image_errors(got, want64, want32=None):
    """-> (NaN positions agree, device error per channel, bound per channel, err_ref per channel).
    64-bit input: the bound is ATOL_64.  32-bit input: err_ref = max |float32 oracle - float64 oracle| of this very stack
    and channel is what float32 arithmetic costs NumPy itself; the device may cost max(4 err_ref, ATOL_64) -- the factor 4
    allows log10f / atan2f / hypotf a few ulps where NumPy's are about one."""
    nan_ok = np.array_equal(np.isnan(got), np.isnan(want64))
    err = _maxerr(got, want64)
    if want32 is None:
        return nan_ok, err, np.full(3, ATOL_64), np.zeros(3)
    err_ref = _maxerr(want32, want64)
    return nan_ok, err, np.maximum(4.0 * err_ref, ATOL_64), err_ref


def check_images(got, patches, what=""):
    """Assert the criterion patch by patch, so that a failure names the patch (and with it the content kind)."""
    worst_err, worst_ref = np.zeros(3), np.zeros(3)
    for i in range(len(patches)):
        want64, want32 = reference_images(patches[i:i + 1])
        nan_ok, err, bound, err_ref = image_errors(got[i:i + 1], want64, want32)
        assert nan_ok, f"{what} patch {i}: NaN positions differ from the oracle's"
        assert (err <= bound).all(), f"{what} patch {i}: error per channel {err} over the bound {bound}"
        worst_err, worst_ref = np.maximum(worst_err, err), np.maximum(worst_ref, err_ref)
    return worst_err, worst_ref


def emulate_f32_stored_logamp(x):
    """Images of REAL float64 patches the way the channel kernels formed them before the log-amplitude slot was made
    relative to the first pixel: float64 extrema, but the log-amplitude itself rounded to float32 before the min-max.
    A known-wrong form: the criterion has to reject it on the low-contrast patches."""
    ch = preprocess_ref.channels_real(np.asarray(x, np.float64))
    la = np.log10(np.abs(x) + 1e-10)
    lo, hi = (f(la, axis=(1, 2), keepdims=True) for f in (np.nanmin, np.nanmax))
    stored = la.astype(np.float32).astype(np.float64)
    ch[..., 1] = np.where(hi > lo, (stored - lo) / np.where(hi > lo, hi - lo, 1.0), 0.0)
    return preprocess_ref.images_of(ch)


# ---------------------------------------------------------------------------------------------- planted thresholds
PLANT_SEEDS = tuple(range(8))
PLANT_SHAPE = (64, 64)
MEDIAN_AT = 8.0            # the raw patch's median, exactly: dividing by it is exact in both arithmetics

Planted = namedtuple("Planted", "patch processed index targets med mad hi lo flags")


def real_dtype(dtype):
    dt = np.dtype(dtype)
    return np.dtype(np.float32) if dt in (np.dtype(np.complex64), np.dtype(np.float32)) else np.dtype(np.float64)


def processed_of(x, stretch, normalize):
    """What the MAD flags are taken of: the oracle's real-input pipeline in the array's own arithmetic (|z| for complex)."""
    x = np.asarray(x)
    p = np.abs(x) if np.iscomplexobj(x) else x
    p = p[None]
    if normalize:
        dt = p.dtype
        p = preprocess_ref.median_normalise(p)
        assert p.dtype == dt
    if stretch:
        p = preprocess_ref.stretch(p, stretch)
    return p[0]


def thresholds(p, sigma):
    """(med, mad, hi, lo) of one processed patch as preprocess_ref.mad_flags forms them, in the array's arithmetic."""
    med = np.nanmedian(p)
    mad = preprocess_ref._mad(p.ravel())
    return med, mad, med + mad * sigma, med - mad * sigma


def _as_input(amp, dtype, rng):
    """Amplitudes -> the input dtype with |x| == amp exactly: complex values get one zero component."""
    dt = np.dtype(dtype)
    if dt.kind != "c":
        return amp.astype(dt)
    z = np.zeros(amp.shape, dt)
    on_re = rng.random(amp.shape) < 0.5
    sign = rng.choice([-1.0, 1.0], size=amp.shape).astype(amp.dtype)
    z.real[on_re] = (sign * amp)[on_re]
    z.imag[~on_re] = (sign * amp)[~on_re]
    return z


def base_patch(seed, dtype, quantum=None):
    """64 x 64 amplitudes around 8 whose median is exactly 8 (the two middle values are set to it); with ``quantum`` the
    values are multiples of it, so many pixels tie at the median."""
    rt = real_dtype(dtype)
    rng = np.random.default_rng(1000 + seed)
    a = np.abs(8.0 + 0.8 * rng.normal(size=PLANT_SHAPE)).astype(rt)
    if quantum:
        return (np.round(a / quantum) * quantum).astype(rt), rng
    a = (a * (rt.type(MEDIAN_AT) / np.median(a))).astype(rt)          # the middle values are now within rounding of 8
    order = np.argsort(a.ravel(), kind="stable")
    mid = a.size // 2
    a.flat[order[mid - 1]] = a.flat[order[mid]] = MEDIAN_AT
    assert np.median(a) == MEDIAN_AT and a.flat[order[mid - 2]] <= MEDIAN_AT <= a.flat[order[mid + 1]]
    return a, rng


def planted_patch(seed, dtype, stretch=None, normalize=False, sigma=5):
    """A patch whose processed form has four pixels exactly at hi, nextafter(hi, +inf), lo, nextafter(lo, -inf) of its own
    MAD thresholds, computed by NumPy in the dtype's arithmetic, planted where they leave median and MAD untouched:
    each replaces a pixel that already lay further than the MAD from the median on the same side."""
    assert stretch in (None, "SQRT")
    rt = real_dtype(dtype)
    amp, rng = base_patch(seed, dtype)
    p = processed_of(amp, stretch, normalize)
    med, mad, hi, lo = thresholds(p, sigma)
    assert p.dtype == rt and np.asarray(hi).dtype == rt and lo > 0 and mad > 0
    above, below = np.flatnonzero(p.ravel() > med + mad), np.flatnonzero(p.ravel() < med - mad)
    index = np.concatenate([rng.choice(above, 2, replace=False), rng.choice(below, 2, replace=False)])
    targets = np.array([hi, np.nextafter(hi, rt.type(np.inf)), lo, np.nextafter(lo, rt.type(-np.inf))], dtype=rt)
    scale = rt.type(MEDIAN_AT if normalize else 1.0)
    raw = (targets * targets if stretch == "SQRT" else targets) * scale        # sqrt(fl(t * t)) == t; * 8 is exact
    amp.flat[index] = raw.astype(rt)
    got = processed_of(amp, stretch, normalize)
    flags = preprocess_ref.mad_flags(got[None], sigma)[0]
    return Planted(_as_input(amp, dtype, rng), got, index, targets, med, mad, hi, lo, flags)


def tied_patch(seed, dtype):
    """For sigma = 0 (hi == lo == med, so the flags are "p != med"): multiples of 1/8, many of them equal to the median."""
    amp, rng = base_patch(seed, dtype, quantum=0.125)
    flags = preprocess_ref.mad_flags(amp[None], 0)[0]
    return _as_input(amp, dtype, rng), flags


# ---------------------------------------------------------------------------------------------- the median on its own
MEDIAN_PERS = (1, 2, 3, 255, 256, 257, 1000, 4096)
MEDIAN_KINDS = ("normal", "all-equal", "half-tied", "negative", "mixed-signs", "low-byte", "top-bytes", "subnormal",
                "infinities", "nans", "finite-only")


def median_stack(kind, per, f32, seed=0):
    """(8, per) float64 values (float32-representable when ``f32``) and finite_only for the kind."""
    rt = np.float32 if f32 else np.float64
    rng = np.random.default_rng(_seed("median", kind, per, f32, seed))
    v = rng.normal(size=(8, per)).astype(rt)
    if kind == "all-equal":
        v[...] = rng.normal(size=(8, 1)).astype(rt)
    elif kind == "half-tied":                  # half the values equal the median: ranks inside one radix bin to the end
        s = np.sort(v, axis=1)
        m = s[:, per // 2]
        lo, hi = per // 4, per // 4 + (per + 1) // 2
        s[:, lo:hi] = m[:, None]
        v = rng.permuted(s, axis=1)
    elif kind == "negative":
        v = -np.abs(v) - rt(1e-3)
    elif kind == "mixed-signs":                # small values around 0 with both zeros present
        v = (v * rt(1e-3)).astype(rt)
        v[:, ::3] = rt(-0.0)
        v[:, 1::5] = rt(0.0)
    elif kind == "low-byte":                   # equal but for the lowest byte of the key: the last radix pass decides
        base = rng.normal(size=(8, 1)).astype(rt)
        bits = base.view(np.uint32 if f32 else np.uint64) & ~(np.uint32(0xFF) if f32 else np.uint64(0xFF))
        low = rng.integers(0, 256, size=(8, per)).astype(bits.dtype)
        v = (bits | low).view(rt)
    elif kind == "top-bytes":                  # magnitudes across the exponent range: the first pass decides
        e = rng.uniform(-30, 30, size=(8, per))
        v = (rng.choice([-1.0, 1.0], size=(8, per)) * 10.0 ** e).astype(rt)
    elif kind == "subnormal":
        tiny = np.finfo(rt).smallest_subnormal
        v = (rng.integers(-1000, 1000, size=(8, per)) * tiny).astype(rt)
    elif kind in ("infinities", "finite-only"):
        k = rng.integers(0, per + 1, size=8)
        for i in range(8):
            at = rng.permutation(per)[:k[i]]
            v[i, at] = rng.choice([-np.inf, np.inf], size=k[i])
        if per >= 2:                            # an even count whose middle is (-inf, +inf): the median is NaN
            v[0, :per // 2] = -np.inf
            v[0, per // 2:] = np.inf
            v[1, :] = np.inf
    elif kind == "nans":                        # 1, per - 1 and per NaNs, and counts between
        for i, k in enumerate((1, per - 1, per, per // 2, 1, per - 1, per, per // 3)):
            v[i, rng.permutation(per)[:max(k, 0)]] = np.nan
    return v.astype(np.float64), kind == "finite-only", v


def median_expected(v_native, finite_only, centre=None):
    """-> (median per patch widened to float64, participant count) by NumPy in v_native's own arithmetic;
    ``centre`` (per patch, v_native's dtype): of |v - centre| instead."""
    med, cnt = np.empty(len(v_native), np.float64), np.empty(len(v_native), np.int32)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        for i, row in enumerate(v_native):
            keep = row[np.isfinite(row) if finite_only else ~np.isnan(row)]
            if centre is not None:
                keep = np.abs(keep - centre[i])
            cnt[i] = keep.size
            med[i] = np.median(keep) if keep.size else np.nan
    return med, cnt
