"""-m gpu: the kernels under Preprocessor.create_dataset against the NumPy oracle at their edges -- the channel kernels
over the case table of preprocess_cases.py (test_preprocess_cases_host.py proves the table on the CPU), the gather form
against the oracle's own tiling, the radix-selection median on its own, the MAD thresholds with planted pixels, degenerate
patches, stacks of more patches than one launch's gridDim.y holds, and the confusion reduction.

Bounds on the ImageNet-normalised images, error against the float64 oracle:
    64-bit input   2e-6 flat
    32-bit input   max(4 err_ref, 2e-6) per channel, err_ref = max |float32 oracle - float64 oracle| on the same patches
(the figures measured on an MI355X are in the docstring of test_channel_kernels_against_the_oracle)."""
import warnings

import numpy as np
import pytest

import preprocess_cases as pc
from oracle import metrics_ref, preprocess_ref

pytestmark = pytest.mark.gpu


def _pre():
    from rfi_toolbox_amd.preprocessing import Preprocessor
    return Preprocessor(np.zeros((1, 1, 8, 8), np.complex128))


# ------------------------------------------------------------------ channel kernels over the case table
@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.id)
def test_channel_kernels_against_the_oracle(case):
    """rfi_preprocess_patches on every shape x dtype x content group.  NaN positions must equal the oracle's; the rest is
    held to 2e-6 (64-bit input) or max(4 err_ref, 2e-6) (32-bit input).

    Largest figures over the table on an MI355X, per channel (gradient, log-amplitude, phase):
        complex128                                    device error 4.8e-07 0       0
        float64                                       device error 4.8e-07 7.2e-07 0
        complex64   err_ref 9.5e-07 7.2e-07 7.2e-07   device error 1.2e-06 7.2e-07 7.2e-07
        float32     err_ref 5.6e-03 3.2e-03 0         device error 8.3e-07 7.2e-07 0
    and over the gather cases below: err_ref 1.1e-06 7.2e-07 7.2e-07, device error 1.1e-06 7.2e-07 7.2e-07.
    The large float32 err_ref is the low-contrast patches, where float32 arithmetic itself loses the min-max; for real
    input the device forms the log-amplitude in double and holds it relative to the patch's first pixel, so it stays at
    float32 rounding of the result there too.  Complex64 input is float32 arithmetic throughout."""
    x = pc.make_patches(case)
    got = _pre()._channels_on_device(x)
    assert got.shape == (*x.shape, 3) and got.dtype == np.float32
    err, err_ref = pc.check_images(got, x, case.id)
    print(f"{case.id}: device error {err}, err_ref {err_ref}")


# ------------------------------------------------------------------ the gather form against the oracle's own tiling
def _waterfall(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    z = ((rng.normal(size=shape) + 1j * rng.normal(size=shape)) * 10.0 ** rng.uniform(-4, 4, size=shape)).astype(dtype)
    fl = rng.random(shape) < 0.02
    fl[..., : shape[-2] // 3, :] = False                    # leaves some tiles blank
    return z, fl


def _flag_form(fl, form, seed):
    """The same flags as uint8 with values other than 1, or as float: non-zero is RFI."""
    rng = np.random.default_rng(seed)
    if form == "u8":
        return np.where(fl, rng.choice(np.array([1, 2, 128, 255], np.uint8), size=fl.shape), 0).astype(np.uint8)
    return np.where(fl, rng.choice(np.array([0.5, -2.0, 1e-30, np.inf], np.float32), size=fl.shape), 0).astype(np.float32)


WF_A, WF_B = (1, 2, 200, 300), (1, 1, 256, 130)
GATHER = [(WF_A, 128, 1, np.complex128, "u8", {}), (WF_A, 128, 2, np.complex64, "f32", {}),
          (WF_A, 128, 4, np.complex128, "f32", {}), (WF_A, 128, 4, np.complex64, "u8", {}),
          (WF_A, 256, 1, np.complex64, "u8", {}), (WF_A, 256, 2, np.complex128, "f32", {}),
          (WF_A, 256, 4, np.complex128, "u8", {}), (WF_A, 256, 4, np.complex64, "f32", {}),
          (WF_B, 128, 1, np.complex64, "f32", {}), (WF_B, 128, 2, np.complex128, "u8", {}),
          (WF_B, 128, 4, np.complex128, "f32", {}), (WF_B, 128, 4, np.complex64, "u8", {}),
          (WF_A, 128, 4, np.complex128, "u8", {"num_patches": 5}), (WF_B, 128, 2, np.complex64, "f32", {"num_patches": 3}),
          (WF_A, 128, 4, np.complex64, "u8", {"inference_mode": True}), (WF_B, 128, 4, np.complex128, "f32", {"inference_mode": True})]


@pytest.mark.parametrize("shape,ps,rot,dtype,form,kw", GATHER,
                         ids=[f"{s[2]}x{s[3]}-ps{p}-rot{r}-{pc.DTYPE_TAG[d]}-{f}" + "".join(f"-{k}" for k in kw)
                              for s, p, r, d, f, kw in GATHER])
def test_gather_form_against_the_oracles_tiling(shape, ps, rot, dtype, form, kw):
    """Views, zero-padded tiling, blank-patch removal, shuffle and labels from the waterfall on the device against
    preprocess_ref.create_dataset under the same np.random.seed: labels bit-equal, images within the channel bounds."""
    from rfi_toolbox_amd.preprocessing import Preprocessor
    z, fl = _waterfall(shape, dtype, seed=ps + rot + shape[-1])
    okw = dict(patch_size=ps, augmentation_rotations=rot, enable_augmentation=rot > 1, **kw)
    np.random.seed(41)
    want64, lab = preprocess_ref.create_dataset(z.astype(np.complex128), fl, **okw)
    want32 = None
    if dtype == np.complex64:
        np.random.seed(41)
        want32, lab32 = preprocess_ref.create_dataset(z, fl, **okw)
        assert np.array_equal(lab, lab32)
    np.random.seed(41)
    pre = Preprocessor(z, flags=_flag_form(fl, form, seed=ps))
    ds = pre.create_dataset(patch_size=ps, augmentation_rotations=rot, enable_augmentation=rot > 1, **kw)
    assert pre._table is not None                                       # the gather kernels really ran
    got, got_lab = ds.images.numpy(), ds.labels.numpy()
    assert got.shape == want64.shape and len(got) > 0
    if kw.get("num_patches"):
        assert len(got) == kw["num_patches"]
    assert np.array_equal(got_lab, lab) and got_lab.dtype == np.uint8
    assert kw.get("inference_mode") or got_lab.any()
    nan_ok, err, bound, err_ref = pc.image_errors(got, want64, want32)
    print(f"device error {err}, err_ref {err_ref}")
    assert nan_ok and (err <= bound).all(), (err, bound)


# ------------------------------------------------------------------ the radix-selection median on its own
def _patch_median(v, absdev_centre, finite_only, f32):
    from rfi_toolbox_amd._lib import check, lib
    from rfi_toolbox_amd.runtime import Context, P
    ctx = Context.get(0)
    n, per = v.shape
    dv = ctx.to_device(np.ascontiguousarray(v, np.float64))
    dc = ctx.to_device(np.ascontiguousarray(absdev_centre, np.float64)) if absdev_centre is not None else None
    med, cnt = ctx.to_device(np.full(n, -7.0)), ctx.to_device(np.full(n, -7, np.int32))
    check(lib.rfi_op_patch_median(ctx.handle, P(dv), n, per, 1 if dc is not None else 0, P(dc), 1 if finite_only else 0,
                                  1 if f32 else 0, P(med), P(cnt)))
    return med.numpy(), cnt.numpy()


@pytest.mark.parametrize("f32", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("per", pc.MEDIAN_PERS)
def test_patch_median_is_numpys_bit_for_bit(per, f32):
    """rfi_op_patch_median, eight patches per call, every content kind, plain and as |v - centre|: the median equals
    np.nanmedian / np.median(np.abs(v - c)) in the data's own arithmetic (float64, or float32 widened) bit for bit -- NaN
    where NumPy gives NaN; NumPy's order does not tell -0.0 from 0.0, so neither does the comparison -- and the
    participant count is exact."""
    for kind in pc.MEDIAN_KINDS:
        v, finite_only, native = pc.median_stack(kind, per, bool(f32))
        want, want_n = pc.median_expected(native, finite_only)
        got, got_n = _patch_median(v, None, finite_only, f32)
        assert np.array_equal(got_n, want_n), (kind, got_n, want_n)
        assert np.array_equal(got, want, equal_nan=True), (kind, got, want)
        centre = np.where(np.isfinite(want), want, 0.0).astype(native.dtype)
        want, want_n = pc.median_expected(native, finite_only, centre)
        got, got_n = _patch_median(v, centre.astype(np.float64), finite_only, f32)
        assert np.array_equal(got_n, want_n), (kind, "absdev", got_n, want_n)
        assert np.array_equal(got, want, equal_nan=True), (kind, "absdev", got, want)


# ------------------------------------------------------------------ thresholds through the public entries, planted pixels
def _assert_planted(flags, planted, what):
    for seed, pl in enumerate(planted):
        got = flags[seed].astype(bool)
        at = got.ravel()[pl.index].tolist()
        assert at == [False, True, False, True], f"{what} seed {seed}: pixels at hi, hi+, lo, lo- flagged {at}"
        assert np.array_equal(got, pl.flags), f"{what} seed {seed}: {np.count_nonzero(got != pl.flags)} flags differ from NumPy's"


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=[pc.DTYPE_TAG[d] for d in pc.DTYPES])
def test_mad_flags_at_planted_thresholds(dtype):
    """rfi_mad_flags with pixels exactly on and one ulp beyond med +- 5 mad, the thresholds NumPy forms in the input's own
    arithmetic (float32 for complex64 / float32): on-threshold pixels unflagged, the next ones flagged, whole map equal."""
    planted = [pc.planted_patch(s, dtype) for s in pc.PLANT_SEEDS]
    flags = _pre()._mad_flags_on_device(np.stack([pl.patch for pl in planted]), 5)
    _assert_planted(flags, planted, f"mad_flags {pc.DTYPE_TAG[dtype]}")


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=[pc.DTYPE_TAG[d] for d in pc.DTYPES])
def test_mad_flags_at_sigma_zero_pin_the_median(dtype):
    """sigma = 0: hi == lo == med, so exactly the pixels tied at the median stay unflagged."""
    pairs = [pc.tied_patch(s, dtype) for s in pc.PLANT_SEEDS]
    flags = _pre()._mad_flags_on_device(np.stack([x for x, _ in pairs]), 0)
    for seed, (_, want) in enumerate(pairs):
        assert np.array_equal(flags[seed].astype(bool), want), seed


@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "norm"])
@pytest.mark.parametrize("stretch", [None, "SQRT"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_preprocess_real_flags_at_planted_thresholds(dtype, stretch, normalize):
    """rfi_preprocess_real's flags are those of the PROCESSED patch (median-normalised, stretched): the planted pixels sit
    on its thresholds."""
    planted = [pc.planted_patch(s, dtype, stretch, normalize) for s in pc.PLANT_SEEDS]
    x = np.stack([pl.patch for pl in planted])
    images, flags = _pre()._real_on_device(x, stretch, normalize, False, 5)
    _assert_planted(flags, planted, f"preprocess_real {pc.DTYPE_TAG[dtype]} {stretch} normalize={normalize}")
    want64, want32 = pc.reference_images(np.stack([pl.processed for pl in planted]))
    nan_ok, err, bound, _ = pc.image_errors(images, want64, want32)
    assert nan_ok and (err <= bound).all(), (err, bound)


# ------------------------------------------------------------------ degenerate patches
def _quiet(fn, *a, **k):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        return fn(*a, **k)


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=[pc.DTYPE_TAG[d] for d in pc.DTYPES])
def test_all_nan_patch_gives_no_flags(dtype):
    rng = np.random.default_rng(2)
    x = np.abs(8 + rng.normal(size=(3, 16, 17)))
    x[2, 4, 4] = 100.0
    x = x.astype(dtype)
    x[1] = np.nan
    x[0, 3, 3] = np.nan                                      # one NaN: skipped by the statistics, never flagged
    flags = _pre()._mad_flags_on_device(x, 5)
    want = _quiet(preprocess_ref.mad_flags, np.abs(x), 5)
    assert not flags[1].any() and flags[2, 4, 4] and not flags[0, 3, 3]
    assert np.array_equal(flags, want)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_log10_of_zeros_is_filled_with_the_mad_of_the_finite_values(dtype):
    """LOG10 stretch: -inf pixels <- the MAD of the patch's finite values; a patch with no finite value <- 0."""
    rng = np.random.default_rng(3)
    x = rng.lognormal(0.0, 1.0, size=(4, 24, 20))
    x[0, 2:5, 3:9] = 0.0                                     # some zeros
    x[1] = 0.0                                               # nothing finite after the stretch
    x[2, ::2] = 0.0                                          # half zeros
    x[3, 0, 0] = np.nan
    x[3, 5, 5] = 0.0
    x = x.astype(dtype)
    proc = _quiet(preprocess_ref.stretch, x, "LOG10")
    assert proc.dtype == dtype and (proc[1] == 0).all() and np.isfinite(proc[0]).all()
    assert proc[0, 2, 3] == _quiet(preprocess_ref._mad, proc[0][x[0] != 0])
    want_flags = _quiet(preprocess_ref.mad_flags, proc, 4)
    images, flags = _pre()._real_on_device(x, "LOG10", False, False, 4)
    assert want_flags.any() and np.array_equal(flags, want_flags)
    want64, want32 = pc.reference_images(proc)               # the channels of the oracle's processed patches
    nan_ok, err, bound, err_ref = pc.image_errors(images, want64, want32)
    print(f"device error {err}, err_ref {err_ref}")
    assert nan_ok and (err <= bound).all(), (err, bound)


# ------------------------------------------------------------------ more patches than one launch's gridDim.y holds
N_LARGE = 66000


def _large_stack(dtype):
    rng = np.random.default_rng(11)
    idx = np.arange(N_LARGE, dtype=np.float64)[:, None, None]
    amp = (1.0 + (idx % 977) * 0.01) * rng.lognormal(0.0, 0.5, size=(N_LARGE, 4, 4))      # content depends on the patch index
    if np.dtype(dtype).kind == "c":
        return (amp * np.exp(1j * rng.uniform(-np.pi, np.pi, size=amp.shape))).astype(dtype)
    amp[::3, 1, 2] *= 50.0                                   # every third patch has a pixel for the MAD flags
    return amp


def test_large_patch_count_complex_channels():
    """66,000 patches of 4 x 4 through rfi_preprocess_patches: past the 65,535 of gridDim.y, so the launchers chunk."""
    z = _large_stack(np.complex128)
    got = _pre()._channels_on_device(z)
    want = preprocess_ref.images_of(preprocess_ref.channels(z))
    d = np.abs(got.astype(np.float64) - want).reshape(N_LARGE, -1).max(axis=1)
    bad = np.flatnonzero(~(d <= pc.ATOL_64))
    assert bad.size == 0, f"{bad.size} patches off, first {bad[:5]}, last {bad[-5:]}, max {np.nanmax(d)}"


def test_large_patch_count_real_with_flags():
    """The same count through rfi_preprocess_real with median normalisation and MAD flags (float64).  The oracle's
    per-patch loops run on the patches around the chunk boundary and at both ends; the whole stack is held to their
    array-at-once restatement, which must agree with them there."""
    x = _large_stack(np.float64)
    images, flags = _pre()._real_on_device(x, None, True, False, 5)
    flat = x.reshape(N_LARGE, -1)
    med = np.median(flat, axis=1)
    proc = x / np.where(med > 0, med, 1.0)[:, None, None]
    pf = proc.reshape(N_LARGE, -1)
    m = np.median(pf, axis=1)
    mad = np.median(np.abs(pf - m[:, None]), axis=1)
    want_flags = ((pf > (m + mad * 5)[:, None]) | (pf < (m - mad * 5)[:, None])).reshape(x.shape)
    near = np.r_[0:64, 65535 - 64:65535 + 64, N_LARGE - 64:N_LARGE]
    assert np.array_equal(preprocess_ref.median_normalise(x[near]), proc[near])
    assert np.array_equal(preprocess_ref.mad_flags(proc[near], 5), want_flags[near])
    assert want_flags.any(axis=(1, 2)).sum() > N_LARGE // 4
    bad = np.flatnonzero((flags != want_flags).any(axis=(1, 2)))
    assert bad.size == 0, f"flags of {bad.size} patches differ, first {bad[:5]}, last {bad[-5:]}"
    want = preprocess_ref.images_of(preprocess_ref.channels(proc))
    d = np.abs(images.astype(np.float64) - want).reshape(N_LARGE, -1).max(axis=1)
    bad = np.flatnonzero(~(d <= pc.ATOL_64))
    assert bad.size == 0, f"{bad.size} patches off, first {bad[:5]}, last {bad[-5:]}, max {np.nanmax(d)}"


# ------------------------------------------------------------------ confusion counts
F32_PALETTE = np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-39, np.nan, np.inf, -np.inf, 1.0, -2.5, 0.0, 0.0], np.float32)
U8_PALETTE = np.array([0, 0, 0, 1, 2, 255], np.uint8)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 257, 2048 * 256 * 8 + 12345])
def test_confusion_counts_of_odd_values_and_sizes(count):
    """Non-zero is positive: -0.0 is not, subnormals, NaN and infinities are; element counts around the wave and block
    sizes, and one past 2048 blocks x 256 threads x 8, where the grid-stride loop wraps."""
    from rfi_toolbox_amd.evaluation import confusion_counts
    rng = np.random.default_rng(count)
    f = F32_PALETTE[rng.integers(0, len(F32_PALETTE), size=count)]
    u = U8_PALETTE[rng.integers(0, len(U8_PALETTE), size=count)]
    assert confusion_counts(f, u) == metrics_ref.confusion(f, u)
    assert confusion_counts(u, f) == metrics_ref.confusion(u, f)
    g = F32_PALETTE[rng.integers(0, len(F32_PALETTE), size=count)]
    assert confusion_counts(f, g) == metrics_ref.confusion(f, g)
    if count > 8:
        tp, fp, fn = metrics_ref.confusion(f, u)
        assert tp > 0 and fp > 0 and fn > 0
