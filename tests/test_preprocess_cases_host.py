"""CPU-only: the case tables of preprocess_cases.py cover what they claim, and the criteria of
test_gpu_preprocess_kernels.py can fail -- seam coverage of the channel-kernel shapes, the planted-threshold
construction (median and MAD untouched; float32 and float64 arithmetic told apart), and the rejection of a known-wrong
form of the real-input log-amplitude channel."""
import numpy as np
import pytest

import preprocess_cases as pc
from oracle import preprocess_ref


# ------------------------------------------------------------------ the channel-kernel table
def test_npb_restates_the_launcher():
    """The formula as csrc/preprocess.hip has it, at the values the table's comments quote."""
    assert pc.npb(128, 8) == 2048 and pc.npb(256, 8) == 2048 and pc.npb(256, 4) == 2048
    assert pc.npb(2500, 8) == 5692 and pc.npb(2500, 4) == 10000
    assert pc.npb(4096, 8) == 4096 and pc.npb(4096, 4) == 12288        # a 64-bit row of 4096 still fits (npb >= pw); 4097 does not
    assert pc.npb(4097, 8) < 4097
    for ph, pw in pc.SHAPES:
        for esz in (8, 4):
            assert pc.npb(pw, esz) >= pw and (pw + pc.npb(pw, esz)) * esz <= 64 * 1024


def test_table_contains_every_seam_class():
    seen = {esz: set() for esz in (8, 4)}
    per_shape = {}
    for ph, pw in pc.SHAPES:
        for esz in (8, 4):
            per_shape[(ph, pw, esz)] = pc.seam_classes(ph, pw, esz)
            seen[esz] |= per_shape[(ph, pw, esz)]
    for esz in (8, 4):
        assert {"row-aligned", "mid-row", "single-block", "wide-row", "cap-active", "ragged-last", "block-over-two-rows",
                "under-one-wave"} <= seen[esz], (esz, seen[esz])
    assert per_shape[(128, 128, 8)] == {"row-aligned"} and 128 * 128 // pc.npb(128, 8) == 8
    assert per_shape[(256, 256, 8)] == {"row-aligned"} and 256 * 256 // pc.npb(256, 8) == 32
    assert {"mid-row", "ragged-last"} <= per_shape[(80, 96, 8)] and {"mid-row", "ragged-last"} <= per_shape[(257, 33, 4)]
    assert {"wide-row", "cap-active", "mid-row", "block-over-two-rows"} <= per_shape[(3, 2500, 8)]
    assert {"wide-row", "single-block"} <= per_shape[(3, 2500, 4)]
    assert per_shape[(4096, 1, 8)] == {"row-aligned"}
    assert {"single-block", "cap-active", "wide-row"} <= per_shape[(1, 4096, 8)]
    # every shape x dtype x group is a case, three patches each, ids unique
    assert len(pc.CASES) == len(pc.SHAPES) * 4 * 3 == len({c.id for c in pc.CASES})
    kinds = {(np.dtype(c.dtype).kind, k) for c in pc.CASES for k in c.kinds}
    for k in ("wide", "zeros", "const", "nonfinite-interior", "nonfinite-seam", "all-nan"):
        assert ("c", k) in kinds and ("f", k) in kinds
    assert {("c", "phase-pi"), ("c", "zero0j"), ("f", "lowc-1e-2"), ("f", "lowc-1e-4")} <= kinds


@pytest.mark.parametrize("case", [c for c in pc.CASES if c.shape in ((80, 96), (3, 2500), (2, 2), (1, 1))], ids=lambda c: c.id)
def test_patches_hold_what_their_kind_says(case):
    x = pc.make_patches(case)
    assert x.shape == (3, *case.shape) and x.dtype == np.dtype(case.dtype)
    assert not np.array_equal(x[0], x[2], equal_nan=True) or case.shape == (1, 1)
    ph, pw = case.shape
    esz, per = pc.esz_of(case.dtype), ph * pw
    n = pc.npb(pw, esz)
    for i, kind in enumerate(case.kinds):
        p = x[i].ravel()
        amp = np.abs(p)
        if kind == "all-nan":
            assert np.isnan(amp).all()
        elif kind == "const":
            assert (amp == amp[0]).all()
        elif kind == "zeros" and per > 16:
            assert (amp == 0).any() and (amp > 0).any()
        elif kind == "wide" and per > 1000:
            assert amp.min() < 1e-4 and amp.max() > 1e4                 # channel 1 of complex input clips at both ends
        elif kind == "phase-pi" and per > 16:
            neg = p.real < 0
            assert (neg & (p.imag == 0) & np.signbit(p.imag)).any() and (neg & (p.imag == 0) & ~np.signbit(p.imag)).any()
        elif kind == "zero0j":
            assert p[0] == 0
        elif kind.startswith("lowc"):
            la = np.log10(amp.astype(np.float64))
            assert per == 1 or (0 < la.max() - la.min() < 0.1 and abs(la.mean() - 3) < 0.1)
        elif kind.startswith("nonfinite") and per > 1:
            a, b = pc.nonfinite_positions(kind, ph, pw, esz)
            assert np.isnan(amp[a]) and np.isinf(amp[b]) and np.isnan(amp).sum() == 1 and np.isinf(amp).sum() == 1
            if kind == "nonfinite-seam" and per > n:
                assert n - pw <= a < n                                   # the halo row of the second block
                assert b // n >= 1 and b % n < pw                        # the first row of a later block


def test_reference_of_the_table_is_well_formed():
    """The oracle runs on every case (NaN / inf content included) and the float32 restatement stays in float32."""
    for case in pc.CASES:
        if case.shape[0] * case.shape[1] > 8000:
            continue
        want64, want32 = pc.reference_images(pc.make_patches(case))
        assert want64.dtype == np.float32 and (want32 is None) == (pc.esz_of(case.dtype) == 8)
        if want32 is not None:
            assert np.array_equal(np.isnan(want32), np.isnan(want64)), case.id
        for i, kind in enumerate(case.kinds):
            ch0 = want64[i, ..., 0] * preprocess_ref.IMAGENET_STD[0] + preprocess_ref.IMAGENET_MEAN[0]
            if kind == "const":
                assert np.abs(ch0).max() < 1e-6                           # flat patch: channel 0 is 0
                if np.dtype(case.dtype).kind == "f":
                    ch1 = want64[i, ..., 1] * preprocess_ref.IMAGENET_STD[1] + preprocess_ref.IMAGENET_MEAN[1]
                    assert np.abs(ch1).max() < 1e-6                       # and for real input channel 1 as well


# ------------------------------------------------------------------ the criterion can fail
@pytest.mark.parametrize("kind,floor", [("lowc-1e-2", 2e-5), ("lowc-1e-4", 2e-3)])
def test_criterion_rejects_a_float32_stored_log_amplitude(kind, floor):
    """Real float64 input whose log-amplitude is rounded to float32 before the per-patch min-max (what the channel
    kernels did) loses channel 1 on low-contrast patches: about 6e-8 |la| / span.  The 64-bit criterion must say so, and
    must accept the float64 form."""
    x = np.stack([pc.make_patch(kind, (32, 32), np.float64, s) for s in (1, 2)])
    want64, _ = pc.reference_images(x)
    wrong = pc.emulate_f32_stored_logamp(x)
    nan_ok, err, bound, _ = pc.image_errors(wrong, want64)
    assert nan_ok and err[1] > floor > bound[1] and err[0] <= bound[0] and err[2] <= bound[2], err
    with pytest.raises(AssertionError, match="over the bound"):
        pc.check_images(wrong, x)
    pc.check_images(want64, x)
    # on ordinary contrast the same wrong form passes: the low-contrast patches are what sees it
    y = np.stack([pc.make_patch("wide", (32, 32), np.float64, 3)])
    pc.check_images(pc.emulate_f32_stored_logamp(y), y)


def test_criterion_sees_nan_positions_and_32_bit_bound():
    case = next(c for c in pc.CASES if c.id == "80x96-c64-B")
    x = pc.make_patches(case)
    want64, want32 = pc.reference_images(x)
    pc.check_images(want32, x)                                            # NumPy's own float32 result is within its bound
    bad = want32.copy()
    bad[1][np.isnan(bad[1])] = 0.0
    with pytest.raises(AssertionError, match="NaN positions"):
        pc.check_images(bad, x)
    bad = want32.copy()
    bad[0, 5, 5, 2] += 1e-4
    with pytest.raises(AssertionError, match="over the bound"):
        pc.check_images(bad, x)


# ------------------------------------------------------------------ planted thresholds
PLANT_CONFIGS = [(dt, None, False) for dt in pc.DTYPES] + \
                [(dt, st, nb) for dt in (np.float64, np.float32) for st in (None, "SQRT") for nb in (False, True)]


@pytest.mark.parametrize("dtype,stretch,normalize", PLANT_CONFIGS,
                         ids=[f"{pc.DTYPE_TAG[d]}-{s}-{'norm' if n else 'raw'}" for d, s, n in PLANT_CONFIGS])
def test_planted_pixels_leave_median_and_mad_bit_identical(dtype, stretch, normalize):
    rt = pc.real_dtype(dtype)
    for seed in pc.PLANT_SEEDS:
        pl = pc.planted_patch(seed, dtype, stretch, normalize)
        assert pl.patch.dtype == np.dtype(dtype) and pl.processed.dtype == rt
        if np.dtype(dtype).kind == "c":                                   # exactly representable amplitudes
            assert ((pl.patch.real == 0) | (pl.patch.imag == 0)).all()
        assert np.median(np.abs(pl.patch)) == pc.MEDIAN_AT
        again = pc.processed_of(pl.patch, stretch, normalize)
        assert np.array_equal(again, pl.processed)
        med, mad, hi, lo = pc.thresholds(again, 5)
        for a, b in ((med, pl.med), (mad, pl.mad), (hi, pl.hi), (lo, pl.lo)):
            assert np.asarray(a).dtype == rt and np.asarray(a).tobytes() == np.asarray(b).tobytes()
        assert np.array_equal(again.ravel()[pl.index], pl.targets)
        assert pl.targets[0] == hi and pl.targets[1] > hi and pl.targets[2] == lo and pl.targets[3] < lo
        assert pl.flags.ravel()[pl.index].tolist() == [False, True, False, True]
        assert 2 <= pl.flags.sum() < 64                                   # the two planted ones and the patch's own few outliers


@pytest.mark.parametrize("dtype", [np.complex64, np.float32], ids=["c64", "f32"])
def test_planted_pixels_tell_float32_from_float64_arithmetic(dtype):
    """The same float32 amplitudes, thresholds formed in float64 (what rfi_mad_flags did for 32-bit input): the flag map
    must differ from the float32 one for at least half of the seeds, else the device test could not tell the two apart."""
    differ = 0
    for seed in pc.PLANT_SEEDS:
        pl = pc.planted_patch(seed, dtype)
        amp = np.abs(pl.patch)
        assert amp.dtype == np.float32
        f64 = preprocess_ref.mad_flags(amp.astype(np.float64)[None], 5)[0]
        differ += int(not np.array_equal(f64, pl.flags))
    assert differ >= len(pc.PLANT_SEEDS) // 2, differ


def test_tied_patch_pins_the_median_at_sigma_zero():
    for dtype in pc.DTYPES:
        x, flags = pc.tied_patch(0, dtype)
        amp = np.abs(x)
        med = np.median(amp)
        assert 10 < (amp == med).sum() == (~flags).sum()                  # unflagged == the pixels tied at the median
        s = np.sort(amp.ravel())
        for wrong in (s[len(s) // 2 - 200], s[len(s) // 2 + 200]):       # a median some ranks off flags other pixels
            assert not np.array_equal(amp != wrong, flags)


# ------------------------------------------------------------------ the median stacks
def test_median_stacks_are_what_they_say():
    for f32 in (False, True):
        for per in pc.MEDIAN_PERS:
            for kind in pc.MEDIAN_KINDS:
                v, finite_only, native = pc.median_stack(kind, per, f32)
                assert v.shape == (8, per) and v.dtype == np.float64 and native.dtype == (np.float32 if f32 else np.float64)
                assert np.array_equal(v, native.astype(np.float64), equal_nan=True)
                med, cnt = pc.median_expected(native, finite_only)
                assert med.shape == (8,) and (cnt >= 0).all() and (cnt <= per).all()
                if kind == "nans":
                    assert cnt[2] == 0 and np.isnan(med[2]) and cnt[0] == per - 1 and cnt[1] == min(1, per)
                if kind == "infinities" and per >= 2 and per % 2 == 0:
                    assert np.isnan(med[0]) and cnt[0] == per              # (-inf + inf) / 2
                if kind == "finite-only":
                    assert np.isfinite(med[cnt > 0]).all()
                if kind == "subnormal" and per > 3:
                    assert (np.abs(native[native != 0]) < np.finfo(native.dtype).tiny).all()
                if kind == "low-byte":
                    u = native.view(np.uint32 if f32 else np.uint64)
                    assert ((u >> 8) == (u[:, :1] >> 8)).all()
