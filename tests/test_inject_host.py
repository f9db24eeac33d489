"""CPU: the NumPy restatement of RFISimulator.inject (tests/inject_ref.py) against RefSimulator itself and against the
rules of include/rfi_hip.h ("rfi_sim_inject"), on the seed, shapes and sample counts tests/test_gpu_inject.py uses; and the
argument checks of the C entry points and of RFISimulator.inject that need no GPU."""
import functools

import numpy as np
import pytest

from inject_ref import IQR_PER_SIGMA, RefInjector, background, iqr_sigma, valid_scalars
from rfisim_ref import RefSimulator

SEED = 0x5EED_1234_ABCD                     # tests/test_gpu_inject.py: the same seed, shapes and samples per shape
SHAPES = ((4, 52), (24, 300), (12, 1300), (650, 52))
N = 3


def _bytes(a):
    """(..., itemsize) uint8: the bytes of every element"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))


@functools.lru_cache(maxsize=None)
def _injected(shape, ring):
    """N samples at `shape` injected into a non-noise background -> [(data, out, mask, touched, ambiguous, chunks)]"""
    T, F = shape
    ref = RefInjector(T, F, seed=SEED)
    ref.gibbs_ringing = ring
    data = background(N, T, F, seed=5, scale=3.7e-3)
    res = []
    for i in range(N):
        out, mask = ref.inject(data[i], scale=3.7e-3)
        res.append((data[i], out, mask, ref.touched, ref.ambiguous, int(ref.events["i0"][0])))
    return res


@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("shape", [(4, 52), (24, 300)])
def test_unit_scale_reference_mode_on_own_noise_is_generate_rfi(shape, ring):
    T, F = shape
    gen, inj, noise = RefSimulator(T, F, seed=SEED), RefInjector(T, F, seed=SEED), RefSimulator(T, F, seed=SEED)
    gen.gibbs_ringing = inj.gibbs_ringing = ring
    for i in range(N):
        noise.generate_clean_data()
        gen.generate_rfi()
        out, mask = inj.inject(noise.planes(), scale=1.0, cross_hand="reference")
        assert np.array_equal(_bytes(out), _bytes(gen.planes())), i
        assert np.array_equal(mask, gen.mask) and np.array_equal(inj.events, gen.events)
        assert inj.baseline_frac == gen.baseline_frac and inj.sample_counter == gen.sample_counter


@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_no_ambiguous_pixel_on_the_gpu_tests_seed(shape, ring):
    for data, out, mask, touched, amb, chunks in _injected(shape, ring):
        assert int(amb.sum()) == 0
        assert mask.any() and touched[0].any()


def test_two_and_three_broadband_chunks_are_covered():
    chunks = [r[5] for r in _injected((24, 300), False)]
    assert 2 in chunks and 3 in chunks, chunks


@pytest.mark.parametrize("ring", [False, True])
def test_untouched_pixels_keep_their_bytes(ring):
    T, F = 24, 300
    data = background(1, T, F, seed=9, dtype=np.complex64)[0]
    plain = RefInjector(T, F, seed=SEED)
    plain.gibbs_ringing = ring
    plain.inject(data, scale=2.0)
    free = ~plain.touched
    assert free[0].any() and free[3].any() and np.array_equal(free[1], free[0]) and np.array_equal(free[2], free[0])
    assert not (free[0] & ~free[3]).any()                        # (LL gets what RR gets but the quadratic sweeps, nothing else)
    # -0.0, NaN with a payload, a signalling NaN and infinities on visibilities nothing touches, and on some that are touched
    words = np.array([0x80000000, 0x7FC12345, 0x7F800001, 0x7F800000, 0xFF800000], dtype=np.uint32).view(np.float32)
    raw = data.copy()
    parts = raw.view(np.float32).reshape(4, T * F, 2)            # (a view: re, im of every visibility)
    for p in range(4):
        idx = np.flatnonzero(free[p].ravel())[:5]
        parts[p, idx, 0] = words
        parts[p, idx[::-1], 1] = words
    hit = np.flatnonzero(plain.touched[0].ravel())[:2]
    parts[0, hit, 0] = words[1]
    inj = RefInjector(T, F, seed=SEED)
    inj.gibbs_ringing = ring
    out, _ = inj.inject(raw, scale=2.0)
    assert np.array_equal(inj.touched, plain.touched)
    assert np.array_equal(_bytes(out)[free], _bytes(raw)[free])
    assert np.isnan(out[0].real.ravel()[hit]).all()              # without flags a non-finite value propagates by IEEE rules
    changed = (_bytes(out) != _bytes(raw)).any(axis=-1)
    assert changed.any() and not (changed & free).any()


@pytest.mark.parametrize("per_pol", [True, False])
def test_flagged_visibilities_keep_their_bytes_and_do_not_change_the_rest(per_pol):
    T, F = 24, 300
    data = background(1, T, F, seed=3)[0]
    rng = np.random.default_rng(1)
    flags = rng.random((4, T, F) if per_pol else (T, F)) < 0.3
    a, b = RefInjector(T, F, seed=SEED), RefInjector(T, F, seed=SEED)
    want, mask_plain = a.inject(data, scale=0.5)
    got, mask = b.inject(data, flags=flags, scale=0.5)
    fl = np.broadcast_to(flags, data.shape)
    assert np.array_equal(_bytes(got)[fl], _bytes(data)[fl])
    assert np.array_equal(_bytes(got)[~fl], _bytes(want)[~fl])   # S does not depend on RR's flag: RL / LR under a flagged RR too
    assert np.array_equal(mask, mask_plain)                      # the truth is the injection truth, also under a flag
    assert not per_pol or (fl[0] & ~fl[1] & a.touched[1]).any()


@pytest.mark.parametrize("cross_hand", ["injected", "reference"])
@pytest.mark.parametrize("ring", [False, True])
def test_channel_rows_are_the_transpose(ring, cross_hand):
    T, F = 24, 300
    data = background(1, T, F, seed=4)[0]
    a, b = RefInjector(T, F, seed=SEED), RefInjector(T, F, seed=SEED)
    a.gibbs_ringing = b.gibbs_ringing = ring
    want, want_mask = a.inject(data, scale=41.0, cross_hand=cross_hand)
    got, got_mask = b.inject(np.ascontiguousarray(data.transpose(0, 2, 1)), scale=41.0, rows="channel", cross_hand=cross_hand)
    assert got.shape == (4, F, T) and got_mask.shape == (F, T)
    assert np.array_equal(_bytes(got.transpose(0, 2, 1)), _bytes(want)) and np.array_equal(got_mask.T, want_mask)
    assert np.array_equal(b.touched.transpose(0, 2, 1), a.touched)


def test_injected_cross_hands_take_the_injected_part_only():
    T, F = 24, 300
    data = background(1, T, F, seed=6)[0]
    a = RefInjector(T, F, seed=SEED)
    out, _ = a.inject(data, scale=1.0)
    zero = RefInjector(T, F, seed=SEED)
    alone, _ = zero.inject(np.zeros_like(data), scale=1.0)        # the injected part by itself: S = RR, cross = factor S
    t = a.touched
    for p in range(4):
        err = np.abs((out[p] - data[p])[t[p]] - alone[p][t[p]]).max()
        assert err <= 1e-12 * np.abs(alone[p]).max(), (p, err)


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_iqr_sigma_is_numpy_percentile_on_the_valid_scalars(dtype):
    data = background(2, 24, 300, seed=8, dtype=dtype, scale=0.02)
    flags = np.random.default_rng(2).random((2, 24, 300)) < 0.2
    data[0, 1, 3, 5] = np.nan
    data[0, 2, 4, 7] = complex(1.0, np.inf)
    for i in range(2):
        for fl in (None, flags[i]):
            x = valid_scalars(data[i], fl)
            assert x.dtype == np.float64 and np.isfinite(x).all()
            assert x.size == 2 * (np.isfinite(data[i].real) & np.isfinite(data[i].imag) & ~(False if fl is None else fl)).sum()
            q75, q25 = np.percentile(x, [75, 25])
            assert iqr_sigma(data[i], fl) == (q75 - q25) / IQR_PER_SIGMA
    assert abs(iqr_sigma(data[1]) / 0.02 - 1.3) < 0.5              # (noise sigma 0.02 under a bandpass of the same order)
    assert np.isnan(iqr_sigma(data[0], np.ones((4, 24, 300), bool)))
    inj = RefInjector(24, 300, seed=SEED)
    inj.inject(data[0], flags=flags[0])
    assert inj.noise_scale == iqr_sigma(data[0], flags[0])
    with pytest.raises(ValueError):
        inj.inject(data[0], flags=np.ones((24, 300), bool))


def test_entry_points_are_bound_and_refuse_null_arguments():
    from rfi_toolbox_amd import _lib
    for name, nargs in (("rfi_sim_inject", 17), ("rfi_sim_transpose_planes", 6)):
        assert len(_lib._PROTOS[name][1]) == nargs and hasattr(_lib.lib, name)
    assert _lib.lib.rfi_sim_inject(None, 0, 0, 1, None, None, 0, 0, 0, None, None, 0, None, None, None, None, None) != 0
    assert b"sim_inject" in _lib.lib.rfi_last_error()
    assert _lib.lib.rfi_sim_transpose_planes(None, None, 1, 4, 4, None) != 0


def test_inject_checks_its_arguments_before_any_device_is_touched():
    from rfi_toolbox_amd.core import RFISimulator
    T, F = 24, 300
    sim = RFISimulator(T, F, seed=1)
    good = np.zeros((2, 4, T, F), np.complex64)
    bad = [dict(data=np.zeros((2, 4, T, F + 1), np.complex64)),                     # wrong plane size
           dict(data=np.zeros((2, 4, F, T), np.complex64)),                         # the other orientation without rows="channel"
           dict(data=np.zeros((2, 4, T, F), np.complex64), rows="channel"),
           dict(data=np.zeros((2, 3, T, F), np.complex64)),                         # three polarisations
           dict(data=good, flags=np.zeros((2, 4, T, F), np.uint8), cross_hand="reference"),
           dict(data=good, flags=np.zeros((2, T, F + 1), np.uint8)),
           dict(data=good, scale=0.0), dict(data=good, scale=-1.0), dict(data=good, scale=np.array([1.0, np.nan])),
           dict(data=good, scale=np.ones(3)), dict(data=good, scale="mad"),
           dict(data=good, rows="freq"), dict(data=good, cross_hand="both"), dict(data=good, inplace=True)]
    for kw in bad:
        kw = dict({"scale": 1.0}, **kw)
        with pytest.raises(ValueError):
            sim.inject(**kw)
    for kw in (dict(data=np.zeros((2, 4, T, F), np.float32)), dict(data=good, flags=np.zeros((2, T, F), np.float32))):
        with pytest.raises(TypeError):
            sim.inject(scale=1.0, **kw)
    with pytest.raises(ValueError, match="sample 1"):
        sim.inject(good, scale=np.array([1.0, 0.0]))
    assert sim._ctx is None and sim.sample_counter == 0
