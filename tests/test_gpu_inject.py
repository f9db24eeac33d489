"""-m gpu: RFISimulator.inject (rfi_sim_inject of csrc/rfi_sim.hip) -- simulated emitters added to visibilities that already
exist -- against the generating kernel bit for bit, against the NumPy restatement tests/inject_ref.py, and through the
calls that consume its batches.  Shapes (T, F): (4, 52) the simulator's minimum, without a burst; (24, 300) F crosses a
256-column workgroup seam and the ring halo with it; (12, 1300) more than 64 narrowband events; (650, 52) more than 64
bursts.  tests/test_inject_host.py checks on the CPU that no pixel of these seeds and shapes is ambiguous."""
import functools

import numpy as np
import pytest
import torch

from inject_ref import RefInjector, background, iqr_sigma

pytestmark = pytest.mark.gpu

SEED = 0x5EED_1234_ABCD
SHAPES = ((4, 52), (24, 300), (12, 1300), (650, 52))
N = 3                                       # samples 0, 1 draw three broadband chunks at this seed, sample 2 two
SIGMA = np.array([3.7e-3, 41.0, 0.6])


def _bytes(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))


def _sim(T, F, ring=False, seed=SEED):
    from rfi_toolbox_amd.core import RFISimulator
    sim = RFISimulator(T, F, seed=seed, device="cuda:0")
    sim.gibbs_ringing = ring
    return sim


def _turn(a, rows):
    """time-orientation planes (..., T, F) as the orientation `rows` stores"""
    return a if rows == "time" else np.ascontiguousarray(np.swapaxes(a, -1, -2))


def _flags(T, F, seed=1):
    return np.random.default_rng(seed).random((N, 4, T, F)) < 0.25


def _data(T, F):
    return background(N, T, F, seed=5) * SIGMA[:, None, None, None]


@functools.lru_cache(maxsize=None)
def _want(shape, ring, cross_hand):
    """the restatement of N samples in the time orientation (flags with "injected") -> per sample (planes, mask, touched,
    ambiguous, events, baseline_frac); computed once and shared, never modified"""
    T, F = shape
    ref = RefInjector(T, F, seed=SEED)
    ref.gibbs_ringing = ring
    data, flags = _data(T, F), _flags(T, F) if cross_hand == "injected" else None
    res = []
    for i in range(N):
        out, mask = ref.inject(data[i], None if flags is None else flags[i], scale=SIGMA[i], cross_hand=cross_hand)
        res.append((out, mask, ref.touched, ref.ambiguous, ref.events, ref.baseline_frac))
    return res


# ---------------------------------------------------------------- against the generating kernel, bit for bit
@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("shape", [(24, 300), (12, 1300)])
def test_unit_scale_reference_mode_on_clean_data_is_generate_batch(shape, ring):
    T, F = shape
    want = _sim(T, F, ring).generate_batch(N, out="complex128")
    sim = _sim(T, F, ring)
    clean = sim.generate_batch(N, clean=True, out="complex128")
    sim.sample_counter = 0
    got = sim.inject(clean.data, scale=1.0, cross_hand="reference")
    assert sim.sample_counter == N and got.rows == "time" and np.array_equal(got.noise_scale, np.ones(N))
    assert np.array_equal(_bytes(got.data.numpy()), _bytes(want.data.numpy()))
    assert np.array_equal(got.mask.numpy(), want.mask.numpy())
    assert np.array_equal(got.events.numpy(), want.events.numpy())
    assert np.array_equal(got.baseline_frac.numpy(), want.baseline_frac.numpy())
    assert got.origin[:4] == want.origin[:4]


# ---------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("rows", ["time", "channel"])
@pytest.mark.parametrize("cross_hand", ["injected", "reference"])
@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_device_matches_restatement(shape, ring, cross_hand, rows):
    T, F = shape
    data = _data(T, F)
    flags = _flags(T, F) if cross_hand == "injected" else None
    sim = _sim(T, F, ring)
    got = sim.inject(_turn(data, rows), None if flags is None else _turn(flags, rows), scale=SIGMA, rows=rows, cross_hand=cross_hand)
    planes, mask, ev, bl = got.data.numpy(), got.mask.numpy(), got.events.numpy(), got.baseline_frac.numpy()
    assert planes.shape == ((N, 4, T, F) if rows == "time" else (N, 4, F, T)) and mask.shape == planes.shape[:1] + planes.shape[2:]
    assert planes.dtype == np.complex128 and got.rows == rows and np.array_equal(got.noise_scale, SIGMA)
    kept = 0
    for i, (want, want_mask, touched, amb, want_ev, want_bl) in enumerate(_want(shape, ring, cross_hand)):
        for f in ("i0", "i1", "i2", "i3"):
            assert np.array_equal(ev[i][f], want_ev[f]), (i, f)
        assert bl[i] == want_bl
        want, want_mask, touched, amb = _turn(want, rows), _turn(want_mask, rows), _turn(touched, rows), _turn(amb, rows)
        for p in range(4):
            err = np.abs(planes[i, p] - want[p]).max()
            print(f"sample {i} pol {p}: max err {err:.3e}, max |want| {np.abs(want[p]).max():.3e}")
            assert err <= 1e-12 * np.abs(want[p]).max(), (i, p, err)
        assert int(amb.sum()) == 0
        assert np.array_equal(mask[i].astype(bool)[~amb], want_mask[~amb]), (i, int((mask[i].astype(bool) != want_mask).sum()))
        keep = ~touched if flags is None else (~touched | _turn(flags[i], rows))
        src = _turn(data[i], rows)
        assert np.array_equal(_bytes(planes[i])[keep], _bytes(src)[keep])
        kept += int(keep.sum())
        assert (_bytes(planes[i])[~keep] != _bytes(src)[~keep]).any()
    # with ringing the restatement itself leaves no visibility of some samples untouched (bursts spread +-8 rows, the cross
    # hands of "reference" take the whole RR), but in every case here at least one of the N samples keeps some
    assert kept > 0


# ---------------------------------------------------------------- complex64: the complex128 result rounded once
@pytest.mark.parametrize("rows", ["time", "channel"])
@pytest.mark.parametrize("ring", [False, True])
def test_complex64_is_the_rounded_complex128_result(ring, rows):
    T, F = 24, 300
    data = _turn(_data(T, F).astype(np.complex64), rows)
    raw = data.view(np.float32).reshape(N, 4, T * F, 2)
    raw[0, :, :6, 0] = np.array([0x80000000, 0x7FC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0xFFC00001], np.uint32).view(np.float32)
    flags = _turn(_flags(T, F), rows)
    a, b = _sim(T, F, ring), _sim(T, F, ring)
    got = a.inject(data, flags, scale=SIGMA, rows=rows)
    wide = b.inject(data.astype(np.complex128), flags, scale=SIGMA, rows=rows)
    z, w = got.data.numpy(), wide.data.numpy()
    assert z.dtype == np.complex64 and w.dtype == np.complex128
    same = (_bytes(w) == _bytes(data.astype(np.complex128))).all(axis=-1)      # stored as loaded in the wide run
    with np.errstate(invalid="ignore", over="ignore"):
        want = w.astype(np.complex64)
    changed = ~same & np.isfinite(want)                    # (a NaN's payload after two roundings is the converter's business)
    assert changed.any() and np.array_equal(_bytes(z)[changed], _bytes(want)[changed])
    assert np.isnan(z[~same & np.isnan(want)]).all()
    assert same[flags].all() and np.array_equal(_bytes(z)[same], _bytes(data)[same])     # as loaded: payloads, -0.0, signalling NaN
    assert np.array_equal(got.mask.numpy(), wide.mask.numpy())


# ---------------------------------------------------------------- scale="iqr"
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("rows", ["time", "channel"])
def test_iqr_scale_is_the_restatements(rows, dtype):
    T, F = 24, 300
    data = _data(T, F).astype(dtype)
    data[0, 1, 3, 5] = np.nan
    data[0, 2, 4, 7] = complex(1.0, np.inf)
    data[1, 0, 0, :9] = complex(-np.inf, 0.0)
    flags = _flags(T, F, seed=3)
    per_baseline = flags[:, 0]
    for fl in (None, flags, per_baseline):
        sim = _sim(T, F)
        got = sim.inject(_turn(data, rows), None if fl is None else _turn(fl, rows), scale="iqr", rows=rows)
        want = np.array([iqr_sigma(data[i], None if fl is None else fl[i]) for i in range(N)])
        assert got.noise_scale.dtype == np.float64 and np.array_equal(got.noise_scale, want), (got.noise_scale, want)
        assert np.all(np.abs(want / SIGMA - 1.5) < 1.0)            # (the scale follows the data's, sample by sample)
    dead = flags.copy()
    dead[1] = True
    sim = _sim(T, F)
    with pytest.raises(ValueError, match="sample 1"):
        sim.inject(_turn(data, rows), _turn(dead, rows), scale="iqr", rows=rows)
    assert sim.sample_counter == 0


# ---------------------------------------------------------------- bit reproducibility, chunks, in place, input kinds
@pytest.mark.parametrize("rows", ["time", "channel"])
@pytest.mark.parametrize("ring", [False, True])
def test_chunks_inplace_and_repeats_are_bit_identical(ring, rows):
    T, F = 24, 300
    data, flags = _turn(_data(T, F).astype(np.complex64), rows), _turn(_flags(T, F), rows)
    one = _sim(T, F, ring).inject(data, flags, scale=SIGMA, rows=rows)
    z, m, ev = one.data.numpy(), one.mask.numpy(), one.events.numpy()
    again = _sim(T, F, ring).inject(data, flags, scale=SIGMA, rows=rows)
    assert np.array_equal(_bytes(again.data.numpy()), _bytes(z)) and np.array_equal(again.mask.numpy(), m)
    sim = _sim(T, F, ring)
    c1 = sim.inject(data[:2], flags[:2], scale=SIGMA[:2], rows=rows)
    c2 = sim.inject(data[2:], flags[2:], scale=SIGMA[2:], rows=rows)
    assert sim.sample_counter == N and c2.origin.first_sample == 2
    assert np.array_equal(_bytes(np.concatenate([c1.data.numpy(), c2.data.numpy()])), _bytes(z))
    assert np.array_equal(np.concatenate([c1.mask.numpy(), c2.mask.numpy()]), m)
    assert np.array_equal(np.concatenate([c1.events.numpy(), c2.events.numpy()]), ev)
    # a DeviceArray: untouched by the copying call, written by the in-place one
    sim = _sim(T, F, ring)
    dev = sim._context().to_device(data)
    copy = sim.inject(dev, flags, scale=SIGMA, rows=rows)
    assert copy.data is not dev and np.array_equal(_bytes(dev.numpy()), _bytes(data)) and np.array_equal(_bytes(copy.data.numpy()), _bytes(z))
    sim.sample_counter = 0
    inp = sim.inject(dev, flags, scale=SIGMA, rows=rows, inplace=True)
    assert inp.data is dev and np.array_equal(_bytes(dev.numpy()), _bytes(z)) and np.array_equal(inp.mask.numpy(), m)
    # a GPU tensor, flags as a bool tensor: in place writes the tensor
    t, tf = torch.from_numpy(data).cuda(), torch.from_numpy(flags).cuda()
    sim = _sim(T, F, ring)
    r = sim.inject(t, tf, scale=SIGMA, rows=rows)
    assert np.array_equal(_bytes(t.cpu().numpy()), _bytes(data)) and np.array_equal(_bytes(r.data.numpy()), _bytes(z))
    sim.sample_counter = 0
    r = sim.inject(t, tf, scale=SIGMA, rows=rows, inplace=True)
    assert np.array_equal(_bytes(t.cpu().numpy()), _bytes(z)) and np.array_equal(_bytes(r.data.numpy()), _bytes(z))


# ---------------------------------------------------------------- downstream: family masks, instances
@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("shape", [(24, 300), (70, 130)])
def test_family_masks_and_instances_follow_the_injected_batch(shape, ring):
    from rfi_toolbox_amd.core import event_instances, event_table, family_masks
    T, F = shape
    gen = _sim(T, F, ring).generate_batch(N, out="complex64")
    want_bits = family_masks(gen).numpy()
    want_inst = event_instances(gen, max_instances=16)
    data = background(N, T, F, seed=2, dtype=np.complex64)
    for rows in ("time", "channel"):
        b = _sim(T, F, ring).inject(_turn(data, rows), scale=0.3, rows=rows)
        bits = family_masks(b).numpy()
        assert bits.shape == ((N, T, F) if rows == "time" else (N, F, T))
        assert np.array_equal(bits, _turn(want_bits, rows))
        assert np.array_equal(bits != 0, b.mask.numpy() != 0)
        assert np.array_equal(b.mask.numpy(), _turn(gen.mask.numpy(), rows))
        if rows == "time":
            inst = event_instances(b, max_instances=16)
            assert np.array_equal(inst.count_host, want_inst.count_host) and inst.count_host.min() > 0
            assert np.array_equal(inst.masks.numpy(), want_inst.masks.numpy())
            for f in ("boxes", "labels", "component"):
                x, y = getattr(inst, f).numpy(), getattr(want_inst, f).numpy()
                for i, c in enumerate(inst.count_host):
                    assert np.array_equal(x[i, :c], y[i, :c]), (f, i)
            for x, y in zip(event_table(b), event_table(gen)):
                assert np.array_equal(x.numpy(), y.numpy())
        else:
            with pytest.raises(ValueError, match="rows="):
                event_instances(b)
            with pytest.raises(ValueError, match="rows="):
                event_table(b)


# ---------------------------------------------------------------- error paths: before anything is allocated or launched
def test_value_errors_before_anything_is_allocated():
    T, F = 24, 300
    sim = _sim(T, F)
    good = np.zeros((2, 4, T, F), np.complex64)
    for kw in (dict(data=np.zeros((2, 4, T, F + 1), np.complex64)), dict(data=np.zeros((2, 4, F, T), np.complex64)),
               dict(data=good, rows="channel"), dict(data=np.zeros((2, 3, T, F), np.complex64)),
               dict(data=good, flags=np.zeros((2, 4, T, F), np.uint8), cross_hand="reference"),
               dict(data=good, scale=0.0), dict(data=good, scale=np.array([1.0, -2.0])), dict(data=good, scale=np.inf)):
        with pytest.raises(ValueError):
            sim.inject(**dict({"scale": 1.0}, **kw))
    with pytest.raises(TypeError):
        sim.inject(np.zeros((2, 4, T, F), np.float32), scale=1.0)               # real dtype
    with pytest.raises(TypeError):
        sim.inject(np.zeros((2, 8, T, F), np.float64), scale=1.0)
    assert sim._ctx is None and sim.sample_counter == 0
    small = _sim(3, 64)
    with pytest.raises(ValueError):
        small.inject(np.zeros((1, 4, 3, 64), np.complex64), scale=1.0)
    assert small._ctx is None
    empty = sim.inject(np.zeros((0, 4, T, F), np.complex64), scale=1.0)
    assert empty.data.shape == (0, 4, T, F) and empty.mask.shape == (0, T, F) and sim.sample_counter == 0
