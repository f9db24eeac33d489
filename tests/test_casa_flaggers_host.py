"""CPU-only checks of the CASA-style baseline flaggers: the NumPy oracle (tests/casa_flaggers_ref.py) against hand-worked
answers and against direct restatements of its definitions, chunking, the flagging quality on synthetic waterfalls and
the argument checks of the public interface.  The device kernels are compared with the same oracle in
tests/test_gpu_casa_flaggers.py."""
import numpy as np
import pytest

import casa_flaggers_ref as ref
from oracle import synth_ref
from rfi_toolbox_amd import flagging
from test_sumthreshold_host import EVENTS


# ---------------------------------------------------------------------------------------------- the robust fit
def test_fit_returns_an_exact_line_and_an_exact_cubic():
    # 12 samples: no residual can lie further than sqrt(11) = 3.3 standard deviations from the mean, so a cutoff of 4
    # rejects nothing whatever the rounding does
    i = np.arange(12, dtype=np.float64)
    line = (2.0 + 0.5 * i).astype(np.float32)
    new, fit, res, _ = ref.robust_fit(line[None], np.ones((1, 12), bool), "line", 4.0, details=True)
    assert not new.any() and np.abs(res).max() < 1e-13 and np.allclose(fit[0], line, rtol=0, atol=1e-13)
    x = (2 * i - 11) / 11
    cubic = (1.0 + x - 0.5 * x * x + 0.25 * x ** 3).astype(np.float32)
    new, fit, res, _ = ref.robust_fit(cubic[None], np.ones((1, 12), bool), "poly", 4.0, maxnpieces=1, details=True)
    assert not new.any() and np.abs(res).max() < 1e-6 and np.allclose(fit[0], cubic, rtol=0, atol=1e-6)       # float32 samples
    exact = ref.fit_pieces((x ** 3)[None].astype(np.float32), np.ones((1, 12), bool), 1, 3)
    assert np.abs(exact[0] - (x ** 3).astype(np.float32)).max() < 1e-7
    # three pieces of four samples: a cubic through every four points
    new, fit, res, _ = ref.robust_fit(cubic[None], np.ones((1, 12), bool), "poly", 4.0, maxnpieces=3, details=True)
    assert not new.any() and np.abs(res).max() < 1e-12


def test_fit_rejects_one_spike_and_refits_without_it():
    i = np.arange(20, dtype=np.float64)
    y = (1.0 + 0.25 * i).astype(np.float32)
    y[5] += 100.0
    new, fit, res, sig = ref.robust_fit(y[None], np.ones((1, 20), bool), "line", 4.0, details=True)
    assert np.flatnonzero(new[0]).tolist() == [5]
    assert sig[0, 0] > 20.0                                       # the spike dominates the first sigma: 100 sqrt(19) / 20
    clean = 1.0 + 0.25 * i
    assert np.allclose(fit[0], clean, rtol=0, atol=1e-12)         # the refit ignores it
    assert abs(res[0, 5] - 100.0) < 1e-12
    # a prior flag is not a new flag, and the masked sample does not pull the fit
    u = np.ones((1, 20), bool)
    u[0, 5] = False
    new, fit, _, _ = ref.robust_fit(y[None], u, "line", 4.0, details=True)
    assert not new.any() and np.allclose(fit[0], clean, rtol=0, atol=1e-12)


def test_fit_degree_falls_back_with_the_valid_samples():
    y = np.array([[3.0, 1.0, 4.0, 1.0, 5.0, 9.0, 2.0, 6.0]], np.float32)
    x = (2 * np.arange(8) - 7) / 7.0

    def run(valid):
        w = np.zeros((1, 8), bool)
        w[0, valid] = True
        return ref.fit_pieces(y, w, 1, 3)[0]

    assert (run([]) == 0.0).all()                                               # no sample: the fit is 0
    assert (run([4]) == 5.0).all()                                              # one: the constant
    two = run([1, 5])
    assert np.allclose(two, 1.0 + (x - x[1]) * 8.0 / (x[5] - x[1]), rtol=0, atol=1e-12)      # two: the line through them
    three = run([0, 3, 6])
    assert np.allclose(three, np.polyval(np.polyfit(x[[0, 3, 6]], [3.0, 1.0, 2.0], 2), x), rtol=0, atol=1e-10)
    four = run([0, 2, 4, 7])
    assert np.allclose(four[[0, 2, 4, 7]], [3.0, 4.0, 5.0, 6.0], rtol=0, atol=1e-10)
    # pieces: L = 5 cut in 7 gives two empty pieces, every sample its own constant
    assert ref.piece_bounds(5, 7) == [(0, 0), (0, 1), (1, 2), (2, 2), (2, 3), (3, 4), (4, 5)]
    assert np.array_equal(ref.fit_pieces(y[:, :5], np.ones((1, 5), bool), 7, 3)[0], y[0, :5].astype(np.float64))
    assert ref.piece_bounds(10, 3) == [(0, 3), (3, 6), (6, 10)]


def test_fit_sums_sequentially():
    # B_0 = ((1 + e) + e) + e in float64 with e = 2^-53 is 1, the balanced tree (1 + e) + (e + e) is 1 + 2^-52: the mean of the
    # four samples (degree 0) tells the pinned order from the other
    e = 2.0 ** -53
    tree, chain = (1.0 + e) + (e + e), ((1.0 + e) + e) + e
    assert tree > 1.0 and chain == 1.0
    y = np.array([[1.0, e, e, e]], np.float32)
    assert y[0, 1] == e
    fit = ref.fit_pieces(y, np.ones((1, 4), bool), 1, 0)
    assert (fit == chain / 4.0).all() and (fit != tree / 4.0).all()


def test_fit_leaves_constant_and_empty_lines_alone():
    y = np.full((2, 9), 2.5, np.float32)
    u = np.ones((2, 9), bool)
    u[1] = False
    new, _, _, sig = ref.robust_fit(y, u, "poly", 3.0, details=True)
    assert not new.any() and (sig[0] == 0).all()


# ---------------------------------------------------------------------------------------------- RFlag
def test_rflag_window_rms_by_hand():
    re = np.array([1.0, 3.0, 1.0, 3.0, 11.0])
    z = (re + 2j * re)[None]
    rms, has = ref.window_rms(z, np.ones((1, 5), bool), 3)
    # windows {1,3} {1,3,1} {3,1,3} {1,3,11} {3,11}: population variances 1, 8/9, 8/9, 56/3, 16, times 1 + 2^2 for both parts
    want = np.sqrt(5.0 * np.array([1.0, 8 / 9, 8 / 9, 56 / 3, 16.0]))
    assert has.all() and np.allclose(rms[0], want, rtol=1e-14, atol=0)
    # a flagged sample leaves its windows: {3} alone has no value, {3, 3} has rms 0
    u = np.array([[False, True, False, True, True]])
    rms, has = ref.window_rms(z, u, 3)
    assert has[0].tolist() == [False, False, True, True, True]
    assert rms[0, 2] == 0.0 and np.isclose(rms[0, 4], np.sqrt(5.0 * 16.0), rtol=1e-14)
    # winsize 1: a window of one sample never has a value
    assert not ref.window_rms(z, np.ones((1, 5), bool), 1)[1].any()


def test_rflag_single_sample_windows_flag_nothing():
    z = np.array([[1.0 + 1j, 500.0 - 3j, 2.0 + 0j]])
    F = np.array([[False, True, True]])
    out = ref.rflag_chunk(z, F)
    assert np.array_equal(out, F)
    assert np.array_equal(ref.rflag_plane(np.array([[7.0 + 1j]])), [[False]])


def test_rflag_overrides_equal_the_computed_thresholds():
    rng = np.random.default_rng(3)
    z = rng.standard_normal((12, 40)) + 1j * rng.standard_normal((12, 40))
    z[4, 10:14] *= 30.0
    z[:, 25] += 8.0 * np.exp(1j * np.arange(12))
    F = rng.random((12, 40)) < 0.05
    out, rms, has, base_t, base_f = ref.rflag_chunk(z, F, details=True)
    assert (out & ~F).any() and not out.all()
    assert base_t.shape == (12,) and np.array_equal(base_t[0], ref.med_plus_mad(rms[0][has[0]]))
    v = rms[0][has[0]]
    assert ref.med_plus_mad(v) == np.median(v) + np.median(np.abs(v - np.median(v)))
    assert np.array_equal(ref.rflag_chunk(z, F, timedev=base_t, freqdev=base_f), out)
    assert not np.array_equal(ref.rflag_chunk(z, F, timedev=base_t * 0.5, freqdev=base_f), out)
    assert not np.array_equal(ref.rflag_chunk(z, F, timedev=base_t, freqdev=base_f * 0.5), out)
    # through the stack interface: a scalar, one per plane, one per (plane, channel)
    stack = np.stack([z, 2.0 * z])
    a = ref.rflag(stack, timedev=np.stack([base_t, 2.0 * base_t]), freqdev=[base_f, 2.0 * base_f])
    assert np.array_equal(a[0], ref.rflag_chunk(z, np.zeros_like(F), timedev=base_t, freqdev=base_f))
    assert np.array_equal(a[0], a[1])                                          # the same plane at twice the scale
    assert np.array_equal(ref.rflag(stack, timedev=1.0, freqdev=2.0)[0], ref.rflag_chunk(z, np.zeros_like(F), timedev=np.full(12, 1.0), freqdev=2.0))


# ---------------------------------------------------------------------------------------------- extend
def _extend_direct(F, ntime, growtime, growfreq, growaround, flagneartime, flagnearfreq):
    """Sample by sample, straight from the definition."""
    F = np.asarray(F).astype(bool)
    C, T = F.shape
    out = np.zeros_like(F)
    for t0 in range(0, T, ntime or T):
        cur = F[:, t0:t0 + (ntime or T)].copy()
        L = cur.shape[1]
        inside = lambda c, t: 0 <= c < C and 0 <= t < L
        if growaround:
            nxt = cur.copy()
            for c in range(C):
                for t in range(L):
                    nb = sum(cur[c + dc, t + dt] for dc in (-1, 0, 1) for dt in (-1, 0, 1) if (dc or dt) and inside(c + dc, t + dt))
                    nxt[c, t] |= nb > 4
            cur = nxt
        nxt = cur.copy()
        for c in range(C):
            if float(100 * int(cur[c].sum())) > growtime * float(L):
                nxt[c] = True
        cur = nxt
        nxt = cur.copy()
        for t in range(L):
            if float(100 * int(cur[:, t].sum())) > growfreq * float(C):
                nxt[:, t] = True
        cur = nxt
        for on, dc, dt in ((flagneartime, 0, 1), (flagnearfreq, 1, 0)):
            if on:
                nxt = cur.copy()
                for c in range(C):
                    for t in range(L):
                        nxt[c, t] |= any(cur[c + s * dc, t + s * dt] for s in (-1, 1) if inside(c + s * dc, t + s * dt))
                cur = nxt
        out[:, t0:t0 + L] = cur
    return out


@pytest.mark.parametrize("density", [0.0, 0.1, 0.5, 0.9, 1.0])
def test_extend_equals_a_direct_restatement(density):
    rng = np.random.default_rng(int(density * 10))
    F = rng.random((9, 14)) < density
    options = [dict(), dict(growaround=True), dict(flagneartime=True), dict(flagnearfreq=True), dict(growtime=100.0, growfreq=100.0),
               dict(growtime=30.0, growfreq=100.0), dict(growtime=100.0, growfreq=30.0),
               dict(growtime=40.0, growfreq=60.0, growaround=True, flagneartime=True, flagnearfreq=True)]
    for kw in options:
        full = dict(growtime=50.0, growfreq=50.0, growaround=False, flagneartime=False, flagnearfreq=False)
        full.update(kw)
        for ntime in (None, 5):
            assert np.array_equal(ref.extend(F, ntime=ntime, **kw), _extend_direct(F, ntime, **full)), (kw, ntime)
    assert np.array_equal(ref.extend(F, growtime=100.0, growfreq=100.0), F)
    assert np.array_equal(ref.extend(F.astype(np.uint8) * 3, growtime=100.0, growfreq=100.0), F)


def test_extend_thresholds_are_strict():
    F = np.zeros((4, 8), bool)
    F[1, :4] = True                                      # exactly 50 per cent of the channel: not grown
    F[2, :5] = True                                      # more: grown
    out = ref.extend(F, growfreq=100.0)
    assert np.array_equal(out[1], F[1]) and out[2].all() and not out[0].any()
    G = np.zeros((4, 8), bool)
    G[:2, 3] = True                                      # exactly half of the four channels at t = 3
    G[:3, 5] = True
    out = ref.extend(G, growtime=100.0)
    assert np.array_equal(out[:, 3], G[:, 3]) and out[:, 5].all()
    H = np.zeros((3, 3), bool)
    H[0, :] = True
    H[1, 0] = True                                       # the centre has 4 flagged neighbours
    assert not ref.extend(H, growtime=100.0, growfreq=100.0, growaround=True)[1, 1]
    H[1, 2] = True                                       # now 5
    assert ref.extend(H, growtime=100.0, growfreq=100.0, growaround=True)[1, 1]
    # neighbours outside the chunk count as unflagged: the same mask cut after the first time sample
    assert not ref.extend(H, ntime=1, growtime=100.0, growfreq=100.0, growaround=True)[1, 1]
    assert ref.extend(np.eye(3, dtype=bool), growtime=100.0, growfreq=100.0, flagneartime=True).sum() == 7


# ---------------------------------------------------------------------------------------------- chunking
def test_ntime_chunking_equals_the_slices():
    assert ref._chunks(10, 4) == [(0, 4), (4, 8), (8, 10)] and ref._chunks(10, None) == [(0, 10)] and ref._chunks(3, 7) == [(0, 3)]
    rng = np.random.default_rng(10)
    z = (1.0 + 0.1 * rng.standard_normal((16, 10))) * np.exp(2j * np.pi * rng.random((16, 10)))
    z[5, :] *= 6.0
    z[:, 6] *= 4.0
    prior = rng.random((16, 10)) < 0.05
    slices = [slice(0, 4), slice(4, 8), slice(8, 10)]
    assert np.array_equal(ref.tfcrop_plane(z, prior, ntime=4),
                          np.concatenate([ref.tfcrop_plane(z[:, s], prior[:, s]) for s in slices], axis=1))
    low = dict(timedevscale=2.0, freqdevscale=2.0)
    assert np.array_equal(ref.rflag_plane(z, prior, ntime=4, **low),
                          np.concatenate([ref.rflag_plane(z[:, s], prior[:, s], **low) for s in slices], axis=1))
    assert np.array_equal(ref.extend_plane(prior, ntime=4, growaround=True, flagneartime=True),
                          np.concatenate([ref.extend_plane(prior[:, s], growaround=True, flagneartime=True) for s in slices], axis=1))
    assert not np.array_equal(ref.tfcrop_plane(z, prior, ntime=4), ref.tfcrop_plane(z, prior))
    assert not np.array_equal(ref.rflag_plane(z, prior, ntime=4, **low), ref.rflag_plane(z, prior, **low))


# ---------------------------------------------------------------------------------------------- the algorithms themselves
@pytest.fixture(scope="module")
def synthetic():
    planes, truth = synth_ref.generate(7, EVENTS, 2, 96, 160, noise=0.1, use_bandpass=False)
    strong = np.zeros((3, 96, 160), bool)                # the pixels of the events of at least 10 times the noise
    for s in range(3):
        for ev in EVENTS[s]:
            if ev[5] >= 10 * 0.1:
                strong[s] |= synth_ref.rasterise([ev], 96, 160)[1]
    return planes, truth.astype(bool), strong


@pytest.mark.parametrize("name", ["tfcrop", "rflag"])
def test_oracle_finds_the_synthetic_rfi(synthetic, name):
    planes, truth, strong = synthetic
    base = getattr(ref, name)(planes)
    for label, flags in ((name, base), (name + " + extend", ref.extend(base))):
        assert flags.shape == planes.shape and flags.dtype == bool
        for s in range(2):
            for p in range(2):
                t, f = truth[s, p], flags[s, p]
                recall, false_rate = (f & strong[s]).sum() / strong[s].sum(), (f & ~t).sum() / (~t).sum()
                print(f"{label}: sample {s} pol {p}: recall {recall:.4f} false-flag rate {false_rate:.4f}")
                assert recall >= 0.9
                assert false_rate <= 0.10
        assert not truth[2].any()
        print(f"{label}: empty sample: {flags[2].mean():.5f} flagged")
        assert flags[2].mean() <= 0.01


def stage_plane():
    """(64, 96) complex128: a curved bandpass, one bright channel, one bright time sample, a short burst."""
    rng = np.random.default_rng(11)
    C, T = 64, 96
    c = np.arange(C)[:, None] / C
    amp = (1.0 + 2.0 * np.sin(3.0 * np.pi * c) ** 2 + c) * (1.0 + 0.05 * rng.standard_normal((C, T)))
    amp[17, :] += 3.0
    amp[:, 70] += 1.5
    amp[40, 20:28] += 1.0
    return amp * np.exp(2j * np.pi * rng.random((C, T)))


def rflag_plane():
    """(64, 96) complex128 around 1 + 0j: a noisy burst in one channel, a few channels off the spectrum at one time
    sample, and one channel with a steady offset (which only the spectral analysis can see)."""
    rng = np.random.default_rng(12)
    z = 1.0 + 0.05 * (rng.standard_normal((64, 96)) + 1j * rng.standard_normal((64, 96)))
    z[40, 20:28] += 2.0 * (rng.standard_normal(8) + 1j * rng.standard_normal(8))
    z[10:14, 70] += 3.0
    z[25, :] += 2.0
    return z


def test_every_stage_changes_the_answer():
    """A plane on which the defaults differ from the same run without the bandpass division, without the frequency stage,
    with a single cubic piece, and (RFlag) without the spectral analysis: a device pipeline that drops one cannot equal the
    oracle on it."""
    z = stage_plane()
    full = ref.tfcrop_plane(z)
    assert full[17].all() and full[:, 70].all() and full[40, 20:28].all() and full.mean() < 0.2
    for kw in (dict(divide=False), dict(flagdimension="time"), dict(maxnpieces=1), dict(flagdimension="freq"), dict(ntime=32)):
        assert not np.array_equal(full, ref.tfcrop_plane(z, **kw)), kw
    z = rflag_plane()
    rf = ref.rflag_plane(z)
    assert rf[40, 21:27].all() and rf[10:14, 70].all() and rf[25].all() and rf.mean() < 0.2
    assert not np.array_equal(rf, ref.rflag_plane(z, freqdev=1e30))
    assert not np.array_equal(rf, ref.rflag_plane(z, timedev=1e30))
    assert not np.array_equal(rf, ref.rflag_plane(z, winsize=5))


# ---------------------------------------------------------------------------------------------- argument checks, no GPU
def test_bad_arguments_raise_before_any_device_call():
    z = np.zeros((2, 8, 8), np.complex64)
    common = [dict(ntime=0), dict(ntime=-3), dict(ntime=2.5), dict(flags=np.zeros((2, 8, 7), bool)),
              dict(flags=np.zeros((2, 8, 8), np.float32)), dict(out="gpu")]
    for kw in common + [dict(timefit="cubic"), dict(freqfit="spline"), dict(flagdimension="both"), dict(maxnpieces=0),
                        dict(maxnpieces=-1), dict(timecutoff=-1.0), dict(freqcutoff=-0.5), dict(timecutoff=float("nan"))]:
        with pytest.raises(ValueError):
            flagging.tfcrop_flags(z, **kw)
    for kw in common + [dict(winsize=2), dict(winsize=0), dict(winsize=-1), dict(timedevscale=-1.0), dict(freqdevscale=-1.0),
                        dict(timedev=np.ones(3)), dict(freqdev=np.ones((2, 8)))]:
        with pytest.raises(ValueError):
            flagging.rflag_flags(z, **kw)
    for real in (np.zeros((8, 8), np.float32), np.zeros((8, 8), np.float64)):
        with pytest.raises(ValueError):
            flagging.rflag_flags(real)
    f = np.zeros((2, 8, 8), bool)
    for kw in (dict(ntime=0), dict(growtime=-1.0), dict(growtime=100.5), dict(growfreq=-0.1), dict(growfreq=101.0), dict(out="gpu"),
               dict(growtime=float("nan"))):
        with pytest.raises(ValueError):
            flagging.extend_flags(f, **kw)
    for bad in (np.zeros((2, 8, 8), np.float32), np.zeros(8, bool)):
        with pytest.raises(ValueError):
            flagging.extend_flags(bad)
    for fn in (flagging.tfcrop_flags, flagging.rflag_flags):
        for data in (np.zeros(8, np.complex64), np.zeros((4, 4), np.int32)):
            with pytest.raises(ValueError):
                fn(data)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.complex64), shape=(1, (1 << 20) + 1), strides=(0, 0))
    for fn in (flagging.tfcrop_flags, flagging.rflag_flags):
        with pytest.raises(ValueError):
            fn(big)
