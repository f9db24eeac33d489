"""CPU-only checks of the SumThreshold baseline flagger: the NumPy oracle (tests/sumthreshold_ref.py) against
hand-worked answers and against the definitions it abbreviates, the host-only ladder entry point against the oracle's
ladder bit for bit, the argument checks of the public interface, and the algorithm's flagging quality on synthetic
waterfalls.  The device kernels are compared with the same oracle in tests/test_gpu_sumthreshold.py."""
import numpy as np
import pytest

import sumthreshold_ref as ref
from oracle import synth_ref
from rfi_toolbox_amd import flagging


# ---------------------------------------------------------------------------------------------- pass: hand-worked
def test_pass_single_spike_window_one():
    v = np.zeros((1, 9), np.float32)
    v[0, 4] = 5.0
    out = ref.sumthreshold_pass(v, np.zeros_like(v, bool), 1, threshold=4.0)
    assert out.tolist() == [[False] * 4 + [True] + [False] * 4]
    # the threshold is strict, and the centre is subtracted first
    assert not ref.sumthreshold_pass(v, np.zeros_like(v, bool), 1, threshold=5.0).any()
    assert not ref.sumthreshold_pass(v, np.zeros_like(v, bool), 1, threshold=4.0, center=1.5)[0, 4]
    # along the other axis the same line gives the same answer
    assert ref.sumthreshold_pass(v.T, np.zeros_like(v.T, bool), 1, 4.0, axis=0).T.tolist() == out.tolist()


def _run_levels(v, levels, chi_1=1.0, rho=1.5):
    f = np.zeros_like(v, bool)
    for k in range(levels):
        f = ref.sumthreshold_pass(v, f, 1 << k, chi_1 / rho ** k)
    return f


def test_pass_faint_run_needs_the_longer_window():
    # four samples of 0.5: each below chi_0 = 1, a pair sums to 1 < 2 chi_1 = 1.33, three to 1.5 < 4 chi_2 = 1.78 (so a window
    # that holds only three of them stays quiet) and the four to 2 > 1.78
    v = np.zeros((1, 16), np.float32)
    v[0, 6:10] = 0.5
    assert not _run_levels(v, 1).any()
    assert not _run_levels(v, 2).any()
    assert _run_levels(v, 3).tolist() == [[False] * 6 + [True] * 4 + [False] * 6]


def test_pass_flagged_sample_lowers_the_count():
    # window of 4 over (1, 1, X, 1) with X flagged: the sum is 3 over n = 3 samples; with chi = 0.9 it hits (3 > 2.7)
    # although the same sum over four counted samples would not (3 < 3.6); all four samples of the window are flagged
    v = np.array([[1.0, 1.0, 100.0, 1.0]], np.float32)
    f = np.array([[False, False, True, False]])
    assert ref.sumthreshold_pass(v, f, 4, 0.9).all()
    assert ref.sumthreshold_pass(v, f, 4, 1.0).tolist() == f.tolist()          # 3 > 3 is false
    # a window with nothing unflagged never hits, whatever the threshold
    assert ref.sumthreshold_pass(v, np.ones_like(f), 4, -1.0).all()
    assert not ref.sumthreshold_pass(np.zeros((1, 4), np.float32), f, 4, 0.0)[0, 0]      # 0 > 0 is false


def test_pass_window_longer_than_the_line_is_a_no_op():
    v = np.full((2, 3), 9.0, np.float32)
    f = np.zeros((2, 3), bool)
    assert not ref.sumthreshold_pass(v, f, 4, 0.1, axis=1).any()
    assert ref.sumthreshold_pass(v, f, 2, 0.1, axis=0).all()


def test_pass_sums_in_a_balanced_tree():
    # (a + b) + (c + d) in float64, not a running sum: 1, e, e, e with e = 2^-53 (all exact in float32) give
    # (1 + e) + (e + e) = 1 + 2^-52 as a tree and ((1 + e) + e) + e = 1 as a chain; 4 chi = 1 tells them apart
    e = 2.0 ** -53
    tree, chain = (1.0 + e) + (e + e), ((1.0 + e) + e) + e
    assert tree > 1.0 and chain == 1.0
    v = np.array([[1.0, e, e, e]], np.float32)
    assert v[0, 1] == e
    assert ref.sumthreshold_pass(v, np.zeros((1, 4), bool), 4, 0.25).all()


# ---------------------------------------------------------------------------------------------- SIR
@pytest.mark.parametrize("eta", [0.0, 0.2, 0.5, 0.73])
def test_sir_equals_its_definition(eta):
    rng = np.random.default_rng(int(eta * 100))
    for L in (1, 2, 7, 33, 64):
        for density in (0.0, 0.1, 0.5, 0.9, 1.0):
            line = rng.random(L) < density
            assert np.array_equal(ref.sir_operator(line[None, :], eta)[0], ref.sir_definition(line, eta)), (L, density)
            assert np.array_equal(ref.sir_operator(line[:, None], eta, axis=0)[:, 0], ref.sir_definition(line, eta))


def test_sir_keeps_prior_flags_and_extends_them():
    line = np.zeros(20, bool)
    line[5:10] = True
    out = ref.sir_operator(line[None], 0.2)[0]
    # q = 205: five flagged of six give 5120 >= 819 * 6 = 4914 on either side, five of seven 5120 < 5733
    assert np.flatnonzero(out).tolist() == [4, 5, 6, 7, 8, 9, 10]
    assert np.array_equal(ref.sir_operator(line[None], 0.0)[0], line)


# ---------------------------------------------------------------------------------------------- ladder through ctypes
@pytest.mark.parametrize("rho", [1.5, 1.3])
def test_ladder_entry_point_equals_the_oracle_bit_for_bit(rho):
    rng = np.random.default_rng(5)
    for sigma in [1.0, 0.1234567, *rng.lognormal(0, 3, 5)]:
        for levels in (1, 7, 8):
            for it in range(3):
                got = flagging.threshold_ladder(sigma, it, iterations=3, levels=levels, rho=rho, chi_1=6.0, base_sensitivity=0.7)
                want = ref.ladder(sigma, it, iterations=3, levels=levels, rho=rho, chi_1=6.0, base_sensitivity=0.7)
                assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (sigma, levels, it)
    # the sensitivity halves per iteration down to base_sensitivity, the levels fall by rho
    last = flagging.threshold_ladder(2.0, 2, iterations=3, levels=3, rho=rho)
    assert last[0] == 12.0 and flagging.threshold_ladder(2.0, 0, iterations=3, levels=3, rho=rho)[0] == 48.0
    assert last[1] == 12.0 / rho


def test_gaussian_weights():
    w = flagging.gaussian_weights(2.5, 10)
    assert w.dtype == np.float64 and w.shape == (21,) and w[10] == 1.0 and np.array_equal(w, w[::-1])
    assert np.array_equal(w, np.exp(-np.arange(-10, 11) ** 2 / (2 * 2.5 * 2.5)))
    assert flagging.gaussian_weights(1.0, 0).tolist() == [1.0]


# ---------------------------------------------------------------------------------------------- argument checks, no GPU
def test_bad_arguments_raise_before_any_device_call():
    x = np.zeros((2, 8, 8), np.complex64)
    bad = [dict(iterations=0), dict(levels=0), dict(levels=9), dict(rho=1.0), dict(rho=0.5), dict(smooth_sigma=(0.0, 1.0)),
           dict(smooth_sigma=(1.0, -1.0)), dict(smooth_half=(-1, 3)), dict(smooth_half=(3, -1)), dict(sir_eta=1.0),
           dict(sir_eta=-0.1), dict(flags=np.zeros((2, 8, 7), bool)), dict(flags=np.zeros((2, 8, 8), np.float32)),
           dict(out="gpu")]
    for kw in bad:
        with pytest.raises(ValueError):
            flagging.sumthreshold_flags(x, **kw)
    for data in (np.zeros(8, np.float32), np.zeros((4, 4), np.int32), np.zeros((4, 4), np.float16)):
        with pytest.raises(ValueError):
            flagging.sumthreshold_flags(data)

    for shape in ((1, (1 << 20) + 1), ((1 << 20) + 1, 1)):          # (a view of one element: nothing that size is allocated)
        big = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), shape=shape, strides=(0, 0))
        with pytest.raises(ValueError):
            flagging.sumthreshold_flags(big)
    f = np.zeros((4, 4), bool)
    v = np.zeros((4, 4), np.float32)
    for kw in (dict(window=3), dict(window=0), dict(window=256), dict(window=2, axis=0 - 3)):
        with pytest.raises(ValueError):
            flagging.sumthreshold_pass(v, f, **{"window": 2, "threshold": 1.0, **kw})
    with pytest.raises(ValueError):
        flagging.sumthreshold_pass(v.astype(np.complex64), f, 2, 1.0)
    with pytest.raises(ValueError):
        flagging.sumthreshold_pass(v, f[:3], 2, 1.0)
    with pytest.raises(ValueError):
        flagging.masked_gaussian_smooth(v, f, np.ones(4), np.ones(3))
    with pytest.raises(ValueError):
        flagging.sir_operator(f, 1.0)
    with pytest.raises(ValueError):
        flagging.sir_operator(np.zeros(4, bool), 0.2)


# ---------------------------------------------------------------------------------------------- the algorithm itself
EVENTS = [[(0, 20, 21, 0, 160, 5.0), (0, 0, 96, 40, 42, 3.0), (0, 60, 61, 30, 94, 0.15), (1, 10, 80, 4, 1, 2.0)],
          [(0, 5, 7, 0, 160, 1.0), (0, 50, 51, 100, 108, 0.8)],
          []]


@pytest.fixture(scope="module")
def synthetic():
    planes, truth = synth_ref.generate(7, EVENTS, 2, 96, 160, noise=0.1, use_bandpass=False)
    return planes, truth.astype(bool), ref.flag(planes)


def test_oracle_finds_the_synthetic_rfi(synthetic):
    planes, truth, flags = synthetic
    assert flags.shape == planes.shape and flags.dtype == bool
    for s in range(2):
        for p in range(2):
            t, f = truth[s, p], flags[s, p]
            recall, false_rate = (f & t).sum() / t.sum(), (f & ~t).sum() / (~t).sum()
            print(f"sample {s} pol {p}: recall {recall:.4f} false-flag rate {false_rate:.4f}")
            assert recall >= 0.99
            assert false_rate <= 0.10
    assert not truth[2].any()
    print(f"empty sample: {flags[2].mean():.5f} flagged")
    assert flags[2].mean() <= 0.005


def test_every_stage_changes_the_answer():
    """A plane on which the defaults differ from the same run without the background fit (iterations=1), without SIR
    and without the longer windows: a device pipeline that drops a stage cannot equal the oracle on it."""
    rng = np.random.default_rng(11)
    C, T = 64, 96
    x = (1.0 + 0.5 * np.arange(C)[:, None] / C) * (1.0 + 0.05 * rng.standard_normal((C, T)))      # gain slope across the channels
    x[17, :] += 3.0                     # one bright channel
    x[:, 70] += 3.0                     # one bright time
    x[40, 20:52] += 0.12                # one faint 32-sample line
    x = x.astype(np.float32)
    full = ref.flag_plane(x)
    assert full[17].all() and full[:, 70].all() and full[40, 20:52].mean() > 0.9
    for kw in (dict(iterations=1), dict(sir_eta=0.0), dict(levels=1)):
        other = ref.flag_plane(x, **kw)
        assert not np.array_equal(full, other), kw
