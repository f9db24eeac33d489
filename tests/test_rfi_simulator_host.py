"""CPU-only: the NumPy restatement of the device RFISimulator (tests/rfisim_ref.py) against fixtures captured from the
reference (tests/golden/make_simulator_golden.py), and the argument checks of rfi_toolbox_amd.core.RFISimulator,
which must raise before any GPU context exists."""
import json
import os

import numpy as np
import pytest

from rfisim_ref import RefSimulator, aggregate, clean_stats, sample_stats, within_spread

# Bounds: a statistic's mean over this file's seeds must lie within K standard errors of the reference's mean, the
# standard error formed from the reference's spread across its 24 seeds (tests/golden/simulator_expected.json).
# K = 4 keeps a false alarm below 1e-4 per statistic for normal means; the 24-seed spread itself is uncertain by
# ~15 %, which K absorbs.
K = 4.0
N_SEEDS = 12


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "simulator_expected.json")) as f:
        return json.load(f)


def test_gibbs_kernel_bitwise(golden):
    from rfi_toolbox_amd.core import RFISimulator
    want = [float.fromhex(h) for h in golden["gibbs_kernel_hex"]]
    assert RefSimulator._make_gibbs_kernel().tolist() == want
    assert RFISimulator._make_gibbs_kernel().tolist() == want
    assert np.asarray(RFISimulator(8, 64, seed=0)._gibbs_kernel).tolist() == want


def test_phase_grid_bitwise(golden):
    from rfi_toolbox_amd.core import RFISimulator
    t, n = np.arange(7)[:, None], np.arange(5, 12)[None, :]
    for case in golden["phase_grid"]:
        want = [float.fromhex(h) for h in case["hex"]]
        assert RefSimulator._phase_grid(t, n, tuple(case["params"])).ravel().tolist() == want
        assert RFISimulator._phase_grid(t, n, tuple(case["params"])).ravel().tolist() == want


def test_reference_defaults():
    from rfi_toolbox_amd.core import RFISimulator
    s = RFISimulator(seed=3)
    assert (s.time_bins, s.freq_bins) == (1024, 1024)
    assert np.array_equal(s.power_range, np.logspace(-6, 4, num=100))
    assert (s.detect_floor, s.drift_prob, s.max_time_fringes, s.max_freq_fringes) == (1.0, 0.3, 30.0, 8.0)
    assert s.gibbs_ringing is False and s.baseline_frac == 0.5
    assert sorted(s.tf_plane) == ["LL", "LR", "RL", "RR"] and s.tf_plane["RR"].dtype == np.complex128
    assert s.mask.shape == (1024, 1024) and s.mask.dtype == bool and not s.mask.any()


@pytest.mark.parametrize("shape", [(256, 256), (128, 384)])
@pytest.mark.parametrize("ring", [False, True])
def test_restatement_statistics_within_reference_spread(golden, shape, ring):
    T, F = shape
    sim = RefSimulator(T, F, seed=77)
    sim.gibbs_ringing = ring
    per = []
    for _ in range(N_SEEDS):
        tf, mask = sim.generate_rfi()
        assert mask.dtype == bool and mask.any()
        assert not sim.ambiguous.any()
        per.append(sample_stats(sim.planes(), mask))
    bad = within_spread(aggregate(per), golden["stats"][f"{T}x{F}_ring{int(ring)}"], k=K)
    assert not bad, bad


@pytest.mark.parametrize("shape", [(256, 256), (128, 384)])
def test_restatement_clean_moments_within_reference_spread(golden, shape):
    T, F = shape
    sim = RefSimulator(T, F, seed=78)
    per = []
    for _ in range(N_SEEDS):
        tf, mask = sim.generate_clean_data()
        assert not mask.any()
        per.append(clean_stats(sim.planes()))
    bad = within_spread(aggregate(per), golden["stats"][f"{T}x{F}_clean"], k=K)
    assert not bad, bad


def test_restatement_sample_counter_and_events():
    a, b = RefSimulator(64, 64, seed=9), RefSimulator(64, 64, seed=9)
    a.generate_rfi()
    a.generate_rfi()
    b.sample_counter = 1
    b.generate_rfi()
    assert np.array_equal(a.planes(), b.planes()) and np.array_equal(a.mask, b.mask)
    assert np.array_equal(a.events, b.events)
    ev = a.events
    assert ev["i0"][0] in (2, 3) and ev["v0"][0] == a.baseline_frac
    assert len(ev) == 14 + int(64 * 0.05) + int(64 * 0.1)
    assert set(ev["i2"][-5:].tolist()) <= {-1, 1}                      # quadratic sweep directions


def test_argument_validation_without_gpu():
    """The reference raises on these sizes (randint bounds); so does the simulator, before any context exists."""
    from rfi_toolbox_amd.core import RFISimulator
    for T, F in ((3, 64), (64, 51)):
        sim = RFISimulator(T, F, seed=0)
        with pytest.raises(ValueError):
            sim.generate_rfi()
        with pytest.raises(ValueError):
            sim.generate_batch(2)
        assert sim._ctx is None and sim.sample_counter == 0
    sim = RFISimulator(64, 64, seed=0)
    sim.power_range = np.ones(1025)
    with pytest.raises(ValueError):
        sim.generate_rfi()
    sim.power_range = np.array([])
    with pytest.raises(ValueError):
        sim.generate_batch(1)
    with pytest.raises(ValueError):
        RFISimulator(64, 64, seed=0).generate_batch(1, out="bogus")
    with pytest.raises(ValueError):
        RFISimulator(0, 64)
    assert sim._ctx is None
