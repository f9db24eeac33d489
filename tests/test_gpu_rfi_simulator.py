"""rfi_toolbox_amd.core.RFISimulator on the GPU (csrc/rfi_sim.hip) against the NumPy restatement tests/rfisim_ref.py,
which draws the same Philox words and follows the reference line by line, and against the distribution statistics
captured from the reference (tests/golden/simulator_expected.json)."""
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from rfisim_ref import (RefSimulator, aggregate, clean_stats, sample_stats, within_spread)

pytestmark = pytest.mark.gpu

SEED = 0x5EED_1234_ABCD


def _pair(T, F, ring, seed=SEED, **attrs):
    from rfi_toolbox_amd.core import RFISimulator
    dev, ref = RFISimulator(T, F, seed=seed, device="cuda:0"), RefSimulator(T, F, seed=seed)
    for s in (dev, ref):
        s.gibbs_ringing = ring
        for k, v in attrs.items():
            setattr(s, k, v)
    return dev, ref


def _compare(batch, ref, n, baseline_frac=None):
    """device SimBatch (complex128) against n restatement samples -> the restatement's event tables"""
    planes, mask, ev = batch.data.numpy(), batch.mask.numpy(), batch.events.numpy()
    bl = batch.baseline_frac.numpy()
    tables = []
    for i in range(n):
        ref.generate_rfi(baseline_frac)
        want_ev = ref.events
        for f in ("i0", "i1", "i2", "i3"):
            assert np.array_equal(ev[i][f], want_ev[f]), (i, f, ev[i][f], want_ev[f])
        for f in ("s0", "sdot", "r0", "phi0", "v0", "v1"):
            a, b = ev[i][f], want_ev[f]
            assert np.all(np.abs(a - b) <= 4 * np.spacing(np.abs(b))), (i, f)
        assert bl[i] == ref.baseline_frac
        want = ref.planes()
        for p in range(4):
            err = np.abs(planes[i, p] - want[p]).max()
            assert err <= 1e-12 * np.abs(want[p]).max(), (i, p, err)
        got_m = mask[i].astype(bool)
        amb = ref.ambiguous
        assert int(amb.sum()) == 0
        assert np.array_equal(got_m[~amb], ref.mask[~amb]), (i, int((got_m != ref.mask).sum()))
        tables.append(want_ev)
    return tables


@pytest.mark.parametrize("shape", [(256, 256), (128, 384), (1024, 1024)])
@pytest.mark.parametrize("ring", [False, True])
def test_device_matches_restatement(shape, ring):
    T, F = shape
    n = 1 if T * F > 300000 else 3
    dev, ref = _pair(T, F, ring)
    _compare(dev.generate_batch(n, out="complex128"), ref, n)
    assert dev.sample_counter == n


@pytest.mark.parametrize("ring", [False, True])
def test_float_outputs_are_rounded_complex128(ring):
    from rfi_toolbox_amd.core import RFISimulator
    T, F, n = 128, 384, 2
    sim = RFISimulator(T, F, seed=11, device="cuda:0")
    sim.gibbs_ringing = ring
    outs = {}
    for out in ("complex128", "complex64", "nchw", "nhwc"):
        sim.sample_counter = 0
        r = sim.generate_batch(n, out=out)
        outs[out] = (r.data.numpy(), r.mask.numpy())
    z, m = outs["complex128"]
    assert np.array_equal(outs["complex64"][0], z.astype(np.complex64))
    stack = np.stack([np.stack([z[i, 0].real, z[i, 0].imag, z[i, 1].real, z[i, 1].imag, z[i, 2].real, z[i, 2].imag,
                                z[i, 3].real, z[i, 3].imag], axis=0) for i in range(n)])      # save_example_pair_npy
    assert np.array_equal(outs["nchw"][0], stack.astype(np.float32))
    assert np.array_equal(outs["nhwc"][0], np.ascontiguousarray(stack.transpose(0, 2, 3, 1)).astype(np.float32))
    for out in outs:
        assert np.array_equal(outs[out][1], m), out


def test_batch_split_invariance_and_reproducibility():
    from rfi_toolbox_amd.core import RFISimulator
    T, F = 256, 256
    mk = lambda: RFISimulator(T, F, seed=42, device="cuda:0")   # noqa: E731
    a = mk().generate_batch(4, out="complex128")
    b = mk()
    b1, b2 = b.generate_batch(2, out="complex128"), b.generate_batch(2, out="complex128")
    za, ma = a.data.numpy(), a.mask.numpy()
    assert np.array_equal(za, np.concatenate([b1.data.numpy(), b2.data.numpy()]))
    assert np.array_equal(ma, np.concatenate([b1.mask.numpy(), b2.mask.numpy()]))
    assert np.array_equal(a.events.numpy(), np.concatenate([b1.events.numpy(), b2.events.numpy()]))
    c = mk()
    for i in range(4):
        tf, mask = c.generate_rfi()
        assert np.array_equal(np.stack([tf[p] for p in ("RR", "RL", "LR", "LL")]), za[i])
        assert np.array_equal(mask, ma[i].astype(bool)) and mask.dtype == bool
        assert c.baseline_frac == a.baseline_frac.numpy()[i]
    again = mk().generate_batch(4, out="complex128")
    assert np.array_equal(again.data.numpy(), za) and np.array_equal(again.mask.numpy(), ma)


def test_generate_batch_leaves_state_alone():
    from rfi_toolbox_amd.core import RFISimulator
    sim = RFISimulator(64, 64, seed=1, device="cuda:0")
    tf0, m0, bl0 = sim.tf_plane, sim.mask, sim.baseline_frac
    sim.generate_batch(2)
    assert sim.tf_plane is tf0 and sim.mask is m0 and sim.baseline_frac == bl0
    tf, mask = sim.generate_rfi()
    assert sim.tf_plane is tf and sim.mask is mask and tf["RR"].dtype == np.complex128 and tf["RR"].shape == (64, 64)


@pytest.mark.parametrize("attrs", [{"detect_floor": 30.0}, {"detect_floor": 1e-3}, {"drift_prob": 0.0},
                                   {"drift_prob": 1.0}, {"power_range": np.array([0.5, 7.0, 2500.0])},
                                   {"power_range": np.array([3.0])}, {"max_time_fringes": 2.0, "max_freq_fringes": 1.0}])
def test_attribute_changes_take_effect(attrs):
    dev, ref = _pair(128, 384, False, seed=7)
    dev.generate_batch(1)                      # the change applies to the NEXT call
    ref.generate_rfi()
    for s in (dev, ref):
        for k, v in attrs.items():
            setattr(s, k, v)
    tables = _compare(dev.generate_batch(2, out="complex128"), ref, 2)
    NN, NB = int(384 * 0.05), int(128 * 0.1)
    for ev in tables:
        drift = np.concatenate([ev["i2"][1:1 + ev["i0"][0]], ev["i1"][4:4 + NN], ev["i2"][4 + NN + NB:9 + NN + NB]])
        if attrs.get("drift_prob") == 0.0:
            assert not drift.any() and np.all(ev["sdot"][:9 + NN + NB] == 0)
        if attrs.get("drift_prob") == 1.0:
            assert drift.all()
        if "power_range" in attrs:
            assert set(ev["v0"][4:4 + NN + NB].tolist()) <= set(attrs["power_range"].tolist())


def test_explicit_baseline_frac():
    dev, ref = _pair(256, 256, True, seed=8)
    b = dev.generate_batch(2, baseline_frac=0.125, out="complex128")
    _compare(b, ref, 2, baseline_frac=0.125)
    assert np.all(b.baseline_frac.numpy() == 0.125)
    tf, mask = dev.generate_rfi(baseline_frac=0.9)
    assert dev.baseline_frac == 0.9


def test_generate_clean_data(golden_dir):
    with open(os.path.join(golden_dir, "simulator_expected.json")) as f:
        golden = json.load(f)
    from rfi_toolbox_amd.core import RFISimulator
    for T, F in ((256, 256), (128, 384)):
        dev, ref = RFISimulator(T, F, seed=3, device="cuda:0"), RefSimulator(T, F, seed=3)
        tf, mask = dev.generate_clean_data()
        ref.generate_clean_data()
        assert not mask.any() and mask.dtype == bool
        for p in ("RR", "RL", "LR", "LL"):
            assert np.abs(tf[p] - ref.tf_plane[p]).max() <= 1e-12 * np.abs(ref.tf_plane[p]).max()
        b = dev.generate_batch(12, clean=True, out="complex128")
        assert b.events is None and not b.mask.numpy().any()
        z = b.data.numpy()
        bad = within_spread(aggregate([clean_stats(z[i]) for i in range(12)]), golden["stats"][f"{T}x{F}_clean"], k=4.0)
        assert not bad, bad


def test_value_error_before_launch():
    from rfi_toolbox_amd.core import RFISimulator
    for T, F in ((64, 51), (3, 64)):
        sim = RFISimulator(T, F, seed=0, device="cuda:0")
        with pytest.raises(ValueError):
            sim.generate_rfi()
        with pytest.raises(ValueError):
            sim.generate_batch(1, out="nhwc")
        assert sim._ctx is None and sim.sample_counter == 0


@pytest.mark.parametrize("shape", [(256, 256), (128, 384)])
@pytest.mark.parametrize("ring", [False, True])
def test_device_statistics_within_reference_spread(golden_dir, shape, ring):
    with open(os.path.join(golden_dir, "simulator_expected.json")) as f:
        golden = json.load(f)
    from rfi_toolbox_amd.core import RFISimulator
    T, F = shape
    sim = RFISimulator(T, F, seed=99, device="cuda:0")
    sim.gibbs_ringing = ring
    b = sim.generate_batch(24, out="complex128")
    z, m = b.data.numpy(), b.mask.numpy().astype(bool)
    per = [sample_stats(z[i], m[i]) for i in range(24)]
    bad = within_spread(aggregate(per), golden["stats"][f"{T}x{F}_ring{int(ring)}"], k=4.0)
    assert not bad, bad


def test_nhwc_batch_feeds_unet8_train_step():
    from rfi_toolbox_amd.core import RFISimulator
    from rfi_toolbox_amd.models import UNet
    sim = RFISimulator(256, 256, seed=5, device="cuda:0")
    b = sim.generate_batch(4, out="nhwc")
    assert b.data.shape == (4, 256, 256, 8) and b.mask.shape == (4, 256, 256)
    torch.manual_seed(0)
    m1 = UNet(8, 1, 8, device="cuda:0")
    state = OrderedDict((k, v.clone()) for k, v in m1.state_dict().items())
    torch.manual_seed(0)
    m2 = UNet(8, 1, 8, device="cuda:0")
    for k, v in m2.state_dict().items():
        assert torch.equal(v, state[k]), k
    loss_dev = m1.train_step(b.data, b.mask)
    loss_host = m2.train_step(b.data.numpy(), b.mask.numpy())
    assert np.isfinite(loss_dev) and loss_dev == loss_host
