"""-m gpu: per-family class-bit targets of RFISimulator batches (rfi_sim_family_bits of csrc/rfi_sim.hip,
rfi_toolbox_amd.core.family_masks) against the NumPy restatement tests/family_masks_ref.py.  Bytes throughout, and no case
has a pixel within AMBIGUOUS of the floor (asserted here as in test_sim_instances_host.py): every comparison is exact."""
import numpy as np
import pytest

import family_masks_ref as fam
import sim_instances_ref as ref
from sim_instances_cases import CASES, ODD_PLANE, case_id

pytestmark = pytest.mark.gpu


def _sim(T, F, seed, **attrs):
    from rfi_toolbox_amd.core import RFISimulator
    sim = RFISimulator(T, F, seed=seed, device="cuda:0")
    for k, v in attrs.items():
        setattr(sim, k, v)
    return sim


def _bits(batch):
    from rfi_toolbox_amd import family_masks
    b = family_masks(batch)
    assert b.dtype == np.uint8 and b.shape == tuple(batch.mask.shape) and b.ctx is batch.mask.ctx
    return b.numpy()


@pytest.mark.parametrize("case", CASES + (ODD_PLANE,), ids=case_id)
def test_matches_restatement_mask_and_instances(case):
    from rfi_toolbox_amd.core import event_instances
    T, F, seed, n = case
    assert not any(s["ambiguous"].any() for s in ref.case_reference(*case))
    batch = _sim(T, F, seed).generate_batch(n)
    got = _bits(batch)
    want = fam.case_bits(*case)
    assert np.array_equal(got, want), [(i, int((got[i] != want[i]).sum())) for i in range(n)]
    assert np.array_equal(got != 0, batch.mask.numpy() != 0)
    # the OR by label of the instance masks of every event
    tg = event_instances(batch, max_instances=256)
    masks, labels, count, base = tg.masks.numpy(), tg.labels.numpy(), tg.count_host, tg.base.numpy()
    ored = np.zeros_like(got)
    for i in range(n):
        for j in range(int(count[i])):
            ored[i] |= masks[base[i] + j] << np.uint8(labels[i, j] - 1)
    assert np.array_equal(got, ored)


def test_ringing_first_sample_and_repeats():
    T, F, seed, n = CASES[4]
    base = _bits(_sim(T, F, seed).generate_batch(n))
    assert np.array_equal(base, _bits(_sim(T, F, seed, gibbs_ringing=True).generate_batch(n)))
    for out in ("complex128", "nhwc"):
        assert np.array_equal(base, _bits(_sim(T, F, seed).generate_batch(n, out=out)))
    # first_sample > 0: the second batch of a simulator continues the first
    sim = _sim(T, F, seed)
    first, rest = sim.generate_batch(1), sim.generate_batch(n - 1)
    assert rest.origin.first_sample == 1
    assert np.array_equal(base, np.concatenate([_bits(first), _bits(rest)]))
    assert np.array_equal(_bits(rest), fam.case_bits(T, F, seed, n - 1, 1.0, 1))
    assert _bits(rest).tobytes() == _bits(rest).tobytes()                # called twice


def test_clean_and_empty_batches():
    T, F, seed, n = CASES[3]
    clean = _sim(T, F, seed).generate_batch(n, clean=True)
    assert clean.events is None
    b = _bits(clean)
    assert b.shape == (n, T, F) and not b.any()
    empty = _bits(_sim(T, F, seed).generate_batch(0))
    assert empty.shape == (0, T, F)
    with pytest.raises(ValueError):
        from rfi_toolbox_amd.core import family_masks
        family_masks((1, 2, 3, 4))


def test_bad_arguments_are_error_codes():
    import copy
    import ctypes as C
    from rfi_toolbox_amd._lib import lib
    from rfi_toolbox_amd.core.instances import _sim_args
    from rfi_toolbox_amd.runtime import P
    T, F, seed, n = CASES[3]
    batch = _sim(T, F, seed).generate_batch(n)
    good = _sim_args(batch)
    out = batch.mask.ctx.empty((n, T, F), np.uint8)
    assert lib.rfi_sim_family_bits(*good, P(out)) == 0
    assert np.array_equal(out.numpy(), fam.case_bits(*CASES[3]))
    assert lib.rfi_sim_family_bits(*good, None) != 0

    def params(**kw):
        p = copy.copy(batch.origin.params)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    for bad in (params(time_bins=3), params(freq_bins=51), params(n_power=0), params(clean=1)):
        assert lib.rfi_sim_family_bits(*(good[:4] + (bad,) + good[5:]), P(out)) != 0
    assert lib.rfi_sim_family_bits(*good[:3], -1, *good[4:], P(out)) != 0
    assert np.array_equal(out.numpy(), fam.case_bits(*CASES[3]))         # the bad calls wrote nothing
