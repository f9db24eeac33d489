"""No GPU: the per-family class-bit targets of the restatement (tests/family_masks_ref.py) on every case of the instance
tests -- what the device's ``family_masks`` is compared with bit for bit."""
import numpy as np
import pytest

import family_masks_ref as fam
import sim_instances_ref as ref
from sim_instances_cases import CASES, ODD_PLANE, case_id


@pytest.mark.parametrize("case", CASES + (ODD_PLANE,), ids=case_id)
def test_family_bits_of_the_restatement(case):
    T, F, seed, n = case
    bits = fam.case_bits(*case)
    samples = ref.case_reference(*case)
    assert bits.shape == (n, T, F) and bits.dtype == np.uint8
    assert not (bits >> fam.NUM_FAMILIES).any()                          # no bit above 4
    for i, s in enumerate(samples):
        assert not s["ambiguous"].any()
        assert np.array_equal(bits[i] != 0, s["mask"]), i                # the union over the families is the mask
    several = bits & (bits - 1)                                          # non-zero where more than one bit is set
    assert several.any()
    if T >= 40 and F >= 64:
        for c in range(fam.NUM_FAMILIES):
            assert ((bits >> c) & 1).reshape(n, -1).any(axis=1).any(), c     # every family is there in some sample
    print(f"FAMILYBITS {case_id(case)} pixels per family " +
          " ".join(str(int(((bits >> c) & 1).sum())) for c in range(fam.NUM_FAMILIES)) + f" several={int((several != 0).sum())}")


def test_bits_follow_the_class_table():
    """bit c - 1 belongs to EVENT_CLASSES[c]: the one-event masks of a family OR into that bit and into no other"""
    T, F, seed, n = CASES[3]
    cls = ref.classes(T, F)
    assert cls.min() == 1 and cls.max() == fam.NUM_FAMILIES
    for s, bits in zip(ref.case_reference(*CASES[3]), fam.case_bits(*CASES[3])):
        for c in range(1, fam.NUM_FAMILIES + 1):
            assert np.array_equal((bits >> (c - 1)) & 1, s["masks"][cls == c].any(axis=0).astype(np.uint8)), c
