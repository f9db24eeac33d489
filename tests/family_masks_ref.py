"""TEST INFRASTRUCTURE ONLY -- per-family class-bit targets of a simulated batch in NumPy: the OR by family of the
restatement's per-event masks (tests/sim_instances_ref.py).  Bit c - 1 is set where an event of ``EVENT_CLASSES[c]``
(1 broadband .. 5 quadratic sweep) flags the pixel."""
import functools

import numpy as np

import sim_instances_ref as ref

NUM_FAMILIES = 5


def sample_bits(sample, T, F):
    """(T, F) uint8 of one of ``sim_instances_ref.case_reference``'s samples"""
    bits = np.zeros((T, F), np.uint8)
    for cls, mask in zip(ref.classes(T, F), sample["masks"]):
        bits |= mask.astype(np.uint8) << np.uint8(cls - 1)
    return bits


@functools.lru_cache(maxsize=None)
def case_bits(T, F, seed, n, detect_floor=1.0, first_sample=0):
    """(n, T, F) uint8 of a case, computed once and shared (treat as read-only)"""
    return np.stack([sample_bits(s, T, F) for s in ref.case_reference(T, F, seed, n, detect_floor, first_sample)])
