"""No GPU: the float64 references of the losses with an ignore bit and positive weights (tests/masked_loss_ref.py).

test_case_table                  the pairwise table covers every pair of factor values that can occur together, stays small,
                                 and its labels carry what each case claims
test_against_autograd            the closed forms equal float64 autograd of the definition written with
                                 F.binary_cross_entropy_with_logits(pos_weight=, reduction="none") at default logits
test_plain_is_class_loss_ref     nothing ignored and unit weights: class_loss_ref.reference to 1e-14
test_ignored_bits_do_not_matter  the low seven bits under an ignored pixel change nothing, bit for bit
test_all_ignored_is_zero         loss exactly 0 and a zero gradient
test_restatement_error           prints e_ref per case: the float32 restatement's dlogits error in units of 2^-24 max |g64|

Lines printed: MASKEDLOSS <case> dloss=... e_ref=... (host)
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import class_loss_ref as R
import loss_step_cases as L
import masked_loss_ref as M


def test_case_table():
    ids = [c.id for c in M.ALL_CASES]
    assert len(set(ids)) == len(ids)
    assert 25 <= len(M.CASES) <= 60 and len(M.WEIGHT_ONLY_CASES) == 8
    rows = [((c.K, c.targets), c.shape, c.logits, c.ignore, c.weights, c.loss) for c in M.CASES]
    have = set().union(*(M._pairs(r) for r in rows))
    want = set().union(*(M._pairs(r) for r in itertools.product(M.HEADS, M.SHAPES, M.RANGES, M.PATTERNS, (False, True), M.LOSSES)
                         if M._allowed(*r)))
    assert have == want
    assert not any(c.loss[0] == "focal" and c.weights for c in M.ALL_CASES)
    assert {c.K for c in M.CASES} == {1, 2, 5, 7} and {c.ignore for c in M.CASES} == set(M.PATTERNS)
    assert 0.0 in M.WEIGHTS[:7] and len(M.WEIGHTS) == 8
    for c in M.ALL_CASES:
        y = M.labels_of(c)
        assert y.shape == c.shape and y.dtype == np.uint8
        t, v = M.targets_of(y, c.K, c.targets, c.switch)
        n_ign = int((v == 0).sum())
        if not c.switch:
            assert c.K == 8 and n_ign == 0 and len(np.unique(y)) > 90 and c.weights
            continue
        assert n_ign == {"none": 0, "all": y.size, "all_but_one": y.size - 1, "sample0": y[0].size}.get(c.ignore, n_ign)
        if c.ignore == "third":
            assert 0.2 * y.size < n_ign < 0.45 * y.size
        if n_ign:
            assert len(np.unique(y[(y & 0x80) != 0] & 0x7F)) > 1          # something lies under the ignored pixels
        if c.ignore in ("none", "third", "sample0"):
            assert all(0 < t[v > 0, k].sum() < (v > 0).sum() for k in range(c.K))


@functools.lru_cache(maxsize=None)
def _logits(K, shape, rng):
    return R.oracle_logits(K, shape, rng)


@pytest.mark.parametrize("case", [c for c in M.ALL_CASES if c.logits == "default"], ids=lambda c: c.id)
def test_against_autograd(case):
    x, y = _logits(case.K, case.shape, "default").double(), M.labels_of(case)
    l64, g64 = M.reference(case, x, y)
    loss, g = M.definition(case, x, y)
    assert abs(float(loss) - float(l64)) <= 1e-12 * max(1.0, abs(float(l64)))
    assert float((g - g64).abs().max()) <= 1e-12 * float(g64.abs().max())


@pytest.mark.parametrize("rng", R.RANGES)
@pytest.mark.parametrize("K", (1, 2, 5, 7, 8))
@pytest.mark.parametrize("loss", R.LOSSES, ids=lambda l: "_".join(map(str, l)))
def test_plain_is_class_loss_ref(loss, K, rng):
    shape = R.SHAPES[1]
    x = _logits(K, shape, rng).double()
    y = R.labels_of(R.ClassCase("", K, shape, "random", loss, rng))
    if K < 8:
        y = y & np.uint8(0x7F)
    want_l, want_g = R.reference(loss, x, y)
    for switch in ((True, False) if K < 8 else (False,)):
        case = M._case(K, "class_bits", shape, rng, "none", False, loss, switch=switch)
        l, g = M.reference(case, x, y)
        assert abs(float(l) - float(want_l)) <= 1e-14 * max(1.0, abs(float(want_l)))
        assert float((g - want_g).abs().max()) <= 1e-14 * float(want_g.abs().max())
    if K == 1:                                   # a map whose bytes are 0 / 1 is the one-class case
        case = M._case(1, "map", shape, rng, "none", False, loss)
        l, g = M.reference(case, x, y & np.uint8(1))
        want_l, want_g = R.reference(loss, x, y & np.uint8(1))
        assert abs(float(l) - float(want_l)) <= 1e-14 * max(1.0, abs(float(want_l)))
        assert float((g - want_g).abs().max()) <= 1e-14 * float(want_g.abs().max())


@pytest.mark.parametrize("case", [c for c in M.CASES if c.ignore not in ("none",)], ids=lambda c: c.id)
def test_ignored_bits_do_not_matter(case):
    x, y = _logits(case.K, case.shape, case.logits), M.labels_of(case)
    ign = (y & 0x80) != 0
    y2 = np.where(ign, y ^ np.uint8(0x7F), y).astype(np.uint8)
    assert not np.array_equal(y, y2) and np.array_equal(y[~ign], y2[~ign])
    for dtype in (torch.float64, torch.float32):
        a, b = M.reference(case, x, y, dtype), M.reference(case, x, y2, dtype)
        assert float(a[0]) == float(b[0]) and torch.equal(a[1], b[1])
        assert float(a[1].reshape(-1, case.K)[ign.reshape(-1)].abs().max()) == 0.0


@pytest.mark.parametrize("case", [c for c in M.CASES if c.ignore == "all"], ids=lambda c: c.id)
def test_all_ignored_is_zero(case):
    x, y = _logits(case.K, case.shape, case.logits), M.labels_of(case)
    for dtype in (torch.float64, torch.float32):
        l, g = M.reference(case, x, y, dtype)
        assert float(l) == 0.0 and not bool(g.any()) and g.shape == (y.size, case.K)


@pytest.mark.parametrize("case", M.ALL_CASES, ids=lambda c: c.id)
def test_restatement_error(case):
    x, y = _logits(case.K, case.shape, case.logits), M.labels_of(case)
    l64, g64, e_ref, dloss = M.figures(case, x, y)
    assert np.isfinite(g64).all() and np.isfinite(l64)
    gmax = float(np.abs(g64).max())
    u = e_ref / (L.U24 * gmax) if gmax else 0.0
    print(f"MASKEDLOSS {case.id} dloss={dloss / (L.U24 * max(1.0, abs(l64))):.2f}u24 e_ref={u:.2f} (host)")
    if case.ignore == "all":
        assert gmax == 0.0 and e_ref == 0.0 and l64 == 0.0
    # what the device test's bounds rest on: the restatement itself is a float32 computation of a few roundings per element
    assert dloss <= L.loss_bound(l64)
    assert u <= 32
