"""No GPU: the float64 references of the class-bit losses (tests/class_loss_ref.py) and the label packing.

test_case_table                     K, shapes, labels, losses and ranges of the device sweep; the pixel counts miss wave and block
test_logit_coverage                 the saturated setups reach +-80 on the float32 oracle's logits, on both sides
test_pooled_is_segmentation_loss    bce_dice on (pixels, K) equals unet_ref.segmentation_loss on (N, K, H, W) in float64, loss and gradient
test_class_dice_against_autograd    bce_class_dice equals float64 autograd of its definition on unsaturated logits
test_one_class_is_the_reference     K = 1: both dice forms equal loss_step_cases.bce_dice_ref
test_high_bits_are_ignored          bits at and above K do not reach the targets
test_pack_unpack_round_trip         pack_class_masks / unpack_class_bits, both layouts
test_restatement_error              prints e_ref per case: the float32 restatement's dlogits error in units of 2^-24 max |g64|

Lines printed: CLASSSETUP k<K> <shape> k=... b=... cover=...   CLASSLOSS <case> dloss=... e_ref=... (host)
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import class_loss_ref as R
import loss_step_cases as L
from oracle import unet_ref
from rfi_toolbox_amd.class_labels import pack_class_masks, unpack_class_bits


def test_case_table():
    ids = [c.id for c in R.CASES]
    assert len(set(ids)) == len(ids) == 4 * 2 * 2 * 4 * 4
    assert {(c.K, c.shape, c.logits, c.labels, c.loss) for c in R.CASES} == \
        set(itertools.product((1, 2, 5, 8), ((2, 6, 10), (3, 34, 46)), R.RANGES, R.LABELS, R.LOSSES))
    for n, h, w in R.SHAPES:
        assert all((n * h * w) % d for d in (64, 256)) and h % 2 == 0 and w % 2 == 0
    assert 3 * 34 * 46 * 8 > 2 * 256 * 8                    # more than one block at every K
    for c in R.CASES:
        y = R.labels_of(c)
        assert y.shape == c.shape and y.dtype == np.uint8
        t = R.unpack(y, c.K).reshape(-1, c.K)
        if c.labels == "random":
            assert len(np.unique(y)) == (120 if y.size == 120 else 256) or len(np.unique(y)) > 90
            assert all(0 < t[:, k].sum() < len(t) for k in range(c.K))
        elif c.labels == "zeros":
            assert t.sum() == 0
        elif c.labels == "ones":
            assert t.sum() == t.size
        elif c.K > 1:
            assert t[:, 0].sum() == 0 and t[:, -1].sum() == len(t)


@functools.lru_cache(maxsize=None)
def _logits(K, shape, rng):
    return R.oracle_logits(K, shape, rng)


@pytest.mark.parametrize("K", R.KS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_logit_coverage(K, shape):
    lo, hi, near, mx, finite = L.coverage(_logits(K, shape, "saturated").numpy())
    k, b = R.saturation(K, shape)
    print(f"CLASSSETUP k{K} {shape} k={k} b={b} cover={lo:.3f}/{hi:.3f}/{near}/{mx:.1f}")
    assert R.saturated_enough(lo, hi, near, mx) and finite
    assert L.coverage(_logits(K, shape, "default").numpy())[3] < 5


def _nchw(a, shape, K):
    n, h, w = shape
    return torch.as_tensor(np.asarray(a)).reshape(n, h, w, K).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("case", [c for c in R.CASES if c.loss[0] == "bce_dice" and c.logits == "default"], ids=lambda c: c.id)
def test_pooled_is_segmentation_loss(case):
    x, y = _logits(case.K, case.shape, "default").double(), R.labels_of(case)
    l64, g64 = R.reference(case.loss, x, y)
    xn = _nchw(x, case.shape, case.K).requires_grad_(True)
    tn = _nchw(R.unpack(y, case.K), case.shape, case.K)
    assert tuple(tn.shape) == (case.shape[0], case.K) + case.shape[1:]
    loss = unet_ref.segmentation_loss(xn, tn)
    g, = torch.autograd.grad(loss, xn)
    assert abs(float(loss) - float(l64)) <= 1e-12 * max(1.0, abs(float(l64)))
    assert float((g.permute(0, 2, 3, 1).reshape(-1, case.K) - g64).abs().max()) <= 1e-12 * float(g64.abs().max())


@pytest.mark.parametrize("case", [c for c in R.CASES if c.loss[0] == "bce_class_dice" and c.logits == "default"], ids=lambda c: c.id)
def test_class_dice_against_autograd(case):
    x, y = _logits(case.K, case.shape, "default").double(), R.labels_of(case)
    l64, g64 = R.reference(case.loss, x, y)
    xn = _nchw(x, case.shape, case.K).requires_grad_(True)
    loss = R.class_dice_loss(xn, _nchw(R.unpack(y, case.K), case.shape, case.K))
    g, = torch.autograd.grad(loss, xn)
    assert abs(float(loss) - float(l64)) <= 1e-12 * max(1.0, abs(float(l64)))
    assert float((g.permute(0, 2, 3, 1).reshape(-1, case.K) - g64).abs().max()) <= 1e-12 * float(g64.abs().max())


@pytest.mark.parametrize("rng", R.RANGES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_one_class_is_the_reference(shape, rng):
    x = _logits(1, shape, rng).double()
    y = R.labels_of(R.ClassCase("", 1, shape, "random", ("bce_dice",), rng))
    want_l, want_g = L.bce_dice_ref(x.reshape(-1), torch.as_tensor(R.unpack(y, 1)).reshape(-1))
    for loss in (("bce_dice",), ("bce_class_dice",)):
        l, g = R.reference(loss, x, y)
        assert abs(float(l) - float(want_l)) <= 1e-14 * max(1.0, abs(float(want_l)))
        assert float((g.reshape(-1) - want_g).abs().max()) <= 1e-14 * float(want_g.abs().max())


def test_high_bits_are_ignored():
    rng = np.random.default_rng(0)
    y = rng.integers(0, 256, (2, 6, 10), dtype=np.uint8)
    x = _logits(5, (2, 6, 10), "default")
    for loss in R.LOSSES:
        a, b = R.reference(loss, x, y), R.reference(loss, x, y & np.uint8(0x1F))
        assert float(a[0]) == float(b[0]) and torch.equal(a[1], b[1])
    assert np.array_equal(unpack_class_bits(y, 5), unpack_class_bits(y & np.uint8(0x1F), 5))
    assert not np.array_equal(unpack_class_bits(y, 5), unpack_class_bits(y & np.uint8(0x0F), 5))


def test_pack_unpack_round_trip():
    rng = np.random.default_rng(1)
    for K in (1, 3, 5, 8):
        m = rng.random((2, K, 9, 11)) < 0.4
        bits = pack_class_masks(m)
        assert bits.shape == (2, 9, 11) and bits.dtype == np.uint8 and int(bits.max()) < (1 << K)
        assert np.array_equal(unpack_class_bits(bits, K), m)
        last = np.moveaxis(m, 1, -1)
        assert np.array_equal(pack_class_masks(last), bits) and np.array_equal(pack_class_masks(last, channel_axis=-1), bits)
        assert np.array_equal(unpack_class_bits(bits, K, channel_axis=-1), last)
        assert np.array_equal(R.unpack(bits, K) != 0, last)                      # the references read the same bits
    every = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(pack_class_masks(unpack_class_bits(every, 8)), every)
    assert np.array_equal(pack_class_masks(unpack_class_bits(every, 3)), every & 7)
    assert pack_class_masks(np.full((2, 4, 4), 7)).max() == 3                    # non-zero is membership, not the value
    with pytest.raises(ValueError):
        pack_class_masks(np.zeros((9, 20, 20), bool))
    with pytest.raises(ValueError):
        unpack_class_bits(every, 9)
    with pytest.raises(ValueError):
        unpack_class_bits(every.astype(np.int32), 3)


E_REF = {}


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_restatement_error(case):
    x, y = _logits(case.K, case.shape, case.logits), R.labels_of(case)
    l64, g64, e_ref, dloss = R.figures(case.loss, x, y)
    assert np.isfinite(g64).all() and np.isfinite(l64)
    gmax = float(np.abs(g64).max())
    u = e_ref / (L.U24 * gmax)
    E_REF[case.id] = u
    print(f"CLASSLOSS {case.id} dloss={dloss / (L.U24 * max(1.0, abs(l64))):.2f}u24 e_ref={u:.2f} (host)")
    # what the device test's bounds rest on: the restatement itself is a float32 computation of a few roundings per element
    assert dloss <= L.loss_bound(l64)
    assert u <= 32
