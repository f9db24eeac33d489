"""-m gpu: the loss pair on class-bit labels (class_loss_reduce / class_loss_finish / class_loss_bwd) on the device's own
logits, against the float64 closed forms of tests/class_loss_ref.py (test_class_loss_host.py pins those on the CPU).

test_class_loss_and_dlogits   UNet(3, K, 4, depth=1), K in {1, 2, 5, 8}, 2 x 6 x 10 and 3 x 34 x 46 (pixel counts no multiple of
                              a wave or a block; the larger one spans several blocks), label bytes over all 256 values / all
                              0x00 / all 0xFF / one class empty with another full, default and saturated logits, the three
                              losses: the returned loss within 8 x 2^-24 max(1, |loss|), debug_tensor("dlogits") within
                              max(2 e_ref, 4 x 2^-24 max |g64|), every element finite, loss() bit-equal to forward_backward's
test_one_class_matches_map    K = 1: class-bit labels with bit 0 give the bits of the label-map step
test_map_mode_keeps_its_message   a label map on K = 2 still raises the one-channel message; bce_class_dice needs class bits
test_refusals                 the models class-bit labels are not for

Lines printed:  CLASSLOSS <case> dloss=..u24 (of 8) dgrad/bound=... e_ref=..u24 cover=...

ON AN MI355X, the largest over the K, shapes and label kinds of each (loss, logit range): the loss error in units of
2^-24 max(1, |loss64|) (bound 8), dlogits as a fraction of its bound max(2 e_ref, 4 x 2^-24 max |g64|), dlogits and the
float32 restatement's own error e_ref in units of 2^-24 max |g64|.  Every element finite in all 256 cases.

  loss               logits      dloss  dgrad/bound  dgrad  e_ref
  bce_class_dice     default     1.75   0.80         3.19   3.02
  bce_class_dice     saturated   1.25   0.81         4.04   3.16
  bce_dice           default     1.65   0.82         3.39   3.11
  bce_dice           saturated   1.12   0.83         3.52   2.65
  focal_a-1_g0.5     default     0.54   0.36         1.66   2.80
  focal_a-1_g0.5     saturated   0.96   0.39         1.57   3.16
  focal_a0.25_g2     default     0.12   0.52         2.47   3.25
  focal_a0.25_g2     saturated   0.81   0.47         2.43   3.58
"""
import functools
import math

import numpy as np
import pytest

import class_loss_ref as R
import loss_step_cases as L
from rfi_toolbox_amd.models import SimpleCNN, UNet, UNetOverfit, UNetResNet18

pytestmark = pytest.mark.gpu

_MODELS, _LOADED = {}, {}


def _model(K, shape, logits):
    if K not in _MODELS:
        _MODELS[K] = UNet(3, K, 4, depth=1).set_targets("class_bits").train()
    m = _MODELS[K]
    if _LOADED.get(K) != (shape, logits):
        m.load_state_dict(R.head_state(K, shape, logits))
        _LOADED[K] = (shape, logits)
    return m


@functools.lru_cache(maxsize=4)
def _input(shape):
    return R.loss_input(shape)


def _set_loss(m, loss):
    if loss[0] == "focal":
        m.set_loss("focal", alpha=loss[1], gamma=loss[2])
    else:
        m.set_loss(loss[0])


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_class_loss_and_dlogits(case):
    m = _model(case.K, case.shape, case.logits)
    _set_loss(m, case.loss)
    x, y = _input(case.shape), R.labels_of(case)
    loss = m.forward_backward(x, y)
    logits, dlogits = m.debug_tensor("logits"), m.debug_tensor("dlogits")
    assert logits.shape == dlogits.shape == (y.size * case.K,)
    loss_fwd = m.loss(x, y)
    l64, g64, e_ref, _ = R.figures(case.loss, logits.reshape(-1, case.K), y)
    dloss = abs(loss - l64)
    finite_g = bool(np.isfinite(dlogits).all())
    dgrad = float(np.abs(dlogits.reshape(-1, case.K).astype(np.float64) - g64).max()) if finite_g else float("inf")
    lo, hi, near, mx, finite = L.coverage(logits)
    gmax = float(np.abs(g64).max())
    bound = L.grad_bound(e_ref, g64)
    print(f"CLASSLOSS {case.id} dloss={dloss / (L.U24 * max(1.0, abs(l64))):.2f}u24 (of 8) dgrad/bound={dgrad / bound:.2f} "
          f"dgrad={dgrad / (L.U24 * gmax):.2f}u24 e_ref={e_ref / (L.U24 * gmax):.2f}u24 cover={lo:.2f}/{hi:.2f}/{near}/{mx:.0f}")
    assert finite
    if case.logits == "saturated":                        # the device's own logits reach what the case is for
        assert R.saturated_enough(lo, hi, near, mx), (lo, hi, near, mx)
    assert finite_g
    assert math.isfinite(loss) and dloss <= L.loss_bound(l64), (loss, l64)
    assert dgrad <= bound, (dgrad, bound, e_ref)
    assert np.float32(loss_fwd).tobytes() == np.float32(loss).tobytes(), (loss_fwd, loss)


@pytest.mark.parametrize("loss", [("bce_dice",), ("focal", 0.25, 2.0)], ids=lambda l: l[0])
def test_one_class_matches_map(loss):
    """one output channel: bit 0 as the class bit is the label map, and both loss paths give the same loss and dlogits bits"""
    shape = R.SHAPES[1]
    x = _input(shape)
    y = (R.labels_of(R.ClassCase("", 1, shape, "random", loss, "default")) & 1).astype(np.uint8)
    got = []
    for targets in ("class_bits", "map"):
        m = UNet(3, 1, 4, depth=1).set_targets(targets).train()
        m.load_state_dict(R.head_state(1, shape, "default"))
        _set_loss(m, loss)
        got.append((np.float32(m.forward_backward(x, y)).tobytes(), m.debug_tensor("dlogits").tobytes()))
    assert got[0] == got[1]


def test_map_mode_keeps_its_message():
    m = UNet(3, 2, 4, depth=1).train()
    x, y = _input(R.SHAPES[0]), np.zeros(R.SHAPES[0], np.uint8)
    with pytest.raises(RuntimeError, match="defined for out_channels == 1"):
        m.loss(x, y)
    with pytest.raises(RuntimeError, match="class-bit labels"):
        m.set_loss("bce_class_dice")
    m.set_targets("class_bits").set_loss("bce_class_dice")
    assert math.isfinite(m.loss(x, y))
    m.set_targets("map")                                  # back: the old message again
    with pytest.raises(RuntimeError, match="defined for out_channels == 1"):
        m.loss(x, y)
    with pytest.raises(ValueError):
        m.set_targets("bits")


def test_refusals():
    class _OverfitOneLevel(UNetOverfit):
        _DEPTH = 1
    for m in (_OverfitOneLevel(3, 2, 4), UNetResNet18(3, 2, 16), SimpleCNN(3, 2, 4)):
        with pytest.raises(RuntimeError, match="class-bit labels are for UNet"):
            m.set_targets("class_bits")
        assert m.targets == "map"
