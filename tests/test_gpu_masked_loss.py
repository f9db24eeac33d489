"""-m gpu: the losses with an ignore bit and positive weights (masked_loss_reduce / masked_loss_finish / masked_loss_bwd) on
the device's own logits, against the float64 closed forms of tests/masked_loss_ref.py (test_masked_loss_host.py pins those
on the CPU).  UNet(3, K, 4, depth=1) as in test_gpu_class_loss.py.

test_masked_loss_and_dlogits   every case of the pairwise table and the K = 8 weights-only cases: the returned loss within 8 x
                               2^-24 max(1, |loss|), debug_tensor("dlogits") within max(2 e_ref, 4 x 2^-24 max |g64|), every
                               element finite, loss() bit-equal to forward_backward's, dlogits bitwise +0.0 at every ignored
                               element, a second run bit-identical, and the low seven bits under the ignored pixels flipped:
                               bit-identical again
test_switch_alone_changes_no_bit   switch on, no bit 7 set, no weights: loss and dlogits are those of the switch off, for each
                               loss and both target kinds (the reduction order is the existing kernels')
test_unit_weights_change_no_bit    weights of 1 without the switch: the same
test_all_ignored_step          train_step returns 0.0 and leaves a zero head gradient
test_refusals                  8 channels with the switch (both orders), weights with focal (both orders), a negative / NaN /
                               miscounted weight, the models out of scope, eval_sweep with the switch on; the model still steps
test_bfloat16_flow             one run in the "bfloat16" compute mode at 2 x 16 x 16: the plane flow reaches the same kernels

Lines printed:  MASKEDLOSS <case> dloss=..u24 (of 8) dgrad/bound=... dgrad=..u24 e_ref=..u24

ON AN MI355X over the 33 cases: the loss at most 1.13 x 2^-24 max(1, |loss64|) from float64 (bound 8), dlogits at most 0.82 of
its bound max(2 e_ref, 4 x 2^-24 max |g64|) and 3.63 x 2^-24 max |g64|, every element finite; the all-ignored cases exactly 0.
"""
import functools
import math

import numpy as np
import pytest

import class_loss_ref as R
import loss_step_cases as L
import masked_loss_ref as M
from rfi_toolbox_amd.models import SimpleCNN, UNet, UNetOverfit, UNetResNet18

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=4)
def _input(shape):
    return R.loss_input(shape)


def _set_loss(m, loss):
    m.set_pos_weight(None)
    if loss[0] == "focal":
        m.set_loss("focal", alpha=loss[1], gamma=loss[2])
    else:
        m.set_loss(loss[0])
    return m


_MODELS = {}


def _model(K, targets, shape, logits):
    key = (K, targets)
    if key not in _MODELS:
        _MODELS[key] = [UNet(3, K, 4, depth=1).set_targets(targets).train(), None]
    m, loaded = _MODELS[key]
    if loaded != (shape, logits):
        m.load_state_dict(R.head_state(K, shape, logits))
        _MODELS[key][1] = (shape, logits)
    return m


def _configure(case):
    m = _model(case.K, case.targets, case.shape, case.logits)
    m.set_ignore(False)
    _set_loss(m, case.loss)
    m.set_ignore(case.switch).set_pos_weight(M.weights_of(case))
    return m


def _bits(m, x, y):
    loss = m.forward_backward(x, y)
    return np.float32(loss).tobytes(), m.debug_tensor("dlogits").tobytes()


@pytest.mark.parametrize("case", M.ALL_CASES, ids=lambda c: c.id)
def test_masked_loss_and_dlogits(case):
    m = _configure(case)
    x, y = _input(case.shape), M.labels_of(case)
    loss = m.forward_backward(x, y)
    logits, dlogits = m.debug_tensor("logits"), m.debug_tensor("dlogits")
    assert logits.shape == dlogits.shape == (y.size * case.K,)
    loss_fwd = m.loss(x, y)
    l64, g64, e_ref, _ = M.figures(case, logits.reshape(-1, case.K), y)
    dloss = abs(loss - l64)
    finite_g = bool(np.isfinite(dlogits).all())
    dgrad = float(np.abs(dlogits.reshape(-1, case.K).astype(np.float64) - g64).max()) if finite_g else float("inf")
    gmax = float(np.abs(g64).max())
    bound = L.grad_bound(e_ref, g64)
    unit = L.U24 * gmax if gmax else 1.0
    print(f"MASKEDLOSS {case.id} dloss={dloss / (L.U24 * max(1.0, abs(l64))):.2f}u24 (of 8) "
          f"dgrad/bound={dgrad / bound if bound else dgrad:.2f} dgrad={dgrad / unit:.2f}u24 e_ref={e_ref / unit:.2f}u24")
    assert bool(np.isfinite(logits).all()) and finite_g
    assert math.isfinite(loss) and dloss <= L.loss_bound(l64), (loss, l64)
    assert dgrad <= bound, (dgrad, bound, e_ref)
    assert np.float32(loss_fwd).tobytes() == np.float32(loss).tobytes(), (loss_fwd, loss)
    ign = np.repeat(((y.reshape(-1) & 0x80) != 0) & case.switch, case.K)
    assert not dlogits.view(np.uint32)[ign].any()                     # every bit 0: +0.0
    if case.ignore == "all":
        assert loss == 0.0 and not dlogits.view(np.uint32).any()
    first = (np.float32(loss).tobytes(), dlogits.tobytes())
    assert _bits(m, x, y) == first                                      # a second run
    if ign.any():
        flipped = np.where((y & 0x80) != 0, y ^ np.uint8(0x7F), y).astype(np.uint8)
        assert not np.array_equal(flipped, y)
        assert _bits(m, x, flipped) == first


@pytest.mark.parametrize("loss,targets", [(l, t) for t in ("map", "class_bits") for l in M.LOSSES
                                          if t != "map" or l[0] != "bce_class_dice"],       # (the per-class term needs class bits)
                         ids=lambda v: M._tag(v) if isinstance(v, tuple) else v)
def test_switch_alone_changes_no_bit(loss, targets):
    shape = R.SHAPES[1]
    x = _input(shape)
    for K in ((1,) if targets == "map" else (1, 5, 7)):
        y = R.labels_of(R.ClassCase("", K, shape, "random", loss, "default")) & np.uint8(0x7F)
        for logits in R.RANGES:
            m = _set_loss(_model(K, targets, shape, logits), loss)
            off = _bits(m.set_ignore(False), x, y)
            on = _bits(m.set_ignore(True), x, y)
            m.set_ignore(False)
            assert on[0] == off[0], (K, logits)
            assert on[1] == off[1], (K, logits)


@pytest.mark.parametrize("loss", M.LOSSES[:2], ids=M._tag)
def test_unit_weights_change_no_bit(loss):
    shape, K = R.SHAPES[1], 8
    x = _input(shape)
    y = R.labels_of(R.ClassCase("", K, shape, "random", loss, "default"))
    m = _set_loss(_model(K, "class_bits", shape, "saturated").set_ignore(False), loss)
    off = _bits(m, x, y)
    on = _bits(m.set_pos_weight(1.0), x, y)
    m.set_pos_weight(None)
    assert m.pos_weight is None and on == off


def test_all_ignored_step():
    shape = R.SHAPES[0]
    for K, targets in ((1, "map"), (5, "class_bits")):
        m = UNet(3, K, 4, depth=1).set_targets(targets).set_ignore(True).train()
        y = np.full(shape, 0x80 | 0x15, np.uint8)
        assert m.train_step(_input(shape), y) == 0.0
        for name in ("final_conv.weight", "final_conv.bias"):
            g = m.grad(name)
            assert not g.any() and np.isfinite(g).all()
        assert all(np.isfinite(v.numpy()).all() for v in m.state_dict().values())


def test_refusals():
    shape = R.SHAPES[0]
    x = _input(shape)

    def steps(m):
        y = np.zeros(shape, np.uint8)
        y[0, 0, :3] = 1
        assert math.isfinite(m.train_step(x, y))

    m = UNet(3, 8, 4, depth=1).set_targets("class_bits").train()
    with pytest.raises(RuntimeError, match="out_channels <= 7"):
        m.set_ignore(True)
    assert m.ignore is False
    steps(m)
    m = UNet(3, 8, 4, depth=1).train().set_ignore(True)
    with pytest.raises(RuntimeError, match="out_channels <= 7"):
        m.set_targets("class_bits")
    assert m.targets == "map"
    m.set_ignore(False).set_targets("class_bits")
    steps(m)

    m = UNet(3, 2, 4, depth=1).set_targets("class_bits").train()
    m.set_loss("focal")
    with pytest.raises(RuntimeError, match="focal"):
        m.set_pos_weight([1.0, 2.0])
    assert m.pos_weight is None
    steps(m)
    m.set_loss("bce_dice").set_pos_weight([1.0, 2.0])
    with pytest.raises(RuntimeError, match="focal"):
        m.set_loss("focal")
    steps(m)
    for bad in ([1.0, -0.5], [float("nan"), 1.0], [float("inf"), 1.0], [1.0, 2.0, 3.0], [1.0]):
        with pytest.raises(RuntimeError, match="set_pos_weight"):
            m.set_pos_weight(bad)
        assert m.pos_weight == [1.0, 2.0]
        steps(m)
    assert m.set_pos_weight(None).pos_weight is None

    class _OverfitOneLevel(UNetOverfit):
        _DEPTH = 1
    for other in (_OverfitOneLevel(3, 1, 4), UNetResNet18(3, 1, 16), SimpleCNN(3, 1, 4)):
        with pytest.raises(RuntimeError, match="are for UNet, UNetBigger and UNetDifferentActivation"):
            other.set_ignore(True)
        with pytest.raises(RuntimeError, match="are for UNet, UNetBigger and UNetDifferentActivation"):
            other.set_pos_weight(2.0)
        assert other.ignore is False and other.pos_weight is None
    xs = np.zeros((1, 32, 32, 3), np.float32)
    assert math.isfinite(other.train_step(xs, np.zeros((1, 32, 32), np.uint8)))

    m = UNet(3, 1, 4, depth=1).set_ignore(True).train()
    with pytest.raises(RuntimeError, match="eval_sweep"):
        m.eval_sweep(x, np.zeros(shape, np.uint8), [0.5])
    steps(m)
    assert m.set_ignore(False).eval_sweep(x, np.zeros(shape, np.uint8), [0.5]).shape == (1, 3)


def test_bfloat16_flow():
    shape = (2, 16, 16)
    case = M._case(5, "class_bits", shape, "default", "third", True, ("bce_class_dice",))
    m = UNet(3, 5, 4, depth=1).set_targets("class_bits").set_compute_dtype("bfloat16").train()
    m.set_loss("bce_class_dice").set_ignore(True).set_pos_weight(M.weights_of(case))
    x, y = R.loss_input(shape), M.labels_of(case)
    loss = m.forward_backward(x, y)
    logits, dlogits = m.debug_tensor("logits"), m.debug_tensor("dlogits")
    l64, g64, e_ref, _ = M.figures(case, logits.reshape(-1, 5), y)
    assert abs(loss - l64) <= L.loss_bound(l64)
    assert float(np.abs(dlogits.reshape(-1, 5) - g64).max()) <= L.grad_bound(e_ref, g64)
    ign = np.repeat((y.reshape(-1) & 0x80) != 0, 5)
    assert ign.any() and not dlogits.view(np.uint32)[ign].any()
    assert np.float32(m.loss(x, y)).tobytes() == np.float32(loss).tobytes()
