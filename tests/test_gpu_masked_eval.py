"""-m gpu: the evaluation counts with the ignore switch on (masked_confusion) and the label byte through the Augmenter.

test_eval_batch_counts_valid_pixels   eval_batch for a map and for class bits equals NumPy counts over the valid pixels of the
                                      device's own logits, as exact integers; with the switch off the counts are the old ones
test_evaluate_rfi_model_averages      evaluate_rfi_model on a two-batch dataset is the per-batch mean of those counts' metrics
test_augmenter_carries_bit7           the warped bytes' bit 7 is the warp of bit 7; flip-only samples are bit-exact copies
"""
import numpy as np
import pytest

import class_loss_ref as R
import masked_loss_ref as M
from rfi_toolbox_amd.evaluation.metrics import _dice, _f1, _iou, _precision, _recall
from rfi_toolbox_amd.models import UNet
from rfi_toolbox_amd.training import Augmenter, evaluate_rfi_model

pytestmark = pytest.mark.gpu

SHAPE = R.SHAPES[1]              # 3 x 34 x 46: several blocks at every K, no multiple of a wave
THRESHOLDS = (0.5, 0.3)


def _counts(logits, t, v, thr):
    """(K, 3) int64 [tp, fp, fn] over the pixels with v: sigmoid in float32 as the kernel forms it"""
    x = logits.astype(np.float32)
    pred = (np.float32(1.0) / (np.float32(1.0) + np.exp(-x, dtype=np.float32))) > np.float32(thr)
    keep = v.astype(bool)[:, None]
    t = t.astype(bool)
    return np.stack([(pred & t & keep).sum(0), (pred & ~t & keep).sum(0), (~pred & t & keep).sum(0)], axis=1).astype(np.int64)


def _near_threshold(logits, thr):
    """pixels whose sigmoid is within float32 rounding of the threshold (expf on the host and the device may differ there)"""
    p = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
    return np.abs(p - thr) < 1e-6


@pytest.mark.parametrize("K,targets", [(1, "map"), (1, "class_bits"), (5, "class_bits"), (7, "class_bits")])
def test_eval_batch_counts_valid_pixels(K, targets):
    case = M._case(K, targets, SHAPE, "default", "third", False, ("bce_dice",))
    m = UNet(3, K, 4, depth=1).set_targets(targets).eval()
    m.load_state_dict(R.head_state(K, SHAPE, "default"))
    x, y = R.loss_input(SHAPE), M.labels_of(case)
    assert ((y & 0x80) != 0).any()
    m.eval_batch(x, y, 0.5)
    logits = m.debug_tensor("logits").reshape(-1, K)          # the eval-mode logits every count below is taken from
    for thr in THRESHOLDS:
        assert not _near_threshold(logits, thr).any()
        for switch in (True, False):
            m.set_ignore(switch)
            t, v = M.targets_of(y, K, targets, switch)
            want = _counts(logits, t, v, thr)
            got = np.asarray(m.eval_batch(x, y, thr), np.int64).reshape(-1, 3)
            assert got.dtype == np.int64 and np.array_equal(got, want), (thr, switch, got, want)
        # the switch changes the counts: the ignored pixels carry targets and predictions
        assert not np.array_equal(_counts(logits, *M.targets_of(y, K, targets, True), thr),
                                  _counts(logits, *M.targets_of(y, K, targets, False), thr))


def test_evaluate_rfi_model_averages():
    K = 5
    case = M._case(K, "class_bits", SHAPE, "default", "third", False, ("bce_dice",))
    m = UNet(3, K, 4, depth=1).set_targets("class_bits").set_ignore(True).train()
    m.load_state_dict(R.head_state(K, SHAPE, "default"))
    x, y = R.loss_input(SHAPE).numpy(), M.labels_of(case)
    got = evaluate_rfi_model(m, (x, y), batch_size=2, threshold=0.5)
    assert m.training
    m.eval()
    rows = [np.asarray(m.eval_batch(x[s], y[s], 0.5), np.int64) for s in (slice(0, 2), slice(2, 3))]
    rules = {"iou": _iou, "precision": _precision, "recall": _recall, "f1": _f1, "dice": _dice}
    for k in range(K):
        for name, f in rules.items():
            want = float(np.mean([f(*(int(v) for v in r[k])) for r in rows]))
            assert got["per_class"][k][name] == want, (k, name)
    valid = (y & 0x80) == 0
    assert sum(int(r[:, 0].sum() + r[:, 2].sum()) for r in rows) == int(M.targets_of(y, K, "class_bits", True)[0][valid.reshape(-1)].sum())


def test_augmenter_carries_bit7():
    n, h, w = 8, 20, 28
    rng = np.random.default_rng(5)
    y = rng.integers(0, 128, (n, h, w), dtype=np.uint8) | (rng.random((n, h, w)) < 0.3).astype(np.uint8) << 7
    y = y.astype(np.uint8)
    x = rng.standard_normal((n, h, w, 3)).astype(np.float32)
    aug = Augmenter(seed=3)
    gates, _ = aug.params(n, h, w, call=1)
    out = aug(x, y, call=1)[1].numpy()
    hi = aug(x, y & np.uint8(0x80), call=1)[1].numpy()
    lo = aug(x, y & np.uint8(0x7F), call=1)[1].numpy()
    assert np.array_equal(out & 0x80, hi) and np.array_equal(out & 0x7F, lo)
    flip_only = [i for i in range(n) if not gates[i, 2] and not gates[i, 3]]
    warped = [i for i in range(n) if gates[i, 2] or gates[i, 3]]
    assert flip_only and warped
    for i in flip_only:
        want = y[i]
        if gates[i, 0]:
            want = want[:, ::-1]
        if gates[i, 1]:
            want = want[::-1, :]
        assert np.array_equal(out[i], want), i
