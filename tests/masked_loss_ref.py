"""Float64 closed forms of the three losses with an ignore bit and per-channel positive weights, and the case table of the
device sweep.  NumPy / torch on the CPU only: test_masked_loss_host.py pins them without a GPU, test_gpu_masked_loss.py
runs the kernels against them.

Logits are ``(pixels, K)`` channel-last and there is one label byte per pixel, as in class_loss_ref.  With the switch on, a
pixel whose byte has bit 7 set is ignored (v = 0, else 1) and the targets come from the low seven bits: bit k for class-bit
targets, "any bit" for a map.  With the switch off the byte means what it means to class_loss_ref.  pi_k is the weight of
channel k (1 when unset), N_v = K sum v, and in log space (softplus, log p = -softplus(-x)):

    BCE    sum v [pi t softplus(-x) + (1 - t) softplus(x)] / N_v                       (0 when N_v = 0)
    dice   I = sum v p t, P = sum v p, T = sum v t, pooled (bce_dice) or per channel (bce_class_dice, mean of the K terms)
    focal  the mean of loss_step_cases.focal_ref's element over the valid elements     (0 when there are none)
    d/dx   v [ (t ? -pi (1 - p) : p) / N_v + w p (1 - p) ((2 I + 1) / D^2 - 2 t / D) ],  w = 1 pooled, 1/K per channel

The dtype of the logits decides the arithmetic, as in class_loss_ref: the same text on a float32 tensor is the float32
restatement whose own dlogits error e_ref scales the device test's bound (loss_step_cases.grad_bound).

CASES is a pairwise table: every pair of values of any two of the six factors (channels and target kind, shape, logit
range, ignore pattern, weights, loss) that can occur together occurs in some case, chosen greedily in a fixed order.  Focal
takes no weights.  WEIGHT_ONLY_CASES are the K = 8 cases: weights set, the switch off, label bytes over all 256 values.
"""
import itertools
from collections import namedtuple

import numpy as np
import torch

import class_loss_ref as R
import loss_step_cases as L

IGNORE = 0x80
WEIGHTS = (0.5, 50.0, 1.0, 7.0, 20.0, 3.0, 0.0, 2.0)          # (includes a zero weight, at channel 6)
HEADS = ((1, "map"), (1, "class_bits"), (2, "class_bits"), (5, "class_bits"), (7, "class_bits"))
SHAPES = R.SHAPES
RANGES = R.RANGES
PATTERNS = ("none", "third", "all_but_one", "sample0", "all")
LOSSES = (("bce_dice",), ("bce_class_dice",), ("focal", 0.25, 2.0))

MaskedCase = namedtuple("MaskedCase", "id K targets shape logits ignore weights loss switch")


def _tag(loss):
    return loss[0] if loss[0] != "focal" else f"focal_a{loss[1]:g}_g{loss[2]:g}"


def _case(K, targets, shape, logits, ignore, weights, loss, switch=True):
    s = "x".join(map(str, shape))
    name = f"k{K}{'map' if targets == 'map' else ''}_{s}_{logits}_{ignore if switch else 'off'}_{'w' if weights else 'nw'}_{_tag(loss)}"
    return MaskedCase(name, K, targets, shape, logits, ignore, weights, loss, switch)


def _allowed(head, shape, logits, ignore, weights, loss):
    if loss[0] == "focal" and weights:
        return False                                           # focal has alpha
    if loss[0] == "bce_class_dice" and head[1] == "map":
        return False                                           # the per-class dice term needs class-bit targets
    return True


def _pairs(row):
    return {(i, a, j, b) for (i, a), (j, b) in itertools.combinations(enumerate(row), 2)}


def _pairwise():
    rows = [r for r in itertools.product(HEADS, SHAPES, RANGES, PATTERNS, (False, True), LOSSES) if _allowed(*r)]
    todo = set().union(*(_pairs(r) for r in rows))
    chosen = []
    while todo:
        best = max(rows, key=lambda r: len(_pairs(r) & todo))   # (max keeps the first of equals: a fixed order)
        chosen.append(best)
        todo -= _pairs(best)
    return chosen


CASES = [_case(h[0], h[1], s, r, ig, w, loss) for h, s, r, ig, w, loss in _pairwise()]
WEIGHT_ONLY_CASES = [_case(8, "class_bits", s, r, "none", True, loss, switch=False)
                     for s in SHAPES for r in RANGES for loss in LOSSES[:2]]
ALL_CASES = CASES + WEIGHT_ONLY_CASES


def weights_of(case):
    """float32 (K,) or None"""
    return np.asarray(WEIGHTS[:case.K], np.float32) if case.weights else None


def ignore_mask(pattern, shape):
    """(N, H, W) bool"""
    n, h, w = shape
    if pattern == "none":
        return np.zeros(shape, bool)
    if pattern == "all":
        return np.ones(shape, bool)
    if pattern == "sample0":
        m = np.zeros(shape, bool)
        m[0] = True
        return m
    if pattern == "all_but_one":
        m = np.ones(n * h * w, bool)
        m[(n * h * w) // 3] = False
        return m.reshape(shape)
    return np.random.default_rng(23 + n * h * w).random(shape) < 1.0 / 3.0


def labels_of(case):
    """(N, H, W) uint8.  Switch on: random low bits under every pixel, the ignored ones too, and bit 7 by the pattern; a map
    has a quarter of its pixels RFI, with several values of the low bits.  Switch off: bytes over all 256 values."""
    base = R.labels_of(R.ClassCase("", case.K, case.shape, "random", case.loss, case.logits))
    if not case.switch:
        return base
    low = base & np.uint8(0x7F)
    if case.targets == "map":
        low = np.where((base & 3) == 3, low, 0).astype(np.uint8)
    return low | (ignore_mask(case.ignore, case.shape).astype(np.uint8) << 7).astype(np.uint8)


def targets_of(labels, K, targets, switch):
    """(t (pixels, K) float64, v (pixels,) float64) of label bytes"""
    b = np.asarray(labels, np.uint8).reshape(-1)
    v = ((b & IGNORE) == 0) if switch else np.ones(b.shape, bool)
    low = b & np.uint8(0x7F) if switch else b
    t = (low != 0).astype(np.float64)[:, None] if targets == "map" else R.unpack(low, K)
    assert t.shape == (b.size, K)
    return t, v.astype(np.float64)


def masked_ref(loss, x, t, v, pi):
    """(loss, dlogits) in the dtype of x: x, t (pixels, K), v (pixels,), pi (K,) tensors of that dtype"""
    K = x.shape[1]
    vv = v[:, None]
    nv = K * v.sum()
    zero = torch.zeros((), dtype=x.dtype)
    if float(nv) == 0:
        return zero, torch.zeros_like(x)
    sp, sn = L._softplus(x), L._softplus(-x)
    p, q = torch.exp(-sn), torch.exp(-sp)
    pos = t > 0
    if loss[0] == "focal":
        alpha, gamma = loss[1], loss[2]
        a1, a0 = (alpha, 1 - alpha) if alpha >= 0 else (1.0, 1.0)
        qg, pg = torch.exp(-gamma * sp), torch.exp(-gamma * sn)
        val = torch.where(pos, a1 * qg * sn, a0 * pg * sp)
        grad = torch.where(pos, -a1 * qg * (gamma * p * sn + q), a0 * pg * (gamma * q * sp + p))
        return (vv * val).sum() / nv, vv * grad / nv
    bce = (vv * torch.where(pos, pi * sn, sp)).sum() / nv
    pmt = torch.where(pos, -pi * q, p)                           # pi-weighted p - t without cancellation
    if loss[0] == "bce_dice":
        inter, d = (vv * p * t).sum(), (vv * p).sum() + (vv * t).sum() + 1
        num = 2 * inter + 1
        return bce + 1 - num / d, vv * (pmt / nv + p * q * (num / (d * d) - 2 * t / d))
    inter, d = (vv * p * t).sum(0), (vv * p).sum(0) + (vv * t).sum(0) + 1
    num = 2 * inter + 1
    return bce + (1 - num / d).sum() / K, vv * (pmt / nv + p * q * (num / (d * d) - 2 * t / d) / K)


def reference(case, logits, labels, dtype=torch.float64):
    """(loss, dlogits (pixels, K)) of a case by the closed forms in `dtype` from (pixels, K) logits and the label bytes"""
    x = torch.as_tensor(np.asarray(logits)).to(dtype).reshape(-1, case.K)
    t, v = targets_of(labels, case.K, case.targets, case.switch)
    w = weights_of(case)
    pi = torch.ones(case.K, dtype=dtype) if w is None else torch.as_tensor(w).to(dtype)
    return masked_ref(case.loss, x, torch.as_tensor(t).to(dtype), torch.as_tensor(v).to(dtype), pi)


def figures(case, logits, labels):
    """(loss64, g64 (pixels, K) ndarray, e_ref = max |g32 - g64| of the float32 restatement, its loss error)"""
    l64, g64 = reference(case, logits, labels)
    l32, g32 = reference(case, logits, labels, torch.float32)
    return float(l64), g64.numpy(), float((g32.double() - g64).abs().max()), abs(float(l32) - float(l64))


def definition(case, logits, labels):
    """(loss, dlogits) in float64 through autograd of the definition in torch ops (unsaturated logits only)"""
    import torch.nn.functional as F
    x = torch.as_tensor(np.asarray(logits)).double().reshape(-1, case.K).clone().requires_grad_(True)
    t, v = targets_of(labels, case.K, case.targets, case.switch)
    t, vv = torch.as_tensor(t), torch.as_tensor(v)[:, None]
    w = weights_of(case)
    K = case.K
    nv = K * float(v.sum())
    if nv == 0:
        return torch.zeros((), dtype=torch.float64), torch.zeros_like(x)
    p = torch.sigmoid(x)
    if case.loss[0] == "focal":
        alpha, gamma = case.loss[1], case.loss[2]
        ce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
        pt = p * t + (1 - p) * (1 - t)
        at = alpha * t + (1 - alpha) * (1 - t) if alpha >= 0 else 1.0
        loss = (vv * at * (1 - pt) ** gamma * ce).sum() / nv
    else:
        pw = None if w is None else torch.as_tensor(w).double()
        bce = (vv * F.binary_cross_entropy_with_logits(x, t, pos_weight=pw, reduction="none")).sum() / nv
        dims = None if case.loss[0] == "bce_dice" else 0
        inter = (vv * p * t).sum() if dims is None else (vv * p * t).sum(0)
        tot = (vv * p).sum() + (vv * t).sum() if dims is None else (vv * p).sum(0) + (vv * t).sum(0)
        loss = bce + (1 - (2.0 * inter + 1.0) / (tot + 1.0)).mean()
    g, = torch.autograd.grad(loss, x)
    return loss.detach(), g
