"""Float64 closed forms of the three losses on class-bit labels and their dlogits, NumPy / torch on the CPU only.
test_class_loss_host.py pins them without a GPU, test_gpu_class_loss.py runs the kernels against them.

Logits are ``(pixels, K)`` channel-last, as the head writes them; a label byte per pixel, target of channel k =
``(label >> k) & 1``.  Written in log space like ``loss_step_cases.bce_dice_ref`` (softplus, log p = -softplus(-x)) and
never through autograd at saturated logits:

    bce_dice        mean over all pixels x K of BCE-with-logits + ONE dice term 1 - (2 I + 1) / (P + T + 1) over all of
                    them: ``bce_dice_ref`` on the flattened tensors, which is ``unet_ref.segmentation_loss``
    bce_class_dice  the same BCE mean + (1/K) sum_k [1 - (2 I_k + 1) / D_k], D_k = P_k + T_k + 1, sums per class
                    d/dx_{i,k} = (p - t) / (pixels K) + (1/K) p (1 - p) ((2 I_k + 1) / D_k^2 - 2 t / D_k)
    focal           ``focal_ref`` on the flattened tensors

The dtype of the logits decides the arithmetic: the same text on a float32 tensor is the float32 restatement whose own
dlogits error, ``e_ref`` in units of 2^-24 max |g64|, scales the device test's bound (``loss_step_cases.grad_bound``).

MEASURED by test_class_loss_host.py on the float32 CPU oracle's logits of ``CASES``: e_ref at most 3.61 x 2^-24 max |g64|
and the restatement's loss at most 2.89 x 2^-24 max(1, |loss64|) from float64 over the 256 cases (its CLASSLOSS lines).
The saturated setups put the farthest logit at +-80 with 2-29 % of the logits below -20 and 6-29 % above +20 (its
CLASSSETUP lines); the K-channel logits have heavier tails than the one-channel setups of loss_step_cases.
"""
from collections import namedtuple

import numpy as np
import torch

import loss_step_cases as L

KS = (1, 2, 5, 8)
SHAPES = ((2, 6, 10), (3, 34, 46))
LABELS = ("random", "zeros", "ones", "empty_full")
LOSSES = (("bce_dice",), ("bce_class_dice",), ("focal", 0.25, 2.0), ("focal", -1.0, 0.5))
RANGES = ("default", "saturated")

ClassCase = namedtuple("ClassCase", "id K shape labels loss logits")


def _tag(loss):
    return loss[0] if loss[0] != "focal" else f"focal_a{loss[1]:g}_g{loss[2]:g}"


CASES = [ClassCase(f"k{K}_{s[0]}x{s[1]}x{s[2]}_{r}_{lab}_{_tag(loss)}", K, s, lab, loss, r)
         for K in KS for s in SHAPES for r in RANGES for lab in LABELS for loss in LOSSES]

SEED = 3                 # the oracle's initial state: UNet(3, K, 4, depth=1)


def unpack(labels, K):
    """(...,) uint8 -> float64 (..., K) targets"""
    b = np.asarray(labels, dtype=np.uint8)
    return ((b[..., None] >> np.arange(K, dtype=np.uint8)) & 1).astype(np.float64)


def labels_of(case):
    """(N, H, W) uint8 over all 256 byte values / all 0x00 / all 0xFF / class 0 empty with class K - 1 full"""
    n, h, w = case.shape
    if case.labels == "zeros":
        return np.zeros((n, h, w), np.uint8)
    if case.labels == "ones":
        return np.full((n, h, w), 0xFF, np.uint8)
    rng = np.random.default_rng(11 + n * h * w + case.K)
    y = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    if case.labels == "empty_full":
        y = (y & np.uint8(0xFE)) | np.uint8(1 << (case.K - 1)) if case.K > 1 else np.zeros_like(y)
    return y


def head_state(K, shape, logits):
    from oracle import unet_ref
    st = unet_ref.init_state(3, K, 4, 1, seed=SEED)
    if logits == "saturated":
        k, b = saturation(K, shape)
        st["final_conv.weight"] = st["final_conv.weight"] * k
        st["final_conv.bias"] = torch.full_like(st["final_conv.bias"], b)
    return st


def loss_input(shape):
    n, h, w = shape
    g = torch.Generator().manual_seed(SEED + 1000 + n * h * w)
    return torch.randn(n, h, w, 3, generator=g)


def oracle_logits(K, shape, logits, state=None):
    """float32 CPU oracle's train-mode logits, (pixels, K)"""
    from oracle import unet_ref
    st = head_state(K, shape, logits) if state is None else state
    with torch.no_grad():
        out = unet_ref.forward(st, unet_ref.nhwc_to_nchw(loss_input(shape)), training=True)
    return out.permute(0, 2, 3, 1).reshape(-1, K)


_SAT = {}


def saturation(K, shape):
    """(k, b): the median of the float32 oracle's default logits moves to 0 and the farthest one to +-80, as
    loss_step_cases.search_setups chooses them (four and six significant digits)"""
    if (K, shape) not in _SAT:
        r = oracle_logits(K, shape, "default").double().numpy()
        # the head is linear in (weight, bias): logit' = k (logit - bias_c) + b per channel; the channels' own biases are
        # small against the spread, so centring the pooled median is what the one-channel setups do too
        from oracle import unet_ref
        bias = unet_ref.init_state(3, K, 4, 1, seed=SEED)["final_conv.bias"].double().numpy()
        z = r - bias
        med = float(np.median(z))
        k = float(f"{80.0 / float(np.abs(z - med).max()):.4g}")
        _SAT[(K, shape)] = (k, float(f"{-k * med:.6g}"))
    return _SAT[(K, shape)]


def saturated_enough(lo, hi, near, mx):
    """what a saturated setup must deliver (loss_step_cases.coverage's figures): the farthest logit at 60 .. 100, at least
    one in a hundred beyond -20 and beyond +20 (the K-channel logits have heavier tails than the one-channel setups of
    loss_step_cases, so fewer lie out there at the same farthest logit), and some inside |x| < 1"""
    return lo >= 0.01 and hi >= 0.01 and near > 0 and 60 <= mx <= 100


# ---- closed forms: x (pixels, K) tensor, t (pixels, K) tensor of its dtype -> (loss, dlogits (pixels, K))
def pooled_ref(x, t):
    loss, g = L.bce_dice_ref(x.reshape(-1), t.reshape(-1))
    return loss, g.reshape(x.shape)


def class_dice_ref(x, t):
    sp, sn = L._softplus(x), L._softplus(-x)
    p, q = torch.exp(-sn), torch.exp(-sp)
    n, K = x.numel(), x.shape[1]
    inter, d = (p * t).sum(0), p.sum(0) + t.sum(0) + 1            # per class
    num = 2 * inter + 1
    loss = (sp - x * t).sum() / n + (1 - num / d).sum() / K
    pmt = torch.where(t > 0, -q, p)                               # p - t without cancellation
    return loss, pmt / n + p * q * (num / (d * d) - 2 * t / d) / K


def focal_ref(x, t, alpha, gamma):
    loss, g = L.focal_ref(x.reshape(-1), t.reshape(-1), alpha, gamma)
    return loss, g.reshape(x.shape)


def reference(loss, logits, labels, dtype=torch.float64):
    """(loss, dlogits) by the closed forms in `dtype` from (pixels, K) logits and (pixels,) label bytes"""
    x = torch.as_tensor(np.asarray(logits)).to(dtype)
    t = torch.as_tensor(unpack(np.asarray(labels).reshape(-1), x.shape[1])).to(dtype)
    if loss[0] == "bce_dice":
        return pooled_ref(x, t)
    if loss[0] == "bce_class_dice":
        return class_dice_ref(x, t)
    return focal_ref(x, t, loss[1], loss[2])


def class_dice_loss(logits_nchw, targets_nchw, smooth=1.0):
    """the definition of bce_class_dice in torch ops, for autograd: logits / targets (N, K, H, W)"""
    x, y = logits_nchw, targets_nchw.to(logits_nchw.dtype)
    bce = (torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))).mean()
    p = torch.sigmoid(x)
    inter, tot = (p * y).sum(dim=(0, 2, 3)), p.sum(dim=(0, 2, 3)) + y.sum(dim=(0, 2, 3))
    return bce + (1 - (2.0 * inter + smooth) / (tot + smooth)).mean()


def figures(loss, logits, labels):
    """(loss64, g64 (pixels, K) ndarray, e_ref = max |g32 - g64| of the float32 restatement, its loss error)"""
    l64, g64 = reference(loss, logits, labels)
    l32, g32 = reference(loss, logits, labels, torch.float32)
    return float(l64), g64.numpy(), float((g32.double() - g64).abs().max()), abs(float(l32) - float(l64))


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for K in KS:
        for s in SHAPES:
            print(K, s, saturation(K, s), L.coverage(oracle_logits(K, s, "saturated").numpy()))
