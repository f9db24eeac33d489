"""TEST INFRASTRUCTURE ONLY -- the whole-step cases of a K-channel U-Net on class-bit labels (test_gpu_unet_family_step.py;
test_family_step_cases_host.py pins them without a GPU).

The seeds have the ``relu_margin`` property of tests/unet_cases.py: in the float64 oracle no BatchNorm output lies within
1e-5 of the activation threshold, for either loss, so the comparison measures arithmetic and not which side of the
threshold a pre-activation lands on (``python tests/family_step_cases.py`` prints the margin of seeds 10 .. 29).  Seed 13
of the width-16 case has a margin of 1e-6: on an MI355X the default arithmetic landed on the other side of one threshold
there and every gradient tensor below it moved by 2e-2 relative, while float32_mfma and float32_planes stayed at the
oracle's own noise."""
from collections import namedtuple

import numpy as np
import torch

Case = namedtuple("Case", "id in_ch K feat depth n h w seed")
CASES = (Case("in8_k5_f4_d2_8x12", 8, 5, 4, 2, 2, 8, 12, 11), Case("in3_k2_f8_d4_16x16", 3, 2, 8, 4, 2, 16, 16, 12),
         # a width of 16: the plane flows keep the gradient the head sends down as a bfloat16 tensor, which the head
         # backward used to write for one output channel only
         Case("in8_k3_f16_d2_16x24", 8, 3, 16, 2, 2, 16, 24, 23))
LOSSES = ("bce_dice", "bce_class_dice")
MARGIN = 1e-5


def class_dice_loss(logits, target, smooth=1.0):
    """bce_class_dice on (N, K, H, W): the BCE mean over all elements + the mean over the classes of each class's own dice
    term, its three sums taken over the batch"""
    y = target.to(logits.dtype)
    bce = (torch.clamp(logits, min=0) - logits * y + torch.log1p(torch.exp(-logits.abs()))).mean()
    p = torch.sigmoid(logits)
    inter = (p * y).sum(dim=(0, 2, 3))
    dice = 1 - (2.0 * inter + smooth) / (p.sum(dim=(0, 2, 3)) + y.sum(dim=(0, 2, 3)) + smooth)
    return bce + dice.mean()


LOSS_FN = {"bce_dice": None, "bce_class_dice": class_dice_loss}


def inputs(c):
    """x (n, h, w, in_ch) float32, label bytes (n, h, w) uint8 over all 256 values"""
    g = torch.Generator().manual_seed(c.seed + 100)
    x = torch.randn(c.n, c.h, c.w, c.in_ch, generator=g)
    y = torch.randint(0, 256, (c.n, c.h, c.w), generator=g, dtype=torch.int64).to(torch.uint8)
    return x, y


def targets(y, K):
    """(n, K, h, w) float32 from label bytes"""
    b = y.numpy()
    return torch.from_numpy(np.stack([(b >> k) & 1 for k in range(K)], axis=1).astype(np.float32))


def relu_margin(c):
    """min |BatchNorm output| of the float64 oracle's train-mode forward (the forward does not depend on the loss)"""
    import unet_cases as U
    from oracle import unet_ref
    st = unet_ref.init_state(c.in_ch, c.K, c.feat, c.depth, seed=c.seed)
    x, y = inputs(c)
    st64, tape = U.to64(st), {}
    unet_ref.loss_and_grads(st64, unet_ref.nhwc_to_nchw(x).double(), targets(y, c.K).double(), tape=tape)
    margin = float("inf")
    for k, out in tape.items():
        if not k.endswith(".out") or ".up." in k:
            continue
        prefix, ci = k[:-4].rsplit(".", 1)
        bn = f"{prefix}.{int(ci) + 1}"
        z = (out.detach() - tape[f"{bn}.mean"][None, :, None, None]) * torch.rsqrt(tape[f"{bn}.var"] + unet_ref.BN_EPS)[None, :, None, None]
        z = z * st64[f"{bn}.weight"][None, :, None, None] + st64[f"{bn}.bias"][None, :, None, None]
        margin = min(margin, float(z.abs().min()))
    return margin


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    for c in CASES:
        for s in range(10, 30):
            print(c.id, "seed", s, f"margin={relu_margin(c._replace(seed=s)):.2e}", flush=True)
