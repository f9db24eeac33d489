#!/usr/bin/env python3
"""A flagger that says which kind of RFI it sees: train a 5-output U-Net on the simulator's per-family targets, score it
per family, flag a larger observation.

    python tools/demo_family_flags.py [--steps 300] [--batch 16] [--features 16] [--seed 0]

RFISimulator(128, 128) batches -> Normalizer("robust_scale", "sample") -> UNet(8, 5, F) with class-bit targets
(core.family_masks) and the bce_class_dice loss -> evaluate_rfi_model on held-out batches (per-family IoU table) ->
predict_flags on a 256 x 256 batch, compared per family with its own family_masks.  Everything stays on the device between
the generator and the optimiser step."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--features", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    import torch
    from rfi_toolbox_amd import EVENT_CLASSES, family_masks
    from rfi_toolbox_amd.class_labels import unpack_class_bits
    from rfi_toolbox_amd.core import RFISimulator
    from rfi_toolbox_amd.inference import predict_flags
    from rfi_toolbox_amd.models import UNet
    from rfi_toolbox_amd.preprocessing import Normalizer
    from rfi_toolbox_amd.training import evaluate_rfi_model

    names = list(EVENT_CLASSES[1:])
    K = len(names)
    torch.manual_seed(a.seed)
    sim = RFISimulator(128, 128, seed=a.seed, device=0)
    nz = Normalizer("robust_scale", scope="sample")
    model = UNet(8, K, a.features, device=0).set_targets("class_bits").set_loss("bce_class_dice").train()

    def batch_of(n):
        b = sim.generate_batch(n, out="nhwc")
        return nz.fit_transform(b.data, out="nhwc", layout="nhwc"), family_masks(b)

    for step in range(1, a.steps + 1):
        x, y = batch_of(a.batch)
        loss = model.train_step(x, y, lr=1e-3)
        if step == 1 or step % 50 == 0 or step == a.steps:
            print(f"step {step:4d}  loss {loss:.4f}", flush=True)

    # held-out batches, per family
    xs, ys = zip(*[(x.numpy(), y.numpy()) for x, y in (batch_of(a.batch) for _ in range(4))])
    res = evaluate_rfi_model(model, (np.concatenate(xs), np.concatenate(ys)), batch_size=a.batch, class_names=names)
    px = unpack_class_bits(np.concatenate(ys), K).sum(axis=(0, 2, 3))
    print(f"\n{'family':<18}{'pixels':>9}{'iou':>8}{'precision':>11}{'recall':>8}{'f1':>8}")
    for c, n_px in zip(res["per_class"], px):
        print(f"{c['name']:<18}{int(n_px):>9}{c['iou']:>8.3f}{c['precision']:>11.3f}{c['recall']:>8.3f}{c['f1']:>8.3f}")
    m = res["macro"]
    print(f"{'macro':<18}{'':>9}{m['iou']:>8.3f}{m['precision']:>11.3f}{m['recall']:>8.3f}{m['f1']:>8.3f}")

    # a larger observation through the tiler: (B, K, T, F) flags
    big = RFISimulator(256, 256, seed=a.seed + 1, device=0).generate_batch(2, out="complex64")
    flags = predict_flags(model, big.data, patch_size=128, stride=96, normalizer=nz)
    truth = unpack_class_bits(family_masks(big).numpy(), K)
    assert flags.shape == truth.shape == (2, K, 256, 256)
    print("\npredict_flags on 2 x 256 x 256 (patch 128, stride 96):")
    for k, name in enumerate(names):
        inter, union = int((flags[:, k] & truth[:, k]).sum()), int((flags[:, k] | truth[:, k]).sum())
        print(f"{name:<18}{int(truth[:, k].sum()):>9} flagged {int(flags[:, k].sum()):>7}  iou {inter / max(union, 1):.3f}")


if __name__ == "__main__":
    main()
