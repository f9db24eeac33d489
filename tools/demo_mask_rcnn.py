#!/usr/bin/env python3
"""Overfit the detector assembly (``MaskRCNN``) on a few synthetic patches with rectangular bright regions and report how
well ``predict`` recovers them: best box IoU per ground-truth region, the IoU of the union mask, and box and mask AP50 / AP /
AR from ``evaluation.score_detections`` (per emitter family with ``--from-simulator``).  A functional
demonstration (the pieces are parity-tested one by one), not a benchmark.

    python tools/demo_mask_rcnn.py [--steps 200] [--dtype float32|bfloat16] [--detect] [--from-masks | --from-simulator]

``--from-masks`` trains on instance targets that ``instances_from_masks`` builds on the GPU from ONE binary mask per image
(the union of its rectangles: two that touch become one instance) instead of the per-rectangle targets.  ``--from-simulator`` trains a six-class detector on ``RFISimulator`` samples instead: 8-channel
NHWC planes from ``generate_batch(out="nhwc")``, normalised per sample (``robust_scale``), with one instance per emitter and a class per
emitter family from ``event_instances`` -- images, targets and instance masks never leave the GPU.  ``--detect`` runs ``MaskRCNN.detect`` (inference on the device) too and prints whether both forms agree."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def batch(rng, n, size):
    x = rng.standard_normal((n, size, size, 3)).astype(np.float32) * 0.1
    targets = []
    for i in range(n):
        boxes, masks = [], []
        for _ in range(2):
            w, h = rng.integers(20, 60, 2)
            x1, y1 = rng.integers(0, size - w), rng.integers(0, size - h)
            m = np.zeros((size, size), np.uint8)
            m[y1:y1 + h, x1:x1 + w] = 1
            x[i, y1:y1 + h, x1:x1 + w] += 2.0
            boxes.append([x1, y1, x1 + w, y1 + h]); masks.append(m)
        targets.append({"boxes": np.asarray(boxes, np.float32), "labels": np.ones(2, np.int64), "masks": np.stack(masks)})
    return x, targets


def report(title, detections, targets, num_classes, names):
    """Box and mask AP of `detections` (the list of predict or the device dict of detect) against `targets`."""
    from rfi_toolbox_amd.evaluation import score_detections
    for kind in ("box", "mask"):
        s = score_detections(detections, targets, num_classes=num_classes, kind=kind, class_names=names)
        print(f"{title} {kind:4s} AP50 {s['AP50']:.3f}  AP {s['AP']:.3f}  AR {s['AR']:.3f}")
        if num_classes > 2:
            for name, c in s["per_class"].items():
                if c["n_gt"] or c["n_det"]:
                    print(f"    {name:16s} AP50 {c['AP50']:.3f}  AP {c['AP']:.3f}  AR {c['AR']:.3f}  ({c['n_gt']} emitters, {c['n_det']} detections)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--dtype", default="float32")
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--detect", action="store_true", help="run MaskRCNN.detect too and compare it with predict")
    ap.add_argument("--from-masks", action="store_true", help="build the targets from each image's binary mask by instances_from_masks")
    ap.add_argument("--from-simulator", action="store_true",
                    help="train on RFISimulator samples with one instance per emitter and a class per family (event_instances)")
    a = ap.parse_args()
    if a.from_masks and a.from_simulator:
        ap.error("--from-masks and --from-simulator exclude each other")
    import torch
    from rfi_toolbox_amd.models import MaskRCNN
    torch.manual_seed(0)
    if a.from_simulator:
        from rfi_toolbox_amd.core import EVENT_CLASSES, RFISimulator, event_instances
        from rfi_toolbox_amd.preprocessing import Normalizer
        det = MaskRCNN(len(EVENT_CLASSES), 8, 16, 64, 128, seed=0).set_compute_dtype(a.dtype)
        sim_batch = RFISimulator(128, 128, seed=1).generate_batch(a.images, out="nhwc")
        x = Normalizer("robust_scale", scope="sample").fit_transform(sim_batch.data, out="nhwc", layout="nhwc")
        step_targets = event_instances(sim_batch, min_side=2, max_instances=16)      # (min_side=2: no one-pixel-wide lines)
        targets = step_targets.to_list()
        print(f"emitters per sample: {step_targets.count_host.tolist()} of {step_targets.n_survivors_host.tolist()} two pixels wide or more; "
              f"families: {sorted({EVENT_CLASSES[c] for t in targets for c in t['labels']})}")
    else:
        det = MaskRCNN(2, 3, 16, 64, 128, seed=0).set_compute_dtype(a.dtype)
        x, targets = batch(np.random.default_rng(1), a.images, 128)
        step_targets = targets
    if a.from_masks:
        from rfi_toolbox_amd.components import instances_from_masks
        step_targets = instances_from_masks(np.stack([t["masks"].any(0) for t in targets]))
        targets = step_targets.to_list()                # (what the report below compares against)
        print(f"instances per image from the binary masks: {step_targets.count_host.tolist()}")
    t0 = time.time()
    for s in range(a.steps):
        l = det.train_step(x, step_targets, lr=2e-3, weight_decay=0.0, max_grad_norm=10.0)
        if s % 20 == 0 or s == a.steps - 1:
            print(f"step {s:4d}  " + "  ".join(f"{k[5:] or 'total'} {v:.4f}" for k, v in l.items()), flush=True)
    print(f"{a.steps} steps in {time.time() - t0:.1f} s")
    det.score_thresh = 0.5
    if a.from_simulator:
        x = x.numpy()                                   # (predict takes host images)
    out = det.predict(x)
    from rfi_toolbox_amd.evaluation import match_instances
    box_iou = match_instances(out, targets, kind="box", class_aware=False).numpy()["iou"]       # (n, D, G), zero behind the counts
    for i, (o, t) in enumerate(zip(out, targets)):
        best = box_iou[i, :, :len(t["boxes"])].max(axis=0, initial=0.0)
        gm = t["masks"].any(0)
        mi = (gm & o["rfi_mask"]).sum() / max((gm | o["rfi_mask"]).sum(), 1)
        print(f"image {i}: {len(o['boxes'])} detections, best box IoU per region {[round(float(b), 3) for b in best]}, union-mask IoU {mi:.3f}")
    names = EVENT_CLASSES if a.from_simulator else ("background", "region")
    report("predict:", out, step_targets if a.from_simulator or a.from_masks else targets, det.num_classes, names)
    if a.detect:
        report("detect (device dict):", det.detect(x, out="device"), step_targets if a.from_simulator or a.from_masks else targets,
               det.num_classes, names)
        dev = det.detect(x)
        same = all(len(d["boxes"]) == len(o["boxes"]) and np.array_equal(d["labels"], o["labels"]) for d, o in zip(dev, out))
        if same:
            db = max((float(np.abs(d["boxes"] - o["boxes"]).max()) for d, o in zip(dev, out) if len(o["boxes"])), default=0.0)
            ds = max((float(np.abs(d["scores"] - o["scores"]).max()) for d, o in zip(dev, out) if len(o["boxes"])), default=0.0)
            px = sum(int((d["rfi_mask"] != o["rfi_mask"]).sum()) for d, o in zip(dev, out))
            print(f"detect agrees with predict: same detections and labels, max |d box| {db:.2e} px, max |d score| {ds:.2e}, "
                  f"{px} union-mask pixels differ")
        else:
            print("detect DISAGREES with predict:", [(len(d["boxes"]), len(o["boxes"])) for d, o in zip(dev, out)])


if __name__ == "__main__":
    main()
