#!/usr/bin/env python3
"""Detector inference: ``MaskRCNN.detect`` (every stage on the device) against ``MaskRCNN.predict`` (the host-array form) in
one process.

    python tools/bench_detect.py [--images 64] [--size 128] [--warmup 1] [--min-seconds 1.0] [--dtypes float32 bfloat16]

Workload: the benched detector shape -- ResNet-50-FPN widths (64, 256, 1024), `images` x size x size x 3 (default 64 x 128 x
128), 2 classes, untrained weights, score_thresh 0 so that every image carries max_det detections (the full mask-branch
and paste work).  Per compute dtype the three variants -- predict, detect with instance masks, detect with the union
only -- are warmed up and then timed in alternation: a host clock around whole calls (each ends in the download of its
results, which waits for the stream), rounds repeated until the detect variants have each run for more than
``--min-seconds``.  Then one profiled detect call gives the times of the new kernels (labelled launches of the library's
profile).  Prints one JSON line per dtype: ms per call of each variant, bytes downloaded per call, the kernel times."""
import argparse
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NEW_KERNELS = ("rois_from_boxes", "detect_candidates", "detect_select", "mask_paste")


def downloaded_bytes(n, h, w, max_det, instance_masks):
    """What a detect call brings down: counts, boxes, scores, labels, the union masks and (if asked for) the instance masks."""
    return n * 4 + n * max_det * (16 + 4 + 4) + n * h * w + (n * max_det * h * w if instance_masks else 0)


def kernel_times(det, x):
    ctx = det.backbone.ctx
    ctx.synchronize()
    ctx.profile_reset()
    ctx.profile(True)
    det.detect(x)
    ctx.synchronize()
    ctx.profile(False)
    path = os.path.join(tempfile.mkdtemp(), "detect_profile.csv")
    ctx.profile_dump(path)
    ctx.profile_reset()
    ms = dict.fromkeys(NEW_KERNELS, 0.0)
    total = 0.0
    with open(path) as f:
        for r in csv.DictReader(f):
            total += float(r["ms"])
            if r["label"] in ms:
                ms[r["label"]] += float(r["ms"])
    out = {f"{k}_ms": round(v, 4) for k, v in ms.items()}
    out["all_kernels_ms"] = round(total, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--dtypes", nargs="+", default=["float32", "bfloat16"])
    a = ap.parse_args()
    import torch
    from rfi_toolbox_amd.models import MaskRCNN
    n, s = a.images, a.size
    x = (np.random.default_rng(0).standard_normal((n, s, s, 3)) * 0.5).astype(np.float32)
    for dt in a.dtypes:
        torch.manual_seed(0)
        det = MaskRCNN(2, 3, 64, 256, 1024, seed=0).set_compute_dtype(dt)
        det.score_thresh = 0.0
        variants = {"predict": lambda: det.predict(x), "detect": lambda: det.detect(x),
                    "detect_union_only": lambda: det.detect(x, instance_masks=False)}
        found = 0
        for _ in range(max(a.warmup, 1)):
            for fn in variants.values():
                found = sum(len(o["boxes"]) for o in fn())
        spent, calls = dict.fromkeys(variants, 0.0), 0
        while calls == 0 or min(spent["detect"], spent["detect_union_only"]) <= a.min_seconds:
            for name, fn in variants.items():
                t0 = time.perf_counter()
                fn()                                  # (returns host arrays: the call has waited for the device)
                spent[name] += time.perf_counter() - t0
            calls += 1
        r = {"dtype": dt, "workload": f"MaskRCNN(2, 3, 64, 256, 1024), {n} x {s} x {s} x 3, score_thresh 0", "calls": calls,
             "detections": found}
        for name in variants:
            r[f"{name}_ms"] = round(spent[name] / calls * 1e3, 3)
        r["detect_speedup"] = round(spent["predict"] / spent["detect"], 2)
        r["detect_union_only_speedup"] = round(spent["predict"] / spent["detect_union_only"], 2)
        r["detect_downloaded_bytes"] = downloaded_bytes(n, s, s, det.max_det, True)
        r["detect_union_only_downloaded_bytes"] = downloaded_bytes(n, s, s, det.max_det, False)
        r["kernels"] = kernel_times(det, x)
        print(json.dumps(r), flush=True)
        del det, variants


if __name__ == "__main__":
    main()
