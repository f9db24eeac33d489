#!/usr/bin/env python3
"""Time the per-family segmentation path on batches resident on the device: targets from the simulator, the K-channel
loss pair and a whole training step at K = 5 against K = 1 of the same width.

    python tools/bench_family_flags.py [--window 1.0] [--repeats 5] [--features 32]

Two batches: 64 x 128 x 128 and 8 x 512 x 512.  Per batch, in the same process and on the same batch:
  family_masks     core.family_masks(batch): one kernel, (n, T, F) class-bit bytes
  instances_or     the route it replaces: event_instances(batch, max_instances=256) masks, downloaded and ORed by label on
                   the host
  loss_net_k5      the loss pair (class_loss_reduce + finish, class_loss_bwd) with the smallest network around it:
                   forward_backward of UNet(8, 5, 4, depth=1), class-bit labels, bce_class_dice.  An upper bound on the pair
                   (the one-level, 4-feature network and the head are in it); read it against ...
  loss_net_k1      ... the same model with one output channel, a label map and bce_dice (loss_reduce, loss_bwd)
  step_k5, step_k1 train_step_async of UNet(8, K, F) with class-bit labels and bce_class_dice (K = 5) or a label map and
                   bce_dice (K = 1), default compute mode
Figures as tools/bench_sim_instances.py takes them: after a warm-up call, device events around the whole call, call after
call for --window seconds and at least --repeats calls; ms is the median call, spread its (90th - 10th percentile) /
median.  One JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BATCHES = {"64x128": (64, 128), "8x512": (8, 512)}


def timed(ctx, fn, window, repeats):
    from rfi_toolbox_amd._lib import check, lib
    fn()
    ctx.synchronize()
    calls, t0 = [], time.perf_counter()
    while time.perf_counter() - t0 < window or len(calls) < repeats:
        check(lib.rfi_timer_start(ctx.handle))
        res = fn()
        ms = C.c_float()
        check(lib.rfi_timer_stop(ctx.handle, C.byref(ms)))
        del res
        calls.append(ms.value)
    calls = np.sort(np.asarray(calls))
    med = float(np.median(calls))
    return {"ms": round(med, 4), "spread": round(float(calls[int(0.9 * (len(calls) - 1))] - calls[int(0.1 * (len(calls) - 1))]) / med, 3),
            "calls": len(calls)}


def instances_or(batch):
    from rfi_toolbox_amd.core import event_instances
    tg = event_instances(batch, max_instances=256)
    masks, labels, base = tg.masks.numpy(), tg.labels.numpy(), tg.base.numpy()
    out = np.zeros(tuple(batch.mask.shape), np.uint8)
    for i, k in enumerate(tg.count_host):
        for j in range(int(k)):
            out[i] |= masks[base[i] + j] << np.uint8(labels[i, j] - 1)
    return out


def run(name, window, repeats, features):
    from rfi_toolbox_amd._lib import Hyper
    from rfi_toolbox_amd.core import RFISimulator, family_masks
    from rfi_toolbox_amd.models import UNet
    n, size = BATCHES[name]
    sim = RFISimulator(size, size, seed=0, device=0)
    batch = sim.generate_batch(n, out="nhwc")
    ctx = batch.mask.ctx
    bits = family_masks(batch)
    assert np.array_equal(bits.numpy(), instances_or(batch))
    res = {"family_masks": timed(ctx, lambda: family_masks(batch), window, repeats),
           "instances_or": timed(ctx, lambda: instances_or(batch), min(window, 0.2), 2)}
    hp = Hyper(1e-4, 0.9, 0.999, 1e-8, 1e-5, 1.0)
    for K in (5, 1):
        labels = bits if K == 5 else batch.mask
        small = UNet(8, K, 4, depth=1, device=0).train()
        big = UNet(8, K, features, device=0).train()
        if K == 5:
            small.set_targets("class_bits").set_loss("bce_class_dice")
            big.set_targets("class_bits").set_loss("bce_class_dice")
        res[f"loss_net_k{K}"] = timed(ctx, lambda: small.forward_backward(batch.data, labels), window, repeats)
        res[f"step_k{K}"] = timed(ctx, lambda: big.train_step_async(batch.data.ptr, labels.ptr, n, size, size, hp), window, repeats)
        del small, big
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--features", type=int, default=32)
    a = ap.parse_args()
    out = {"tool": "bench_family_flags", "features": a.features}
    for name in BATCHES:
        out[name] = run(name, a.window, a.repeats, a.features)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
