#!/usr/bin/env python3
"""Time the losses with an ignore bit and positive weights against the plain ones, on batches resident on the device, and
the label tiling against a device copy.

    python tools/bench_masked_loss.py [--rounds 7] [--calls 5] [--features 32]

Two batches: 64 x 128 x 128 and 8 x 512 x 512; K = 1 (a label map, bce_dice) and K = 5 (class bits, bce_class_dice).  Per
batch and K, four variants of the SAME two models, switched between the calls:
  plain      no switch, no weights: loss_reduce / loss_bwd (K = 1) or class_loss_reduce / class_loss_bwd (K = 5)
  ignore0    set_ignore(True), no label has bit 7: masked_loss_reduce / _finish / _bwd on the same bytes
  ignore30   set_ignore(True), bit 7 set under 30 % of the pixels
  weights    set_pos_weight, no switch
and two figures per variant:
  loss_net   the loss turn-around (reduce + finish + backward) with the smallest network around it: forward_backward of
             UNet(8, K, 4, depth=1).  An upper bound on the three kernels; the variants differ in nothing else
  step       train_step_async of UNet(8, K, F), default compute mode
The variants alternate inside one process: a round times every variant for --calls calls (device events around each call,
after one warm-up call), and there are --rounds rounds.  ms is the median of the round medians, spread their (max - min) /
median: a gap between two variants smaller than the spreads is not a difference.
  tile_labels   8 baselines of 1024 x 1024 at patch 128, stride 96, with a per-polarisation invalid map, against
                rfi_memcpy device-to-device of as many bytes as it writes
One JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BATCHES = {"64x128": (64, 128), "8x512": (8, 512)}
VARIANTS = ("plain", "ignore0", "ignore30", "weights")
WEIGHTS = {1: [4.0], 5: [0.5, 50.0, 1.0, 7.0, 20.0]}


def one_call(ctx, fn):
    from rfi_toolbox_amd._lib import check, lib
    check(lib.rfi_timer_start(ctx.handle))
    fn()
    ms = C.c_float()
    check(lib.rfi_timer_stop(ctx.handle, C.byref(ms)))
    return ms.value


def alternate(ctx, runs, rounds, calls):
    """runs: name -> (setup, fn).  -> name -> {"ms", "spread", "rounds"}"""
    med = {k: [] for k in runs}
    for _ in range(rounds):
        for name, (setup, fn) in runs.items():
            setup()
            fn()
            ctx.synchronize()
            med[name].append(float(np.median([one_call(ctx, fn) for _ in range(calls)])))
    out = {}
    for name, v in med.items():
        m = float(np.median(v))
        out[name] = {"ms": round(m, 4), "spread": round((max(v) - min(v)) / m, 3), "rounds": len(v)}
    return out


def configure(model, variant, K):
    model.set_pos_weight(None).set_ignore(variant.startswith("ignore"))
    if variant == "weights":
        model.set_pos_weight(WEIGHTS[K])


def run(name, rounds, calls, features):
    from rfi_toolbox_amd._lib import Hyper
    from rfi_toolbox_amd.core import RFISimulator, family_masks
    from rfi_toolbox_amd.models import UNet
    n, size = BATCHES[name]
    sim = RFISimulator(size, size, seed=0, device=0)
    batch = sim.generate_batch(n, out="nhwc")
    ctx = batch.mask.ctx
    hp = Hyper(1e-4, 0.9, 0.999, 1e-8, 1e-5, 1.0)
    ignored = np.random.default_rng(0).random((n, size, size)) < 0.3
    res = {}
    for K in (1, 5):
        plain = (family_masks(batch) if K == 5 else batch.mask)
        holes = ctx.to_device(plain.numpy().astype(np.uint8) | (ignored.astype(np.uint8) << 7).astype(np.uint8))
        small = UNet(8, K, 4, depth=1, device=0).train()
        big = UNet(8, K, features, device=0).train()
        if K == 5:
            small.set_targets("class_bits").set_loss("bce_class_dice")
            big.set_targets("class_bits").set_loss("bce_class_dice")
        labels = {v: (holes if v == "ignore30" else plain) for v in VARIANTS}
        loss = {v: ((lambda v=v: configure(small, v, K)), (lambda v=v: small.forward_backward(batch.data, labels[v]))) for v in VARIANTS}
        step = {v: ((lambda v=v: configure(big, v, K)),
                    (lambda v=v: big.train_step_async(batch.data.ptr, labels[v].ptr, n, size, size, hp))) for v in VARIANTS}
        res[f"loss_net_k{K}"] = alternate(ctx, loss, rounds, calls)
        res[f"step_k{K}"] = alternate(ctx, step, rounds, calls)
        del small, big
    return res


def tile_labels_run(rounds, calls):
    from rfi_toolbox_amd._lib import DEVICE, check, lib
    from rfi_toolbox_amd.inference import tile_labels
    from rfi_toolbox_amd.runtime import Context
    ctx = Context.get(0)
    rng = np.random.default_rng(1)
    B, S = 8, 1024
    lab = ctx.to_device(rng.integers(0, 32, (B, S, S), dtype=np.uint8))
    inv = ctx.to_device((rng.random((B, 4, S, S)) < 0.1).astype(np.uint8))
    out = tile_labels(lab, 128, stride=96, invalid=inv)
    dst = ctx.empty(out.shape, np.uint8)
    runs = {"tile_labels": ((lambda: None), (lambda: tile_labels(lab, 128, stride=96, invalid=inv))),
            "device_copy": ((lambda: None), (lambda: check(lib.rfi_memcpy(ctx.handle, C.c_void_p(dst.ptr), DEVICE, C.c_void_p(out.ptr), DEVICE,
                                                                             out.nbytes))))}
    res = alternate(ctx, runs, rounds, calls)
    res["tiles"] = int(out.shape[0])
    res["bytes_out"] = int(out.nbytes)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--features", type=int, default=32)
    a = ap.parse_args()
    out = {"tool": "bench_masked_loss", "features": a.features}
    for name in BATCHES:
        out[name] = run(name, a.rounds, a.calls, a.features)
    out["tile_labels_8x1024"] = tile_labels_run(a.rounds, a.calls)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
