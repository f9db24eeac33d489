#!/usr/bin/env python3
"""Time the on-device training augmentation (training.Augmenter, csrc/augment.hip) on device-resident batches of
64 x 128 x 128 x C float32 with their masks, C = 3 and 8.

    python tools/bench_augment.py [--batch 64] [--size 128] [--window 0.5] [--repeats 5]

Every figure is taken after a warm-up call, from device events on the library's stream ending in a synchronise
(rfi_timer_start / rfi_timer_stop); a figure is the median over --repeats windows of at least --window / --repeats
seconds each, its spread (max - min) / median.

  augment  rfi_augment_batch with the reference's defaults (about a quarter of the samples are flip-only copies, the
           others bilinear gathers).  Bytes the algorithm must move: one read and one write of images and masks.
  copy     yardstick taken in the same process: a device-to-device rfi_memcpy moving the same number of bytes.
  step     one train_step of UNet(C, 1, 32) on the same batch (device-resident, float32 default arithmetic).
One JSON line per channel count: ms, effective GB/s, the ratio to the copy, and the share of a training step.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rfi_toolbox_amd._lib import DEVICE, check, lib      # noqa: E402
from rfi_toolbox_amd.models import UNet                  # noqa: E402
from rfi_toolbox_amd.runtime import Context              # noqa: E402
from rfi_toolbox_amd.training import Augmenter           # noqa: E402


def timed(ctx, fn, window):
    """mean device ms per call of fn over >= window seconds (events on the stream, the stop synchronises)"""
    fn()
    ctx.synchronize()
    calls, total_ms, t0 = 0, 0.0, time.perf_counter()
    while time.perf_counter() - t0 < window or calls == 0:
        check(lib.rfi_timer_start(ctx.handle))
        fn()
        ms = C.c_float()
        check(lib.rfi_timer_stop(ctx.handle, C.byref(ms)))
        total_ms += ms.value
        calls += 1
    return total_ms / calls


def median_of(ctx, fn, window, repeats):
    ms = [timed(ctx, fn, window / repeats) for _ in range(repeats)]
    med = float(np.median(ms))
    return med, (max(ms) - min(ms)) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    ctx = Context.get(0)
    n, s = args.batch, args.size
    rng = np.random.default_rng(0)
    rows = []
    for c in (3, 8):
        x = ctx.to_device((rng.standard_normal((n, s, s, c)) * 2).astype(np.float32))
        y = ctx.to_device((rng.random((n, s, s)) < 0.3).astype(np.uint8))
        xo, yo = ctx.empty(x.shape, np.float32), ctx.empty(y.shape, np.uint8)
        aug = Augmenter(seed=1)
        cfg = aug._config()
        calls = [0]

        def augment():
            calls[0] += 1
            check(lib.rfi_augment_batch(ctx.handle, C.c_void_p(x.ptr), DEVICE, C.c_void_p(y.ptr), DEVICE, n, s, s, c,
                                        C.byref(cfg), calls[0], C.c_void_p(xo.ptr), C.c_void_p(yo.ptr)))

        half = x.nbytes + y.nbytes                       # the kernel reads `half` bytes and writes `half` bytes
        a, b = ctx.empty((half,), np.uint8), ctx.empty((half,), np.uint8)
        a.zero_()
        copy = lambda: check(lib.rfi_memcpy(ctx.handle, C.c_void_p(b.ptr), DEVICE, C.c_void_p(a.ptr), DEVICE, half))   # noqa: E731
        model = UNet(c, 1, 32)
        step = lambda: model.train_step(xo, yo)          # noqa: E731
        aug_ms, aug_spread = median_of(ctx, augment, args.window, args.repeats)
        copy_ms, copy_spread = median_of(ctx, copy, args.window, args.repeats)
        step_ms, step_spread = median_of(ctx, step, 2 * args.window, args.repeats)
        gates, _ = aug.params(n, s, s, call=1)
        row = {"shape": [n, s, s, c], "bytes_moved": 2 * half,
               "flip_only_share": round(float(((gates[:, 2] == 0) & (gates[:, 3] == 0)).mean()), 3),
               "augment_ms": round(aug_ms, 4), "augment_GBps": round(2 * half / (aug_ms * 1e-3) / 1e9, 1),
               "augment_spread": round(aug_spread, 3),
               "copy_ms": round(copy_ms, 4), "copy_GBps": round(2 * half / (copy_ms * 1e-3) / 1e9, 1),
               "copy_spread": round(copy_spread, 3), "augment_over_copy": round(aug_ms / copy_ms, 2),
               "train_step_ms": round(step_ms, 3), "train_step_spread": round(step_spread, 3),
               "augment_share_of_step": round(aug_ms / step_ms, 4), "device": ctx.device_name()}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del model, a, b, x, y, xo, yo
    return rows


if __name__ == "__main__":
    main()
