#!/usr/bin/env python3
"""Time the all-thresholds confusion sweep (evaluation.threshold_sweep, csrc/threshold_sweep.hip) on device-resident
inputs: 64 x 1024 x 1024 float32 scores with a uint8 truth mask, K = 99 thresholds (0.01 ... 0.99).

    python tools/bench_threshold_sweep.py [--batch 64] [--size 1024] [--k 99] [--window 1.0] [--repeats 5]

Every figure is taken after a warm-up call, from device events on the library's stream ending in a synchronise
(rfi_timer_start / rfi_timer_stop) around the whole call; a figure is the median over --repeats windows of at least
--window / --repeats seconds each, its spread (max - min) / median.

  sweep_bimodal  probabilities as a trained flagger gives them: 95 % below the first threshold, 4 % above the last, 1 % between
  sweep_uniform  probabilities uniform in [0, 1): every element takes the binary search and an LDS atomic
  sweep_logits   kind="logits" on the logits of the bimodal case (adds one expf and one division per element)
Yardsticks that exist without the sweep, same process, same arrays:
  confusion      ONE confusion_counts(float32 pred, uint8 true): the same 5 B per element of HBM traffic, no histogram
  k_loop         what the sweep replaces: K x (rfi_threshold_logits -> confusion_counts(uint8 mask, uint8 true))
One JSON line: ms and spread of each, the sweep's effective GB/s (5 B per element), its ratio to the single pass, the
ratio of the K-call loop to it, and uniform / bimodal (what is left of the contention on the middle bins).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rfi_toolbox_amd._lib import check, lib                                  # noqa: E402
from rfi_toolbox_amd.evaluation import confusion_counts, threshold_sweep     # noqa: E402
from rfi_toolbox_amd.runtime import Context                                  # noqa: E402


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
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--k", type=int, default=99)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    ctx = Context.get(0)
    shape = (args.batch, args.size, args.size)
    n = int(np.prod(shape))
    thr = (np.arange(1, args.k + 1, dtype=np.float32) / np.float32(args.k + 1))
    rng = np.random.default_rng(0)
    u = rng.random(n, dtype=np.float32)
    v = rng.random(n, dtype=np.float32)
    lo, hi = float(thr[0]), float(thr[-1])
    bimodal = np.where(u < 0.95, v * lo, np.where(u < 0.99, hi + (1 - hi) * v + np.float32(1e-6), v)).astype(np.float32)
    logits = np.where(u < 0.95, -12 + 7 * v, np.where(u < 0.99, 5 + 7 * v, -4.5 + 9 * v)).astype(np.float32)
    truth = ctx.to_device((rng.random(n, dtype=np.float32) < 0.05).astype(np.uint8).reshape(shape))
    d_bimodal, d_uniform = ctx.to_device(bimodal.reshape(shape)), ctx.to_device(v.reshape(shape))
    d_logits, mask = ctx.to_device(logits.reshape(shape)), ctx.empty(shape, np.uint8)
    middle = float(((bimodal > lo) & ~(bimodal > hi)).mean())
    del u, bimodal, logits

    def k_loop():
        for t in thr:
            check(lib.rfi_threshold_logits(ctx.handle, C.c_void_p(d_logits.ptr), n, float(t), C.c_void_p(mask.ptr)))
            confusion_counts(mask, truth)

    cases = [("sweep_bimodal", lambda: threshold_sweep(d_bimodal, truth, thr)),
             ("sweep_uniform", lambda: threshold_sweep(d_uniform, truth, thr)),
             ("sweep_logits", lambda: threshold_sweep(d_logits, truth, thr, kind="logits")),
             ("confusion", lambda: confusion_counts(d_bimodal, truth)),
             ("k_loop", k_loop)]
    row = {"shape": list(shape), "k": int(thr.size), "bytes_per_pass": 5 * n, "bimodal_middle_share": round(middle, 4)}
    ms = {}
    for name, fn in cases:
        ms[name], spread = median_of(ctx, fn, args.window, args.repeats)
        row[name + "_ms"], row[name + "_spread"] = round(ms[name], 4), round(spread, 3)
    for name in ("sweep_bimodal", "sweep_uniform", "sweep_logits", "confusion"):
        row[name + "_GBps"] = round(5 * n / (ms[name] * 1e-3) / 1e9, 1)
    row.update(sweep_over_confusion=round(ms["sweep_bimodal"] / ms["confusion"], 2),
               k_loop_over_sweep=round(ms["k_loop"] / ms["sweep_logits"], 1),
               uniform_over_bimodal=round(ms["sweep_uniform"] / ms["sweep_bimodal"], 2), device=ctx.device_name())
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    main()
