#!/usr/bin/env python3
"""Time flag_statistics and compute_ffi on device-resident complex64 arrays with 10 % flags (evaluation/statistics.py).

    python tools/bench_flag_statistics.py [--log2 24 26 28] [--iters 10] [--warmup 3] [--numpy]

Per call: device time between HIP events recorded on the library's stream (rfi_timer_start / rfi_timer_stop) and
host wall time.  Traffic is counted from the algorithm: pass 1 reads z (8 B) and the flag (1 B) and stores |z|
(4 B); each later full pass (two median digits, the deviation pass with the first MAD digit, two MAD digits) reads
|z| and the flag (5 B).  Effective bytes/s is that traffic over the device time, next to the 6.3 TB/s copy rate.
--numpy also times a NumPy computation of the same quantities on the host at the smallest size.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rfi_toolbox_amd._lib import check, lib                                 # noqa: E402
from rfi_toolbox_amd.evaluation import compute_ffi, flag_statistics         # noqa: E402
from rfi_toolbox_amd.runtime import Context                                 # noqa: E402

COPY_RATE = 6.3e12
PASSES = 6                       # full-array passes of a complex64 call with medians
BYTES_PER_ELEM = 8 + 1 + 4 + 5 * (PASSES - 1)


def timed(ctx, fn, iters):
    check(lib.rfi_timer_start(ctx.handle))
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    wall = (time.perf_counter() - t0) / iters
    ms = C.c_float()
    check(lib.rfi_timer_stop(ctx.handle, C.byref(ms)))
    return ms.value / iters, wall * 1e3


def numpy_ffi(z, f):
    a = np.abs(z)
    out = {}
    for tag, v in (("all", a.ravel()), ("clean", a[~f])):
        med = np.median(v)
        out[tag] = (float(np.mean(v)), float(np.std(v)), float(med), float(np.median(np.abs(v - med))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[24, 26, 28])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--numpy", action="store_true")
    args = ap.parse_args()
    ctx = Context.get(0)
    rows = []
    for lg in args.log2:
        n = 1 << lg
        g = torch.Generator(device="cuda").manual_seed(lg)
        z = torch.randn(n, dtype=torch.complex64, device="cuda", generator=g)
        f = torch.rand(n, device="cuda", generator=g) < 0.1
        torch.cuda.synchronize()
        row = {"log2_n": lg, "n": n, "full_passes": PASSES, "bytes_per_call": n * BYTES_PER_ELEM}
        for name, fn in (("flag_statistics", lambda: flag_statistics(z, f)), ("compute_ffi", lambda: compute_ffi(z, f))):
            for _ in range(args.warmup):
                fn()
            dev_ms, wall_ms = timed(ctx, fn, args.iters)
            row[f"{name}_ms"] = round(dev_ms, 4)
            row[f"{name}_wall_ms"] = round(wall_ms, 4)
        row["effective_TBps"] = round(row["bytes_per_call"] / (row["flag_statistics_ms"] * 1e-3) / 1e12, 3)
        row["share_of_copy_rate"] = round(row["effective_TBps"] * 1e12 / COPY_RATE, 3)
        if args.numpy and lg == min(args.log2):
            zh, fh = z.cpu().numpy(), f.cpu().numpy()
            t0 = time.perf_counter()
            numpy_ffi(zh, fh)
            row["numpy_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del z, f
        torch.cuda.empty_cache()
    return rows


if __name__ == "__main__":
    main()
