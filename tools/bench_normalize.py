#!/usr/bin/env python3
"""Time the on-device input normalisation (preprocessing.Normalizer, csrc/dataset_norm.hip) on 16 simulator samples of
1024 x 1024 complex128 (1 GiB in HBM), per method and scope.

    python tools/bench_normalize.py [--samples 16] [--size 1024] [--window 0.5] [--host]

Every figure is taken after a warm-up call, from device events on the library's stream ending in a synchronise
(rfi_timer_start / rfi_timer_stop), over a window of at least --window seconds.

  fit     Normalizer.fit on the DeviceArray (statistics call + the host arithmetic on its scalars).  Bytes the algorithm
          must move: one read of the source per pass -- 2 passes (moments, fused with the first two radix digits) for
          global_min_max / standardize, 6 (one per 11-bit digit of fp64) for robust_scale.
  apply   rfi_norm_apply into a preallocated (n, T, F, 8) float32 buffer: one read of the source + one float32 write.
  memcpy  yardstick taken in the same run: a device-to-device rfi_memcpy moving the same number of bytes as apply
          (a copy of B bytes moves 2 B), repeated; its spread is (max - min) / median over the repeats.
  --host  also times the route this replaces: device -> host copy, NumPy on 16 threads (one sample per task), host ->
          device copy of the float32 result.
One JSON line per (method, scope), then a summary line.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rfi_toolbox_amd._lib import C128, DEVICE, NORM_NCHW, NORM_NHWC, check, lib      # noqa: E402
from rfi_toolbox_amd.core import RFISimulator                                        # noqa: E402
from rfi_toolbox_amd.preprocessing import Normalizer                                 # noqa: E402
from rfi_toolbox_amd.runtime import Context                                          # noqa: E402

METHODS = ("global_min_max", "standardize", "robust_scale")


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
    return total_ms / calls, calls


def host_params(v, method, scope):
    if method == "global_min_max":
        lo, hi = v.min(), v.max()
        return (lo, hi - lo) if hi > lo else None
    if method == "standardize":
        sd = v.std()
        return v.mean(), (sd + 1e-8 if scope == "dataset" else (sd if sd > 0 else 1.0))
    q25, q75 = np.percentile(v, (25, 75))
    return np.median(v), (q75 - q25 + 1e-8 if scope == "dataset" else (q75 - q25 if q75 - q25 >= 10 * np.finfo(float).eps else 1.0))


def host_route(ctx, data, method, scope, out_dev):
    """device -> host, NumPy on 16 threads, host -> device; returns wall seconds"""
    t0 = time.perf_counter()
    z = data.numpy()
    n = z.shape[0]
    x = z.view(np.float64).reshape(n, 4, z.shape[2], z.shape[3], 2)
    pool = ThreadPoolExecutor(16)
    pair = host_params(x.ravel(), method, scope) if scope == "dataset" else None
    out = np.empty((n, z.shape[2], z.shape[3], 8), dtype=np.float32)

    def one(i):
        p = pair if scope == "dataset" else host_params(x[i].ravel(), method, scope)
        s = x[i].transpose(1, 2, 0, 3).reshape(z.shape[2], z.shape[3], 8)
        out[i] = 0.0 if p is None else (s - p[0]) / p[1]
    list(pool.map(one, range(n)))
    pool.shutdown()
    out_dev.copy_from(out)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    ctx = Context.get(0)
    n, T = args.samples, args.size
    data = RFISimulator(T, T, seed=2024, device=0).generate_batch(n, out="complex128").data
    ctx.synchronize()
    scalars = n * 8 * T * T
    src_bytes, dst_bytes = scalars * 8, scalars * 4
    dst = ctx.empty((n, T, T, 8), np.float32)

    # yardstick: a device-to-device copy moving as many bytes as apply does
    half = (src_bytes + dst_bytes) // 2
    a, b = ctx.empty((half,), np.uint8), ctx.empty((half,), np.uint8)
    a.zero_()
    copy = lambda: check(lib.rfi_memcpy(ctx.handle, C.c_void_p(b.ptr), DEVICE, C.c_void_p(a.ptr), DEVICE, half))   # noqa: E731
    copy_ms = [timed(ctx, copy, args.window / args.repeats)[0] for _ in range(args.repeats)]
    copy_med = float(np.median(copy_ms))
    copy_gbps = 2 * half / (copy_med * 1e-3) / 1e9
    spread = (max(copy_ms) - min(copy_ms)) / copy_med
    del a, b

    rows = []
    for scope in ("dataset", "sample"):
        for method in METHODS:
            nz = Normalizer(method, scope=scope, device=0)
            fit_ms, fit_calls = timed(ctx, lambda: nz.fit(data), args.window)
            passes = 6 if method == "robust_scale" else 2
            params = ctx.to_device(np.stack([nz.centres, nz.scales], axis=1).astype(np.float64)) if scope == "sample" else None
            apply = lambda: check(lib.rfi_norm_apply(                                                                # noqa: E731
                ctx.handle, C.c_void_p(data.ptr), C128, NORM_NCHW, n, T * T, nz.centres[0], nz.scales[0],
                C.c_void_p(params.ptr) if params is not None else None, C.c_void_p(dst.ptr), NORM_NHWC))
            apply_ms, apply_calls = timed(ctx, apply, args.window)
            apply_gbps = (src_bytes + dst_bytes) / (apply_ms * 1e-3) / 1e9
            row = {"method": method, "scope": scope, "samples": n, "size": T,
                   "fit_ms": round(fit_ms, 3), "fit_calls": fit_calls, "fit_passes": passes, "fit_bytes": passes * src_bytes,
                   "fit_GBps": round(passes * src_bytes / (fit_ms * 1e-3) / 1e9, 1),
                   "apply_ms": round(apply_ms, 3), "apply_calls": apply_calls, "apply_bytes": src_bytes + dst_bytes,
                   "apply_GBps": round(apply_gbps, 1), "apply_over_memcpy": round(apply_gbps / copy_gbps, 3)}
            if args.host:
                row["host_route_ms"] = round(host_route(ctx, data, method, scope, dst) * 1e3, 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
    print(json.dumps({"memcpy_bytes_moved": 2 * half, "memcpy_ms": [round(m, 3) for m in copy_ms],
                      "memcpy_GBps": round(copy_gbps, 1), "memcpy_spread": round(spread, 4),
                      "device": ctx.device_name()}), flush=True)
    return rows


if __name__ == "__main__":
    main()
