#!/usr/bin/env python3
"""Time the validity-aware 8-channel input (prior flags and non-finite samples; csrc/dataset_norm.hip, csrc/pol_gather.hip,
rfi_model_predict_flags_valid) against the unmasked path, on 16 simulator samples of 4 x 1024 x 1024 with 10 % random
prior flags per polarisation.

    python tools/bench_valid_path.py [--samples 16] [--size 1024] [--window 0.5] [--dtypes complex128,complex64]

Every row is measured in a process of its own (this script starts itself once per row, one after the other), after a
warm-up call, from device events on the library's stream ending in a synchronise (rfi_timer_start / rfi_timer_stop), over
a window of at least --window seconds.  A row times the masked call and, in the same process on the same data, its
yardstick:

  map      rfi_valid_map (one read of the data and the flags, one byte written per visibility)  |  a device-to-device
           rfi_memcpy moving the same number of bytes, repeated; its spread is (max - min) / median over the repeats
  fit      Normalizer(robust_scale, "sample").fit(data, flags=...): the map pass + 6 masked passes  |  the same fit without flags
  apply    rfi_valid_apply into a preallocated (n, T, F, 8) float32 buffer                         |  rfi_norm_apply
  gather   rfi_valid_gather, 128 x 128 tiles at stride 128, one view                               |  rfi_norm_gather
  predict  predict_flags(UNet(8, 1, 16), ..., flags=...), whole call, host operands and results    |  the same call without flags
  predict_device  the same with data, flags and results in HBM (no transfers)                      |  the same call without flags

Expected from the bytes moved: the masked kernels read one extra byte per visibility of 8 (complex64) or 16 (complex128)
bytes, the map adds one read of the data per fit; the histogram passes are bound by their atomics, not by bytes.
One JSON line per row (the map row carries the memcpy repeats and their spread).
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = ("map", "fit", "apply", "gather", "predict", "predict_device")


def timed(ctx, fn, window):
    """mean device ms per call of fn over >= window seconds (events on the stream, the stop synchronises)"""
    from rfi_toolbox_amd._lib import check, lib
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


def one_row(args):
    from rfi_toolbox_amd._lib import (COMPLEX_CODES, DEVICE, NORM_NCHW, NORM_NHWC, VALID_FLAGS_POL, check, lib)
    from rfi_toolbox_amd.core import RFISimulator
    from rfi_toolbox_amd.inference import predict_flags, tiling_table
    from rfi_toolbox_amd.preprocessing import Normalizer
    from rfi_toolbox_amd.runtime import Context
    ctx = Context.get(0)
    n, T, dt = args.samples, args.size, np.dtype(args.dtype)
    px = T * T
    data = RFISimulator(T, T, seed=2024, device=0).generate_batch(n, out=args.dtype).data
    flags_host = (np.random.default_rng(5).random((n, 4, T, T)) < 0.1).astype(np.uint8)
    flags = ctx.to_device(flags_host)
    ctx.synchronize()
    code = COMPLEX_CODES[dt]
    src_bytes, vis = n * 4 * px * dt.itemsize, n * 4 * px
    row = {"row": args.row, "dtype": args.dtype, "samples": n, "size": T}
    P = lambda d: C.c_void_p(d.ptr)                                                                      # noqa: E731
    if args.row == "map":
        vmap = ctx.empty((n, 4, px), np.uint8)
        masked = lambda: check(lib.rfi_valid_map(ctx.handle, P(data), code, NORM_NCHW, n, px, P(flags), VALID_FLAGS_POL, P(vmap),  # noqa: E731
                                                 None, 0))
        half = (src_bytes + 2 * vis) // 2
        a, b = ctx.empty((half,), np.uint8), ctx.empty((half,), np.uint8)
        a.zero_()
        plain = lambda: check(lib.rfi_memcpy(ctx.handle, P(b), DEVICE, P(a), DEVICE, half))                # noqa: E731
        copies = [timed(ctx, plain, args.window / args.repeats)[0] for _ in range(args.repeats)]
        row.update(bytes=src_bytes + 2 * vis, yardstick="memcpy of the same bytes", memcpy_ms=[round(m, 3) for m in copies],
                   memcpy_spread=round((max(copies) - min(copies)) / float(np.median(copies)), 4))
        plain_ms = float(np.median(copies))
    elif args.row == "fit":
        nz = Normalizer("robust_scale", scope="sample", device=0)
        masked = lambda: nz.fit(data, flags=flags)                                                       # noqa: E731
        plain_ms = timed(ctx, lambda: nz.fit(data), args.window)[0]
        row.update(yardstick="fit without flags", method="robust_scale", scope="sample")
    elif args.row == "apply":
        nz = Normalizer("robust_scale", scope="sample", device=0).fit(data, flags=flags)
        params = ctx.to_device(np.stack([nz.centres, nz.scales], axis=1).astype(np.float64))
        dst, vmap = ctx.empty((n, T, T, 8), np.float32), ctx.empty((n, 4, px), np.uint8)
        check(lib.rfi_valid_map(ctx.handle, P(data), code, NORM_NCHW, n, px, P(flags), VALID_FLAGS_POL, P(vmap), None, 0))
        masked = lambda: check(lib.rfi_valid_apply(ctx.handle, P(data), code, NORM_NCHW, n, px, 0.0, 1.0, P(params), P(vmap), 0.0,  # noqa: E731
                                                   P(dst), NORM_NHWC))
        plain_ms = timed(ctx, lambda: check(lib.rfi_norm_apply(ctx.handle, P(data), code, NORM_NCHW, n, px, 0.0, 1.0, P(params), P(dst),
                                                               NORM_NHWC)), args.window)[0]
        row.update(bytes=src_bytes + vis + 8 * vis, yardstick="rfi_norm_apply")
    elif args.row == "gather":
        table = tiling_table(n, T, T, 128, 128, 1)
        out = ctx.empty((len(table), 128, 128, 8), np.float32)
        common = (ctx.handle, P(data), DEVICE, code, n, T, T, table.ctypes.data_as(C.c_void_p), len(table), 128, 0.25, 3.0, None)
        masked = lambda: check(lib.rfi_valid_gather(*common, P(flags), DEVICE, VALID_FLAGS_POL, 0.0, P(out), DEVICE))   # noqa: E731
        plain_ms = timed(ctx, lambda: check(lib.rfi_norm_gather(*common, P(out), DEVICE)), args.window)[0]
        row.update(bytes=src_bytes + vis + 8 * vis, yardstick="rfi_norm_gather", tiles=len(table))
    else:
        import torch
        from rfi_toolbox_amd.models import UNet
        torch.manual_seed(0)
        model = UNet(8, 1, 16, device=0).eval()
        on_host = args.row == "predict"
        obs, prior = (data.numpy(), flags_host) if on_host else (data, flags)
        nz = Normalizer("standardize", device=0).fit(data)
        kw = dict(patch_size=128, normalizer=nz, out="host" if on_host else "device")
        masked = lambda: predict_flags(model, obs, flags=prior, **kw)                                     # noqa: E731
        plain_ms = timed(ctx, lambda: predict_flags(model, obs, **kw), args.window)[0]
        row.update(yardstick="predict_flags without flags", model="UNet(8, 1, 16)", patch_size=128, host_operands=on_host)
    ms, calls = timed(ctx, masked, args.window)
    row.update(masked_ms=round(ms, 3), calls=calls, yardstick_ms=round(plain_ms, 3), ratio=round(ms / plain_ms, 3),
               device=ctx.device_name())
    if "bytes" in row:
        row["masked_GBps"] = round(row["bytes"] / (ms * 1e-3) / 1e9, 1)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dtypes", default="complex128,complex64")
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--row", choices=ROWS, help=argparse.SUPPRESS)          # (set by this script for its child processes)
    ap.add_argument("--dtype", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.row:
        return one_row(args)
    for dtype in args.dtypes.split(","):
        for row in args.rows.split(","):
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", row, "--dtype", dtype, "--samples", str(args.samples),
                                   "--size", str(args.size), "--window", str(args.window), "--repeats", str(args.repeats)], timeout=300)
            if done.returncode:
                sys.exit(f"row {row} ({dtype}) ended with status {done.returncode}")     # (nothing more is started after a failure)


if __name__ == "__main__":
    main()
