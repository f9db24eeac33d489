#!/usr/bin/env python3
"""Throughput of whole-observation flag prediction (rfi_toolbox_amd.inference.predict_flags) against the bare eval
forward of the same model, and the per-phase split of one call.

    python tools/bench_predict_flags.py [--planes 16] [--size 1024] [--iters 3] [--warmup 1] [--dtypes float32 bfloat16]

Workload: `planes` complex64 planes of size x size, ps 128, batch 64, UNet(3, 1, 32).  For each compute dtype and each
tiling (stride = ps, views 1 / stride 64 / views 4) predict_flags is timed on host input (NumPy) and on device-resident
input (a CUDA tensor, flags returned on the device), wall clock per call.  The bare forward: the eval forward of a
resident batch of 64 patches, device in and out, timed between events on the library's stream.  The phase split comes
from the library's profile of one host-input call at stride = ps (upload / download on the copy stream, gather =
channel extraction, stitch, forward = every other kernel).  Prints one JSON line.
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rfi_toolbox_amd._lib import DEVICE, check, lib                        # noqa: E402
from rfi_toolbox_amd.inference import predict_flags, tiling_count         # noqa: E402
from rfi_toolbox_amd.models import UNet                                   # noqa: E402

PS, BATCH = 128, 64
TILINGS = {"stride128_views1": dict(stride=128, views=1), "stride64_views1": dict(stride=64, views=1),
           "stride128_views4": dict(stride=128, views=4)}


def wall(fn, iters, sync):
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    sync()
    return (time.perf_counter() - t0) / iters


def bare_forward(model, iters):
    ctx = model.ctx
    x = torch.randn(BATCH, PS, PS, 3, device="cuda")
    y = torch.empty(BATCH, PS, PS, device="cuda")
    torch.cuda.synchronize()

    def step():
        check(lib.rfi_model_forward_nhwc(model._h, C.c_void_p(x.data_ptr()), DEVICE, BATCH, PS, PS,
                                         C.c_void_p(y.data_ptr()), DEVICE))
    for _ in range(3):
        step()
    ctx.timer_start()
    for _ in range(iters):
        step()
    ms = ctx.timer_stop() / iters
    return BATCH / (ms * 1e-3), ms


def phase_split(model, data):
    ctx = model.ctx
    ctx.synchronize()
    ctx.profile_reset()
    ctx.profile(True)
    t0 = time.perf_counter()
    predict_flags(model, data, PS, batch_size=BATCH)
    total = (time.perf_counter() - t0) * 1e3
    ctx.profile(False)
    path = os.path.join(tempfile.mkdtemp(), "predict_profile.csv")
    ctx.profile_dump(path)
    ctx.profile_reset()
    ph = {"upload": 0.0, "gather": 0.0, "forward": 0.0, "stitch": 0.0, "download": 0.0}
    with open(path) as f:
        for r in csv.DictReader(f):
            ms = float(r["ms"])
            if r["label"] == "predict_upload":
                ph["upload"] += ms
            elif r["label"] == "predict_download":
                ph["download"] += ms
            elif r["label"] == "stitch":
                ph["stitch"] += ms
            elif r["family"] == "preprocess":
                ph["gather"] += ms
            else:
                ph["forward"] += ms
    out = {f"{k}_ms": round(v, 3) for k, v in ph.items()}
    out["wall_ms"] = round(total, 3)
    main_ms = ph["gather"] + ph["forward"] + ph["stitch"]
    # upload share: the copies against the main stream's work (they run on the copy stream beside it)
    out["upload_share_of_chunk_time"] = round(ph["upload"] / main_ms, 4) if main_ms else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=16)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtypes", nargs="+", default=["float32", "bfloat16"])
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    shape = (args.planes, args.size, args.size)
    host = (rng.standard_normal(shape, dtype=np.float32) + 1j * rng.standard_normal(shape, dtype=np.float32)).astype(np.complex64)
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    result = {"workload": f"{args.planes} x complex64 {args.size}x{args.size}, ps {PS}, batch {BATCH}, UNet(3,1,32)"}
    for dt in args.dtypes:
        torch.manual_seed(0)
        model = UNet(3, 1, 32, device="cuda:0").eval().set_compute_dtype(dt)
        fwd_rate, fwd_ms = bare_forward(model, 20)
        r = {"bare_forward_patches_per_s": round(fwd_rate, 1), "bare_forward_ms_per_batch": round(fwd_ms, 4)}
        for name, kw in TILINGS.items():
            patches = args.planes * tiling_count(args.size, args.size, PS, kw["stride"], kw["views"])
            for src, data in (("host", host), ("device", dev)):
                fn = lambda: predict_flags(model, data, PS, batch_size=BATCH, **kw)        # noqa: E731
                for _ in range(args.warmup):
                    fn()
                s = wall(fn, args.iters, torch.cuda.synchronize)
                r[f"{name}_{src}"] = {"planes_per_s": round(args.planes / s, 2),
                                      "mpixel_per_s": round(args.planes * args.size ** 2 / s / 1e6, 2),
                                      "patches_per_s": round(patches / s, 1), "ms_per_call": round(s * 1e3, 3)}
            r[f"{name}_device_vs_bare_forward"] = round(r[f"{name}_device"]["patches_per_s"] / fwd_rate, 4)
        r["phases_host_stride128_views1"] = phase_split(model, host)
        result[dt] = r
        del model
    print(json.dumps(result))


if __name__ == "__main__":
    main()
