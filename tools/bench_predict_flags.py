#!/usr/bin/env python3
"""Throughput of whole-observation flag prediction (rfi_toolbox_amd.inference.predict_flags) against the bare eval
forward of the same model, and the per-phase split of one call.

    python tools/bench_predict_flags.py [--planes 16] [--size 1024] [--iters 3] [--warmup 1] [--dtypes float32 bfloat16]
                                        [--channels {3,8}]

Workload: `planes` complex64 planes of size x size, ps 128, batch 64, UNet(3, 1, 32).  For each compute dtype and each
tiling (stride = ps, views 1 / stride 64 / views 4) predict_flags is timed on host input (NumPy) and on device-resident
input (a CUDA tensor, flags returned on the device), wall clock per call.  The bare forward: the eval forward of a
resident batch of 64 patches, device in and out, timed between events on the library's stream.  The phase split comes
from the library's profile of one host-input call at stride = ps (upload / download on the copy stream, gather =
channel extraction, stitch, forward = every other kernel).  Prints one JSON line.

--channels 8: UNet(8, 1, 32) on `planes` baselines of (4, size, size) complex64, the same tilings and host / device rows
for normalizer=None, a fitted dataset-scope pair and sample-scope robust_scale.  The phase split (host input, views 1 and
views 4) reports the fused tiling + normalisation kernel on its own (pol_gather, also per chunk) and, for sample scope,
the statistics kernels; beside it the time of Normalizer.transform on the same samples (the same per-pixel arithmetic
without tiling) and of the sample-scope statistics alone (2 passes over the data, 3 to 6 with quantiles, one
synchronisation per group).
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
    x = torch.randn(BATCH, PS, PS, model.in_channels, device="cuda")
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


def phase_split(model, data, **kw):
    ctx = model.ctx
    ctx.synchronize()
    ctx.profile_reset()
    ctx.profile(True)
    t0 = time.perf_counter()
    predict_flags(model, data, PS, batch_size=BATCH, **kw)
    total = (time.perf_counter() - t0) * 1e3
    ctx.profile(False)
    path = os.path.join(tempfile.mkdtemp(), "predict_profile.csv")
    ctx.profile_dump(path)
    ctx.profile_reset()
    pol = model.in_channels == 8
    other = "statistics" if pol else "gather"              # preprocess-family kernels that are not the fused gather
    ph = {"upload": 0.0, other: 0.0, "forward": 0.0, "stitch": 0.0, "download": 0.0}
    if pol:
        ph["pol_gather"] = 0.0
    chunks = 0
    with open(path) as f:
        for r in csv.DictReader(f):
            ms = float(r["ms"])
            chunks += r["label"] == "stitch"
            if r["label"] == "pol_gather":
                ph["pol_gather"] += ms
            elif r["label"] == "predict_upload":
                ph["upload"] += ms
            elif r["label"] == "predict_download":
                ph["download"] += ms
            elif r["label"] == "stitch":
                ph["stitch"] += ms
            elif r["family"] == "preprocess":
                ph[other] += ms
            else:
                ph["forward"] += ms
    out = {f"{k}_ms": round(v, 3) for k, v in ph.items()}
    out["wall_ms"] = round(total, 3)
    if pol:
        out["chunks"] = chunks
        out["pol_gather_ms_per_chunk"] = round(ph["pol_gather"] / chunks, 4) if chunks else None
    main_ms = ph[other] + ph.get("pol_gather", 0.0) + ph["forward"] + ph["stitch"]
    # upload share: the copies against the main stream's work (they run on the copy stream beside it)
    out["upload_share_of_chunk_time"] = round(ph["upload"] / main_ms, 4) if main_ms else None
    return out


def pol_rows(args, result):
    """--channels 8: the rows of the 8-channel path into `result`."""
    from rfi_toolbox_amd.preprocessing import Normalizer
    rng = np.random.default_rng(0)
    shape = (args.planes, 4, args.size, args.size)
    host = (rng.standard_normal(shape, dtype=np.float32) + 1j * rng.standard_normal(shape, dtype=np.float32)).astype(np.complex64)
    dev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    result["workload"] = f"{args.planes} x (4, {args.size}, {args.size}) complex64, ps {PS}, batch {BATCH}, UNet(8,1,32)"
    forms = {"none": None, "dataset_pair": Normalizer("standardize", "dataset").fit(host[:1]),
             "sample_robust_scale": Normalizer("robust_scale", "sample")}
    for dt in args.dtypes:
        torch.manual_seed(0)
        model = UNet(8, 1, 32, device="cuda:0").eval().set_compute_dtype(dt)
        ctx = model.ctx
        fwd_rate, fwd_ms = bare_forward(model, 20)
        r = {"bare_forward_patches_per_s": round(fwd_rate, 1), "bare_forward_ms_per_batch": round(fwd_ms, 4)}
        for form, nz in forms.items():
            for name, kw in TILINGS.items():
                patches = args.planes * tiling_count(args.size, args.size, PS, kw["stride"], kw["views"])
                for src, data in (("host", host), ("device", dev)):
                    fn = lambda: predict_flags(model, data, PS, batch_size=BATCH, normalizer=nz, broadcast_pols=False, **kw)  # noqa: E731
                    for _ in range(args.warmup):
                        fn()
                    s = wall(fn, args.iters, torch.cuda.synchronize)
                    r[f"{form}_{name}_{src}"] = {"baselines_per_s": round(args.planes / s, 2),
                                                 "mpixel_per_s": round(args.planes * args.size ** 2 / s / 1e6, 2),
                                                 "patches_per_s": round(patches / s, 1), "ms_per_call": round(s * 1e3, 3)}
                r[f"{form}_{name}_device_vs_bare_forward"] = round(r[f"{form}_{name}_device"]["patches_per_s"] / fwd_rate, 4)
            for name in ("stride128_views1", "stride128_views4"):
                r[f"phases_host_{form}_{name}"] = phase_split(model, host, normalizer=nz, broadcast_pols=False, **TILINGS[name])
        # the same per-pixel arithmetic without tiling, and the sample-scope statistics alone, on device-resident samples
        d = ctx.to_device(host)
        fitted = Normalizer("robust_scale", "sample").fit(d)
        for label, fn in (("normalizer_transform_ms", lambda: fitted.transform(d)),
                          ("sample_statistics_no_quantiles_ms", lambda: fitted.statistics(d, quantiles=False)),
                          ("sample_statistics_quantiles_ms", lambda: fitted.statistics(d, quantiles=True))):
            fn()
            r[label] = round(wall(fn, args.iters, ctx.synchronize) * 1e3, 3)
        r["pixels"] = args.planes * args.size ** 2
        result[dt] = r
        del model, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=16)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtypes", nargs="+", default=["float32", "bfloat16"])
    ap.add_argument("--channels", type=int, choices=(3, 8), default=3, help="input channels of the model (8: the polarisation-stacked path)")
    args = ap.parse_args()
    if args.channels == 8:
        result = {}
        pol_rows(args, result)
        print(json.dumps(result))
        return
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
