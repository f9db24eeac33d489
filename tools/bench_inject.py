#!/usr/bin/env python3
"""Time RFISimulator.inject against RFISimulator.generate_batch on the GPU (rfi_toolbox_amd.core, csrc/rfi_sim.hip).

    python tools/bench_inject.py [--rounds 5] [--iters 10] [--warmup 2] [--sizes 128 512 1024] [--quick]

Sizes (T = F): 64 x 128^2, 8 x 512^2, 8 x 1024^2.  For each size and dtype (complex64, complex128) the baseline
``generate_batch(out=dtype)`` and every inject variant -- rows time / channel, Gibbs ringing off / on, without / with prior
flags, a given sigma / scale="iqr" -- run ALTERNATING in one process: a round times `iters` back-to-back calls of the
baseline, then of each variant, between two synchronisations (wall clock, allocation of the outputs included, which both
sides pay alike); `rounds` rounds.  Reported per variant: the median over rounds of the time per call, the spread
(max - min over rounds), and the ratio to the baseline of the same dtype, size and ringing in the same rounds.  For the
variants with a given sigma the device time of the simulator's own launches (HIP events, the library's profile) is
printed too, from one more pass of `iters` calls: it leaves out allocation and the upload of sigma.  The input
is a device array (a clean generate_batch of the same dtype); flags are a device uint8 map with 10 % set.
scale="iqr" adds the invalid map and the statistics passes and reads four scalars back, so it synchronises.
Prints one line per configuration and a final JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rfi_toolbox_amd._lib import lib                         # noqa: E402
from rfi_toolbox_amd.core import RFISimulator                # noqa: E402
from rfi_toolbox_amd.runtime import Context                  # noqa: E402

SAMPLES = {128: 64, 512: 8, 1024: 8}


def timed(ctx, fn, iters):
    ctx.synchronize()
    t0 = time.perf_counter()
    keep = None
    for _ in range(iters):
        keep = fn()                                           # (the previous result is released as the next one is bound)
    ctx.synchronize()
    del keep
    return (time.perf_counter() - t0) * 1e3 / iters


def bench_size(ctx, size, dtype, args):
    n = SAMPLES.get(size, max(1, (8 * 1024 * 1024) // (size * size)))
    sim = RFISimulator(size, size, seed=1234, device=ctx.device_index)
    data = sim.generate_batch(n, clean=True, out=dtype).data
    flags = ctx.to_device((np.random.default_rng(0).random((n, 4, size, size)) < 0.1).astype(np.uint8))

    def gen(ring):
        def f():
            sim.gibbs_ringing = ring
            return sim.generate_batch(n, out=dtype)
        return f

    def inj(ring, rows, fl, scale):
        def f():
            sim.gibbs_ringing = ring
            return sim.inject(data, flags if fl else None, scale=scale, rows=rows)
        return f

    variants = [("generate_batch", ring, None, False, None, gen(ring)) for ring in (False, True)]
    for ring in (False, True):
        for rows in ("time", "channel"):
            for fl in (False, True):
                for scale in (1.0, "iqr"):
                    if args.quick and (fl or scale == "iqr") and (ring or rows == "channel"):
                        continue
                    variants.append(("inject", ring, rows, fl, scale, inj(ring, rows, fl, scale)))
    for v in variants:
        for _ in range(args.warmup):
            v[5]()
    times = [[] for _ in variants]
    for _ in range(args.rounds):
        for i, v in enumerate(variants):
            times[i].append(timed(ctx, v[5], args.iters))
    # device time of the simulator's own launches (HIP events around the event-table and pixel / inject kernels, no
    # allocation inside the window): only where no other preprocessing kernel runs, so not for scale="iqr"
    fam = lib.rfi_profile_family_name(7).decode()             # FAM_PREPROCESS
    kernel = []
    for v in variants:
        if v[4] == "iqr":
            kernel.append(None)
            continue
        ctx.synchronize()
        ctx.profile_reset()
        ctx.profile(True)
        keep = None
        for _ in range(args.iters):
            keep = v[5]()
        ctx.synchronize()
        ctx.profile(False)
        del keep
        rep = ctx.profile_report().get(fam)
        kernel.append(rep["ms"] / args.iters if rep else None)
    base = {v[1]: np.array(times[i]) for i, v in enumerate(variants) if v[0] == "generate_batch"}
    base_kernel = {v[1]: kernel[i] for i, v in enumerate(variants) if v[0] == "generate_batch"}
    out = []
    for i, (what, ring, rows, fl, scale, _) in enumerate(variants):
        t = np.array(times[i])
        out.append({"size": size, "samples_per_call": n, "dtype": dtype, "call": what, "gibbs_ringing": ring, "rows": rows,
                    "flags": fl, "scale": scale, "ms_per_call_median": float(np.median(t)), "ms_spread": float(t.max() - t.min()),
                    "ms_rounds": [float(x) for x in t], "kernel_ms_per_call": kernel[i],
                    "baseline_kernel_ms_per_call": base_kernel[ring], "ratio_to_generate_batch": float(np.median(t / base[ring])),
                    "baseline_ms_median": float(np.median(base[ring])), "baseline_ms_spread": float(base[ring].max() - base[ring].min())})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 512, 1024])
    ap.add_argument("--quick", action="store_true", help="flags and scale='iqr' only with rows='time', ringing off")
    args = ap.parse_args()
    ctx = Context.get(0)
    results = []
    for size in args.sizes:
        for dtype in ("complex64", "complex128"):
            for r in bench_size(ctx, size, dtype, args):
                results.append(r)
                name = r["call"] if r["call"] == "generate_batch" else \
                    f"inject rows={r['rows']:7s} flags={int(r['flags'])} scale={r['scale']}"
                print(f"{r['samples_per_call']:3d} x {size}^2 {dtype:10s} ring={int(r['gibbs_ringing'])} {name:44s} "
                      f"{r['ms_per_call_median']:9.3f} ms/call  spread {r['ms_spread']:7.3f}  x{r['ratio_to_generate_batch']:.2f} of "
                      f"generate_batch ({r['baseline_ms_median']:.3f} ms, spread {r['baseline_ms_spread']:.3f})"
                      + ("" if r["kernel_ms_per_call"] is None else f"  kernels {r['kernel_ms_per_call']:.3f} ms"), flush=True)
    print(json.dumps({"tool": "bench_inject", "device": ctx.device_name(), "rounds": args.rounds, "iters": args.iters,
                      "results": results}))


if __name__ == "__main__":
    main()
