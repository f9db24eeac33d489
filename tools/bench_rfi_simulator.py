#!/usr/bin/env python3
"""Time RFISimulator.generate_batch on the GPU (rfi_toolbox_amd.core, csrc/rfi_sim.hip).

    python tools/bench_rfi_simulator.py [--iters 20] [--warmup 3] [--sizes 1024 256]

For each size (T = F), output (complex64, complex128, nhwc) and Gibbs ringing off / on:
  - kernel time per call: the library's HIP-event profile around the event-table and pixel kernels
    (no allocation, no synchronisation inside the window), and samples/s from it;
  - call rate: samples/s of back-to-back generate_batch calls, wall clock, including the output allocation;
  - bytes written per call (planes + mask, counted from the shapes; the event table is < 0.1 %) over the kernel time,
    against the 6.3 TB/s attainable HBM write/copy rate: the share says whether HBM or the fp64 arithmetic bounds it.
The reference's NumPy time for one 1024x1024 generate_rfi() is quoted from tests/golden/simulator_expected.json: it
was measured on the development host when the fixture was made, not on the machine running this tool.
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

HBM_RATE = 6.3e12
OUT_BYTES = {"complex64": 32, "complex128": 64, "nhwc": 32}     # per pixel, four polarisations / eight channels


def family_ms(ctx, name):
    rep = ctx.profile_report()
    r = rep.get(name)
    return (r["ms"], r["launches"]) if r else (0.0, 0)


def run(size, out, ring, iters, warmup, ctx):
    n = max(1, (8 * 1024 * 1024) // (size * size))          # 8 samples at 1024^2, 128 at 256^2
    sim = RFISimulator(size, size, seed=1234, device=ctx.device_index)
    sim.gibbs_ringing = ring
    for _ in range(warmup):
        sim.generate_batch(n, out=out)
    ctx.synchronize()
    fam = lib.rfi_profile_family_name(7).decode()             # FAM_PREPROCESS: the simulator's launches
    ctx.profile_reset()
    ctx.profile(True)
    t0 = time.perf_counter()
    keep = []
    for _ in range(iters):
        keep.append(sim.generate_batch(n, out=out))
        if len(keep) > 2:
            keep.pop(0)
    ctx.synchronize()
    wall = time.perf_counter() - t0
    ctx.profile(False)
    ms, launches = family_ms(ctx, fam)
    kernel_ms = ms / max(launches, 1)
    bytes_call = n * size * size * (OUT_BYTES[out] + 1)
    rate = bytes_call / (kernel_ms * 1e-3) if kernel_ms > 0 else float("nan")
    return {"size": size, "out": out, "gibbs_ringing": ring, "samples_per_call": n,
            "kernel_ms_per_call": kernel_ms, "kernel_us_per_sample": kernel_ms * 1e3 / n,
            "samples_per_s_kernel": n / (kernel_ms * 1e-3) if kernel_ms > 0 else float("nan"),
            "samples_per_s_calls": n * iters / wall,
            "bytes_written_per_sample": bytes_call // n, "write_TBps": rate / 1e12, "share_of_hbm": rate / HBM_RATE,
            "bound": "HBM writes" if rate / HBM_RATE >= 0.6 else "fp64 arithmetic (not HBM)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 256])
    args = ap.parse_args()
    ctx = Context.get(0)
    with open(os.path.join(ROOT, "tests", "golden", "simulator_expected.json")) as f:
        ref_cpu = json.load(f)["reference_cpu_seconds_1024x1024"]
    results = []
    for size in args.sizes:
        for out in ("complex64", "complex128", "nhwc"):
            for ring in (False, True):
                r = run(size, out, ring, args.iters, args.warmup, ctx)
                results.append(r)
                print(f"{size}^2 {out:10s} ring={int(ring)}  {r['kernel_us_per_sample']:8.1f} us/sample (kernel)  "
                      f"{r['samples_per_s_kernel']:9.0f} samples/s (kernel)  {r['samples_per_s_calls']:9.0f} samples/s "
                      f"(calls)  {r['write_TBps']:.2f} TB/s = {100 * r['share_of_hbm']:.0f} % of 6.3  -> {r['bound']}",
                      flush=True)
    summary = {"tool": "bench_rfi_simulator", "device": ctx.device_name(), "results": results,
               "reference_numpy_s_per_1024x1024_sample": ref_cpu["median"],
               "reference_numpy_note": "dev-box figure: one CPU core of the development host, from the golden fixture"}
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
