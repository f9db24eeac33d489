#!/usr/bin/env python3
"""Time the CASA-style baseline flaggers (flagging.tfcrop_flags, rflag_flags, extend_flags; csrc/casa_flaggers.hip) on 64
device-resident complex64 planes of 1024 x 1024 with their default arguments, flags left on the device.

    python tools/bench_casa_flaggers.py [--planes 64] [--size 1024] [--ntime N] [--repeats 5] [--no-cpu]

Every figure is taken after a warm-up call, from device events on the library's stream ending in a synchronise
(rfi_timer_start / rfi_timer_stop); the result is the median over --repeats calls, its spread (max - min) / median.
GB/s is bytes of input (8 per complex64 sample, 1 per flag for extend) over that time: a rate a user can compare with
the size of an observation, not the traffic of the implementation (the fits walk every line fifteen times per stage).
The CPU baseline is the NumPy oracle of the same arithmetic (tests/casa_flaggers_ref.py) on one plane of the same size.
One JSON line per pipeline."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from rfi_toolbox_amd import flagging                      # noqa: E402
from rfi_toolbox_amd._lib import check, lib               # noqa: E402
from rfi_toolbox_amd.runtime import Context               # noqa: E402


def timed(ctx, call, repeats):
    out = call()
    ctx.synchronize()
    ms = []
    for _ in range(repeats):
        check(lib.rfi_timer_start(ctx.handle))
        out = call()
        t = C.c_float()
        check(lib.rfi_timer_stop(ctx.handle, C.byref(t)))
        ms.append(t.value)
    med = float(np.median(ms))
    return out, med, (max(ms) - min(ms)) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--ntime", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    ctx = Context.get(0)
    n, s = args.planes, args.size
    rng = np.random.default_rng(0)
    one = (1.0 + 0.1 * rng.standard_normal((s, s))) * np.exp(0.3j * rng.standard_normal((s, s)))
    one[s // 3] += 2.0                                     # a channel, a burst and a faint line to find
    one[:, s // 2] += 2.0
    one[s // 5, s // 4:s // 4 + 64] += 0.2
    host = np.stack([np.roll(one, 37 * i, axis=1) for i in range(n)]).astype(np.complex64)
    x = ctx.to_device(host)
    rows = []
    flags = {}
    ext = dict(ntime=args.ntime, growaround=True, flagneartime=True, flagnearfreq=True)
    runs = [("tfcrop", 8, lambda: flagging.tfcrop_flags(x, ntime=args.ntime, out="device")),
            ("rflag", 8, lambda: flagging.rflag_flags(x, ntime=args.ntime, out="device")),
            ("extend", 1, lambda: flagging.extend_flags(flags["tfcrop"], out="device", **ext))]
    for name, bytes_in, call in runs:
        out, med, spread = timed(ctx, call, args.repeats)
        flags[name] = out
        got = out.numpy()
        row = {"pipeline": name, "shape": [n, s, s], "ntime": args.ntime, "flagged_share": round(float(got.mean()), 4),
               "ms_per_call": round(med, 3), "spread": round(spread, 3), "planes_per_s": round(n / (med * 1e-3), 1),
               "input_GBps": round(bytes_in * n * s * s / (med * 1e-3) / 1e9, 2), "device": ctx.device_name()}
        if not args.no_cpu:
            import casa_flaggers_ref as ref
            t0 = time.perf_counter()
            if name == "tfcrop":
                want = ref.tfcrop_plane(host[0], ntime=args.ntime)
            elif name == "rflag":
                want = ref.rflag_plane(host[0], ntime=args.ntime)
            else:
                want = ref.extend_plane(flags["tfcrop"].numpy()[0], ntime=args.ntime, growaround=True, flagneartime=True, flagnearfreq=True)
            row["cpu_oracle_s_per_plane"] = round(time.perf_counter() - t0, 3)
            row["cpu_oracle_equal"] = bool(np.array_equal(want, got[0].view(bool)))
            row["speedup_per_plane"] = round(row["cpu_oracle_s_per_plane"] / (med * 1e-3 / n), 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


if __name__ == "__main__":
    main()
