#!/usr/bin/env python3
"""Time the SumThreshold baseline flagger (flagging.sumthreshold_flags, csrc/sumthreshold.hip) on 64 device-resident
complex64 planes of 1024 x 1024 with the default strategy, flags left on the device.

    python tools/bench_sumthreshold.py [--planes 64] [--size 1024] [--repeats 5] [--no-cpu]

Every figure is taken after a warm-up call, from device events on the library's stream ending in a synchronise
(rfi_timer_start / rfi_timer_stop); the result is the median over --repeats calls, its spread (max - min) / median.

Bytes the algorithm must move, per sample (the formula behind `algorithmic_bytes`; intermediate planes that a fused
implementation could keep on chip are NOT counted, so the figure is the HBM roofline's yardstick, not this
implementation's traffic):
  prepare     8 (complex64 in) + 4 (float32 magnitude out) + 1 (flags out)
  iteration   statistics: 2 selections x 3 radix digits x (4 + 4 + 1)    (magnitude, background, flags)
              passes:     2 axes x levels x (4 + 4 + 1 + 1)              (magnitude, background, flags in, flags out)
              smooth:     4 + 1 + 4 (all but the last iteration)         (magnitude, flags in, background out)
  SIR         2 axes x (1 + 1)
The CPU baseline is the NumPy oracle of the same arithmetic (tests/sumthreshold_ref.py) on one plane of the same size.
One JSON line.
"""
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

HBM_PEAK_GBPS = 8000.0                                    # MI355X HBM3E


def algorithmic_bytes(samples, iterations=3, levels=7):
    per = 13 + iterations * (2 * 3 * 9 + 2 * levels * 10) + (iterations - 1) * 9 + 4
    return samples * per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    ctx = Context.get(0)
    n, s = args.planes, args.size
    rng = np.random.default_rng(0)
    one = (1.0 + 0.1 * rng.standard_normal((s, s))) * np.exp(2j * np.pi * rng.random((s, s)))
    one[s // 3] += 2.0                                     # a channel, a burst and a faint line to find
    one[:, s // 2] += 2.0
    one[s // 5, s // 4:s // 4 + 64] += 0.2
    host = np.stack([np.roll(one, 37 * i, axis=1) for i in range(n)]).astype(np.complex64)
    x = ctx.to_device(host)

    def call():
        return flagging.sumthreshold_flags(x, out="device")

    flags = call()
    ctx.synchronize()
    share = float(flags.numpy().mean())
    ms = []
    for _ in range(args.repeats):
        check(lib.rfi_timer_start(ctx.handle))
        flags = call()
        t = C.c_float()
        check(lib.rfi_timer_stop(ctx.handle, C.byref(t)))
        ms.append(t.value)
    med = float(np.median(ms))
    by = algorithmic_bytes(n * s * s)
    row = {"shape": [n, s, s], "dtype": "complex64", "flagged_share": round(share, 4), "ms_per_call": round(med, 3),
           "spread": round((max(ms) - min(ms)) / med, 3), "planes_per_s": round(n / (med * 1e-3), 1),
           "algorithmic_bytes": by, "achieved_GBps": round(by / (med * 1e-3) / 1e9, 1),
           "share_of_hbm_peak": round(by / (med * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4), "device": ctx.device_name()}
    if not args.no_cpu:
        import sumthreshold_ref as ref
        t0 = time.perf_counter()
        want = ref.flag_plane(host[0])
        row["cpu_oracle_s_per_plane"] = round(time.perf_counter() - t0, 3)
        row["cpu_oracle_equal"] = bool(np.array_equal(want, flags.numpy()[0].view(bool)))
        row["speedup_per_plane"] = round(row["cpu_oracle_s_per_plane"] / (med * 1e-3 / n), 1)
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    main()
