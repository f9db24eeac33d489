#!/usr/bin/env python3
"""Time the per-emitter instance targets of RFISimulator batches (rfi_toolbox_amd.core.event_table / event_instances,
csrc/rfi_sim.hip) on batches resident on the device.

    python tools/bench_sim_instances.py [--window 1.0] [--repeats 5]

Two batches, max_instances=64: 64 x 128 x 128 (the detector's training batch) and 8 x 512 x 512.  Per batch, in the same
process and on the same batch:
  event_table        area and box of every event slot
  instances          event_instances(batch, max_instances=64): table + selection + classes + instance masks
  instances_nomasks  the same with instance_masks=False
  masks_kernel       rfi_sim_instances alone, writing the instance masks into the buffer of a finished call
  fill               a plain hipMemsetAsync of that buffer: the write-rate yardstick of the store-bound mask kernel
  from_masks         instances_from_masks(batch.mask, max_instances=64): the other route to InstanceTargets (connected
                     components; on these masks it finds one grid plus specks, not the emitters)
Figures are taken after a warm-up call, from device events on the library's stream around the whole call (allocation of the
result and the read-back of the counts included, its release not), call after call for --window seconds and at least
--repeats calls: ms is the median call, spread its (90th - 10th percentile) / median.  masks_over_fill is the ratio of the
two medians.  One JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BATCHES = {"64x128": (64, 128), "8x512": (8, 512)}
G = 64


def timed(ctx, fn, window, repeats):
    from rfi_toolbox_amd._lib import check, lib
    fn()
    ctx.synchronize()
    calls, t0 = [], time.perf_counter()
    while time.perf_counter() - t0 < window or len(calls) < repeats:
        check(lib.rfi_timer_start(ctx.handle))
        res = fn()
        ms = C.c_float()
        check(lib.rfi_timer_stop(ctx.handle, C.byref(ms)))
        del res                                       # (the result's memory is released outside the timed call)
        calls.append(ms.value)
    calls = np.sort(np.asarray(calls))
    med = float(np.median(calls))
    return {"ms": round(med, 4), "spread": round(float(calls[int(0.9 * (len(calls) - 1))] - calls[int(0.1 * (len(calls) - 1))]) / med, 3),
            "calls": len(calls)}


def run(name, window, repeats):
    from rfi_toolbox_amd._lib import check, lib
    from rfi_toolbox_amd.components import instances_from_masks
    from rfi_toolbox_amd.core import RFISimulator, event_instances, event_table
    from rfi_toolbox_amd.core.instances import _sim_args
    from rfi_toolbox_amd.runtime import P
    n, size = BATCHES[name]
    sim = RFISimulator(size, size, seed=0, device=0)
    batch = sim.generate_batch(n, out="nhwc")
    ctx = batch.mask.ctx
    tg = event_instances(batch, max_instances=G)
    if tg.count_host[0] == tg.n_survivors_host[0]:      # nothing cut: the first sample's instances add up to its mask
        assert np.array_equal(tg.masks.numpy()[:tg.count_host[0]].any(0), batch.mask.numpy()[0]), "instance masks do not add up to the mask"
    out = {"instances_per_sample": round(float(tg.count_host.mean()), 1), "samples_cut": int((tg.n_survivors_host > tg.count_host).sum()),
           "mask_bytes": int(tg.masks.nbytes)}
    out["event_table"] = timed(ctx, lambda: event_table(batch), window, repeats)
    out["instances"] = timed(ctx, lambda: event_instances(batch, max_instances=G), window, repeats)
    out["instances_nomasks"] = timed(ctx, lambda: event_instances(batch, max_instances=G, instance_masks=False), window, repeats)
    out["masks_kernel"] = timed(ctx, lambda: check(lib.rfi_sim_instances(*_sim_args(batch), P(tg.component), P(tg.count), P(tg.base), G, 1,
                                                                         P(tg.labels), P(tg.masks))), window, repeats)
    out["fill"] = timed(ctx, lambda: check(lib.rfi_memset(ctx.handle, P(tg.masks), 0, tg.masks.nbytes)), window, repeats)
    out["masks_over_fill"] = round(out["masks_kernel"]["ms"] / out["fill"]["ms"], 2)
    out["mask_write_GBps"] = round(tg.masks.nbytes / out["masks_kernel"]["ms"] / 1e6, 1)
    out["from_masks"] = timed(ctx, lambda: instances_from_masks(batch.mask, max_instances=G), window, repeats)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    from rfi_toolbox_amd.runtime import Context
    out = {"device": Context.get(0).device_name()}
    for name in BATCHES:
        out[name] = run(name, args.window, args.repeats)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
