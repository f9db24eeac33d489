#!/usr/bin/env python3
"""Time connected-component labelling and its consumers (rfi_toolbox_amd.components, csrc/components.hip) on planes resident
on the device, next to scipy.ndimage.label on the same planes on this node's host.

    python tools/bench_label_components.py [--window 1.0] [--repeats 5] [--step-timeout 300]

Two stacks of simulator-like masks (lines along time and along frequency, short bursts and specks; about 5 % flagged, four fifths of it in one crossing grid),
8-connected: 64 x 128 x 128 (the detector's training batch) and 64 x 1024 x 1024.  Per stack:
  label      label_components(out="device"): nothing is read back
  despeckle  remove_small_components(min_area=4, out="device"): labelling + the read-back of K + table + keep
  instances  instances_from_masks(min_area=16, max_instances=64): labelling + table + selection + instance masks
  scipy      scipy.ndimage.label over the same planes, one after the other, one host thread (one pass, wall clock)
GPU figures are taken after a warm-up call, from device events on the library's stream ending in a synchronise around the
whole call (the result's allocation and the read-backs included, its release not), call after call for --window seconds
and at least --repeats calls: ms is the median call, spread its (90th - 10th percentile) / median; mean_ms and max_ms show
what the median hides (the runtime's allocator now and then stalls a call that allocates gigabytes).  The
labels of the first planes are compared with scipy's before anything is timed.

Every (stack, step) runs in a child process of its own under --step-timeout seconds, and a step that fails ends the run.
One JSON line."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STACKS = {"64x128": (64, 128), "64x1024": (64, 1024)}
STEPS = ("label", "despeckle", "instances")


def planes(batch, size, seed=0):
    """Binary masks in the manner of the simulator's: full-length and partial lines both ways, bursts, specks."""
    rng = np.random.default_rng(seed)
    m = np.zeros((batch, size, size), np.uint8)
    for p in m:
        for _ in range(max(3, size // 16)):
            w = int(rng.integers(1, 4))
            if rng.random() < 0.5:
                r, a, b = rng.integers(0, size - w), *sorted(rng.integers(0, size, 2))
                p[r:r + w, a:b + 1] = 1
            else:
                c, a, b = rng.integers(0, size - w), *sorted(rng.integers(0, size, 2))
                p[a:b + 1, c:c + w] = 1
        for _ in range(size // 8):
            y, x = rng.integers(0, size - 8, 2)
            p[y:y + int(rng.integers(1, 8)), x:x + int(rng.integers(1, 8))] = 1
        p[rng.random((size, size)) < 0.004] = 1
    return m


def run_step(stack, step, window, repeats):
    from rfi_toolbox_amd import components as cc
    from rfi_toolbox_amd._lib import check, lib
    from rfi_toolbox_amd.runtime import Context
    import scipy.ndimage as ndi
    batch, size = STACKS[stack]
    host = planes(batch, size)
    ctx = Context.get(0)
    dev = ctx.to_device(host)
    fn = {"label": lambda: cc.label_components(dev, 8, out="device"),
          "despeckle": lambda: cc.remove_small_components(dev, 4, 8, out="device"),
          "instances": lambda: cc.instances_from_masks(dev, 8, min_area=16, max_instances=64)}[step]
    s8 = ndi.generate_binary_structure(2, 2)
    lab, k = cc.label_components(dev, 8)
    for i in range(min(batch, 4)):
        want, kk = ndi.label(host[i], s8)
        assert kk == k[i] and np.array_equal(want, lab[i]), "labels differ from scipy.ndimage.label"
    del lab

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
    row = {"ms": round(med, 4), "spread": round(float(calls[int(0.9 * (len(calls) - 1))] - calls[int(0.1 * (len(calls) - 1))]) / med, 3),
           "mean_ms": round(float(calls.mean()), 4), "max_ms": round(float(calls[-1]), 2), "calls": len(calls)}
    if step == "label":
        t0 = time.perf_counter()
        comps = sum(ndi.label(p, s8)[1] for p in host)
        row.update(scipy_ms=round((time.perf_counter() - t0) * 1e3, 2), components_per_plane=round(comps / batch, 1),
                   flagged_share=round(float(host.mean()), 4), device=ctx.device_name())
    if step == "instances":
        t = fn()
        row.update(instances_per_plane=round(float(t.count_host.mean()), 1), planes_cut=int((t.n_survivors_host > t.count_host).sum()))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-timeout", type=float, default=300.0)
    ap.add_argument("--child", nargs=2, metavar=("STACK", "STEP"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return run_step(args.child[0], args.child[1], args.window, args.repeats)
    out = {}
    for stack in STACKS:
        for step in STEPS:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--window", str(args.window),
                   "--repeats", str(args.repeats), "--child", stack, step]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:                     # a step that failed, faulted or ran out of time ends the run
                sys.stderr.write(r.stdout + r.stderr)
                print(json.dumps({"failed": [stack, step], "returncode": r.returncode, **out}), flush=True)
                return r.returncode
            out[f"{stack}_{step}"] = json.loads(r.stdout.strip().splitlines()[-1])
    for stack in STACKS:
        lab = out[f"{stack}_label"]
        lab["scipy_over_gpu"] = round(lab["scipy_ms"] / lab["ms"], 1)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
