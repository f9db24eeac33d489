#!/usr/bin/env python3
"""Time the instance stitch (rfi_toolbox_amd.inference.stitch_instances, csrc/instance_stitch.hip) on per-tile detections
resident on the device, next to three reference numbers measured in the same process.

    python tools/bench_detect_observation.py [--window 1.0] [--repeats 5] [--step-timeout 300]

Cases: 8 baselines of 1024 x 1024 in 128-tiles at stride 128 and 96 with max_det = 20, stride 96 once more with
max_det = 100, and one 512 x 512 plane.  The detections are simulator-like: per plane 12 lines along time or frequency, one
to three pixels wide, and 6 blobs, each cut into its per-tile pieces, plus max_det / 5 small blobs per tile.  Per case:
  stitch        rfi_stitch_instances with instance masks at max_events = 64
  stitch_flags  the same without instance masks (what detect_observation does by default)
  copy          a device-to-device copy of the same tile-mask bytes: the floor, since every byte must be read once
  detect        MaskRCNN(6, 8, 16, 64, 128).detect over the same number of tiles in batches of 64 (resident input, untrained
                weights, score_thresh 0): the work detect_observation does before the stitch
  numpy         the route available without the kernels, once, wall clock: download the tile masks, then OR every valid slot
                into its plane with one slice assignment per slot -- the flags alone, no links, the lower bound of a host merge
GPU figures are taken after a warm-up call, from device events on the library's stream around the whole call, call after
call for --window seconds and at least --repeats calls: ms is the median call, spread its (90th - 10th percentile) /
median.  The flags of the stitch are compared with the NumPy route's before the row is printed.

Every case runs in a child process of its own under --step-timeout seconds, and a case that fails ends the run.
One JSON line."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PS = 128
CASES = {"8x1024_s128_d20": (8, 1024, 128, 20), "8x1024_s96_d20": (8, 1024, 96, 20), "8x1024_s96_d100": (8, 1024, 96, 100),
         "1x512_s128_d20": (1, 512, 128, 20)}


def make(n, size, s, D, seed=0):
    """-> the tile detections of n planes of size x size (views 1, edge pad) and the (row0, col0) of a plane's tiles."""
    from rfi_toolbox_amd.inference import tiling_table
    rng = np.random.default_rng(seed)
    tiles = [(int(r0), int(c0)) for _, _, r0, c0 in tiling_table(1, size, size, PS, s)]
    N = n * len(tiles)
    det = {"boxes": np.zeros((N, D, 4), np.float32), "scores": np.zeros((N, D), np.float32), "labels": np.zeros((N, D), np.int32),
           "counts": np.zeros((N,), np.int32), "masks": np.zeros((N, D, PS, PS), np.uint8)}
    for p in range(n):
        events = []                                        # (label, score, r0, r1, c0, c1): rectangles of the plane
        for _ in range(12):
            w, at = int(rng.integers(1, 4)), int(rng.integers(0, size - 3))
            a, b = sorted(int(v) for v in rng.integers(0, size, 2))
            along_time = rng.random() < 0.5
            events.append((1 + int(along_time), float(rng.random()), at, at + w, a, b + 1) if along_time else
                          (1 + int(along_time), float(rng.random()), a, b + 1, at, at + w))
        for _ in range(6):
            y, x = (int(v) for v in rng.integers(0, size - 40, 2))
            events.append((3 + int(rng.integers(0, 3)), float(rng.random()), y, y + int(rng.integers(4, 40)), x, x + int(rng.integers(4, 40))))
        for ti, (r0, c0) in enumerate(tiles):
            i, k = p * len(tiles) + ti, 0
            for label, score, y0, y1, x0, x1 in events:
                ya, yb, xa, xb = max(y0, r0) - r0, min(y1, r0 + PS, size) - r0, max(x0, c0) - c0, min(x1, c0 + PS, size) - c0
                if ya >= yb or xa >= xb or k >= D:
                    continue
                det["masks"][i, k, ya:yb, xa:xb] = 1
                det["boxes"][i, k], det["scores"][i, k], det["labels"][i, k] = (xa, ya, xb, yb), score, label
                k += 1
            for _ in range(D // 5):
                if k >= D:
                    break
                y, x = (int(v) for v in rng.integers(0, PS - 8, 2))
                h, w = (int(v) for v in rng.integers(2, 8, 2))
                det["masks"][i, k, y:y + h, x:x + w] = 1
                det["boxes"][i, k], det["scores"][i, k], det["labels"][i, k] = (x, y, x + w, y + h), float(rng.random()) * 0.3, 5
                k += 1
            det["counts"][i] = k
    return det, tiles


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
        del res
        calls.append(ms.value)
    calls = np.sort(np.asarray(calls))
    med = float(np.median(calls))
    return {"ms": round(med, 4), "spread": round(float(calls[int(0.9 * (len(calls) - 1))] - calls[int(0.1 * (len(calls) - 1))]) / med, 3),
            "calls": len(calls)}


def run_case(name, window, repeats):
    import torch
    from rfi_toolbox_amd._lib import DEVICE, check, lib
    from rfi_toolbox_amd.inference import stitch_instances
    from rfi_toolbox_amd.models import MaskRCNN
    from rfi_toolbox_amd.runtime import Context, P
    n, size, s, D = CASES[name]
    host, tiles = make(n, size, s, D)
    ctx = Context.get(0)
    det = {k: ctx.to_device(v) for k, v in host.items()}
    N = len(host["counts"])
    copy_dst = ctx.empty(host["masks"].shape, np.uint8)
    kw = dict(channels=size, times=size, patch_size=PS, stride=s, max_events=64)

    def stitch():
        return stitch_instances(det, instance_masks=True, **kw)

    def stitch_flags():
        return stitch_instances(det, instance_masks=False, **kw)

    def copy():
        check(lib.rfi_memcpy(ctx.handle, P(copy_dst), DEVICE, P(det["masks"]), DEVICE, det["masks"].nbytes))

    torch.manual_seed(0)
    model = MaskRCNN(6, 8, 16, 64, 128)
    model.score_thresh, model.max_det = 0.0, D
    bs = min(64, N)
    x = ctx.to_device(np.random.default_rng(1).standard_normal((bs, PS, PS, 8)).astype(np.float32))

    def detect():
        for _ in range(-(-N // bs)):
            model.detect(x, instance_masks=True, out="device")

    row = {k: timed(ctx, f, window, repeats) for k, f in (("stitch", stitch), ("stitch_flags", stitch_flags), ("copy", copy),
                                                          ("detect", detect))}
    ctx.profile(True)                                      # one profiled call: which pass the time goes to
    ctx.profile_reset()
    stitch()
    ctx.synchronize()
    with tempfile.TemporaryDirectory() as tmp:
        ctx.profile_dump(os.path.join(tmp, "launches.csv"))
        lines = [l.split(",") for l in open(os.path.join(tmp, "launches.csv")).read().splitlines()[1:]]
    ctx.profile(False)
    row["passes_ms"] = {l[2]: round(float(l[3]), 4) for l in lines if l[2].startswith("stitch_inst")}
    # the NumPy route: the tile masks come down, then one OR per valid slot
    t0 = time.perf_counter()
    hm, hc = det["masks"].numpy(), det["counts"].numpy()
    t_down = time.perf_counter() - t0
    flags = np.zeros((n, size, size), np.uint8)
    for i in range(N):
        r0, c0 = tiles[i % len(tiles)]
        h, w = min(PS, size - r0), min(PS, size - c0)
        for j in range(int(hc[i])):
            flags[i // len(tiles), r0:r0 + h, c0:c0 + w] |= hm[i, j, :h, :w]
    t_all = time.perf_counter() - t0
    res = stitch()
    assert np.array_equal(res["rfi_mask"].numpy(), flags), "the flags differ from the NumPy route's"
    row.update(numpy_ms=round(t_all * 1e3, 1), numpy_download_ms=round(t_down * 1e3, 1), tiles=N, slots=int(hc.sum()),
               events=res["counts"].numpy().tolist(), mask_mbytes=round(host["masks"].nbytes / 1e6, 1), device=ctx.device_name())
    row["stitch_over_copy"] = round(row["stitch"]["ms"] / row["copy"]["ms"], 2)
    row["stitch_over_detect"] = round(row["stitch"]["ms"] / row["detect"]["ms"], 3)
    row["numpy_over_stitch"] = round(row["numpy_ms"] / row["stitch"]["ms"], 1)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-timeout", type=float, default=300.0)
    ap.add_argument("--child", metavar="CASE", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return run_case(args.child, args.window, args.repeats)
    out = {}
    for name in CASES:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--window", str(args.window),
               "--repeats", str(args.repeats), "--child", name]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:                         # a case that failed, faulted or ran out of time ends the run
            sys.stderr.write(r.stdout + r.stderr)
            print(json.dumps({"failed": name, "returncode": r.returncode, **out}), flush=True)
            return r.returncode
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
