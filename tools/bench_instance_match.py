#!/usr/bin/env python3
"""Time instance matching (rfi_toolbox_amd.evaluation.detection, csrc/instance_match.hip) on detections and instance
targets resident on the device, next to two reference numbers measured in the same process.

    python tools/bench_instance_match.py [--window 1.0] [--repeats 5] [--step-timeout 300]

Three cases of simulator-like instances (thin lines along time and along frequency, one to three pixels wide, plus small
blobs), D = 100 detections per image, of which two thirds are a ground truth moved by up to two pixels:
64 x 128 x 128 with G = 16, the same with G = 64, and 8 x 512 x 512 with G = 64.  Per case:
  pack      rfi_op_pack_masks over the n D detection planes
  copy      a device-to-device copy of the same mask bytes: the floor of the pack kernel (it reads every byte once)
  mask_iou  rfi_op_mask_iou on the packed planes of both sides
  match     rfi_op_match_instances at the ten default thresholds
  update    DetectionScorer.update on the device dict and the InstanceTargets: pack of both sides, IoU, matching, the
            allocation of the results and the read-back of the small arrays
  numpy     the route available without this module, once, wall clock: download both sets of masks, then
            (a & b).sum() for every pair whose boxes overlap
GPU figures are taken after a warm-up call, from device events on the library's stream around the whole call, call after
call for --window seconds and at least --repeats calls: ms is the median call, spread its (90th - 10th percentile) /
median.  The intersections of the first image are compared with NumPy's before anything is timed.

Every case runs in a child process of its own under --step-timeout seconds, and a case that fails ends the run.
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

CASES = {"64x128_g16": (64, 128, 100, 16), "64x128_g64": (64, 128, 100, 64), "8x512_g64": (8, 512, 100, 64)}


def instance(rng, size):
    m = np.zeros((size, size), np.uint8)
    w = int(rng.integers(1, 4))
    kind = rng.random()
    if kind < 0.4:
        r, a, b = rng.integers(0, size - w), *sorted(rng.integers(0, size, 2))
        m[r:r + w, a:b + 1] = 1
    elif kind < 0.8:
        c, a, b = rng.integers(0, size - w), *sorted(rng.integers(0, size, 2))
        m[a:b + 1, c:c + w] = 1
    else:
        y, x = rng.integers(0, size - 12, 2)
        m[y:y + int(rng.integers(2, 12)), x:x + int(rng.integers(2, 12))] = 1
    return m


def box_of(m):
    ys, xs = np.nonzero(m)
    return np.asarray([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1], np.float32) if len(ys) else np.zeros(4, np.float32)


def make(n, size, D, G, seed=0):
    rng = np.random.default_rng(seed)
    gm, dm = np.zeros((n, G, size, size), np.uint8), np.zeros((n, D, size, size), np.uint8)
    gl, dl = rng.integers(1, 6, (n, G)).astype(np.int32), rng.integers(1, 6, (n, D)).astype(np.int32)
    for i in range(n):
        for g in range(G):
            gm[i, g] = instance(rng, size)
        for d in range(D):
            if rng.random() < 2 / 3:
                g = int(rng.integers(0, G))
                dm[i, d] = np.roll(gm[i, g], tuple(rng.integers(-2, 3, 2)), (0, 1))
                dl[i, d] = gl[i, g]
            else:
                dm[i, d] = instance(rng, size)
    scores = np.sort(rng.random((n, D)).astype(np.float32), axis=1)[:, ::-1].copy()
    gb = np.stack([[box_of(m) for m in img] for img in gm])
    db = np.stack([[box_of(m) for m in img] for img in dm])
    return dm, db, dl, scores, gm, gb, gl


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
    from rfi_toolbox_amd._lib import DEVICE, check, lib
    from rfi_toolbox_amd.components import InstanceTargets
    from rfi_toolbox_amd.evaluation import DetectionScorer, default_iou_thresholds
    from rfi_toolbox_amd.runtime import Context, P
    n, size, D, G = CASES[name]
    dm, db, dl, scores, gm, gb, gl = make(n, size, D, G)
    ctx = Context.get(0)
    up = ctx.to_device
    wc = (size + 63) // 64
    d_masks, g_masks = up(dm), up(gm)
    cnt_d, cnt_g = np.full(n, D, np.int32), np.full(n, G, np.int32)
    d_count, g_count = up(cnt_d), up(cnt_g)
    d_base, g_base = up(np.arange(n, dtype=np.int32) * D), up(np.arange(n, dtype=np.int32) * G)
    sides = []
    for m in (n * D, n * G):
        sides.append((ctx.empty((m, size, wc), np.uint64), ctx.empty((m,), np.int32), ctx.empty((m, 4), np.int32)))
    (d_bits, d_area, d_ext), (g_bits, g_area, g_ext) = sides
    inter, iou = ctx.empty((n, D, G), np.int32), ctx.empty((n, D, G), np.float32)
    thr = default_iou_thresholds()
    T = thr.size
    det_match, gt_match = ctx.empty((n, T, D), np.int32), ctx.empty((n, T, G), np.int32)
    d_scores, d_labels, g_labels = up(scores), up(dl), up(gl)
    copy_dst = ctx.empty(dm.shape, np.uint8)

    def pack():
        check(lib.rfi_op_pack_masks(ctx.handle, P(d_masks), n * D, size, size, P(d_bits), P(d_area), P(d_ext)))

    def copy():
        check(lib.rfi_memcpy(ctx.handle, P(copy_dst), DEVICE, P(d_masks), DEVICE, d_masks.nbytes))

    def mask_iou():
        check(lib.rfi_op_mask_iou(ctx.handle, P(d_bits), P(d_area), P(d_ext), P(d_count), P(d_base), n * D, P(g_bits), P(g_area), P(g_ext),
                                  P(g_count), P(g_base), n * G, n, D, G, size, size, P(inter), P(iou)))

    def match():
        check(lib.rfi_op_match_instances(ctx.handle, P(iou), P(d_scores), P(d_labels), P(d_count), P(g_labels), P(g_count), n, D, G,
                                         thr.ctypes.data_as(C.c_void_p), T, 1, P(det_match), P(gt_match)))

    z = np.zeros(n, np.int32)
    targets = InstanceTargets((size, size), up(gb), g_labels, g_count, g_count, g_base, up(np.zeros((n, G), np.int32)), g_masks, cnt_g, cnt_g, z,
                              num_classes=6)
    det = {"boxes": up(db), "scores": d_scores, "labels": d_labels, "counts": d_count, "masks": d_masks}

    def update():
        return DetectionScorer(6).update(det, targets)

    pack()
    check(lib.rfi_op_pack_masks(ctx.handle, P(g_masks), n * G, size, size, P(g_bits), P(g_area), P(g_ext)))
    mask_iou()
    want = (dm[0].reshape(D, -1).astype(np.int64) @ gm[0].reshape(G, -1).astype(np.int64).T).astype(np.int32)
    assert np.array_equal(inter.numpy()[0], want), "intersections differ from NumPy's"

    row = {k: timed(ctx, f, window, repeats) for k, f in (("pack", pack), ("copy", copy), ("mask_iou", mask_iou), ("match", match),
                                                          ("update", update))}
    # the NumPy route: both sets of masks come down, then every pair whose boxes overlap
    t0 = time.perf_counter()
    hd, hg = d_masks.numpy(), g_masks.numpy()
    t_down = time.perf_counter() - t0
    pairs, total = 0, 0
    for i in range(n):
        for d in range(D):
            a, ab = hd[i, d], db[i, d]
            for g in range(G):
                b = gb[i, g]
                if min(ab[2], b[2]) > max(ab[0], b[0]) and min(ab[3], b[3]) > max(ab[1], b[1]):
                    total += int((a & hg[i, g]).sum())
                    pairs += 1
    t_all = time.perf_counter() - t0
    assert total == int(inter.numpy().sum(dtype=np.int64)), "the NumPy route found another total intersection"
    row.update(numpy_ms=round(t_all * 1e3, 1), numpy_download_ms=round(t_down * 1e3, 1), overlapping_pairs=pairs, pairs=n * D * G,
               mask_mbytes=round((dm.nbytes + gm.nbytes) / 1e6, 1), device=ctx.device_name())
    row["pack_over_copy"] = round(row["pack"]["ms"] / row["copy"]["ms"], 2)
    row["numpy_over_update"] = round(row["numpy_ms"] / row["update"]["ms"], 1)
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
