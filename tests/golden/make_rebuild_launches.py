#!/usr/bin/env python3
"""Generate tests/golden/rebuild_launches.json: every kernel launch of a pass that has derived filter copies to rebuild
("Derived filter copies: who invalidates, who rebuilds"), in order, from the context profile.

Run from the repository root on an MI355X:

    RFI_HIP_LIB=<librfi_hip.so of the parent commit> python tests/golden/make_rebuild_launches.py

The committed fixture is a regression pin of the rebuild orchestration: it was written with the library of the commit BEFORE
the staleness of the copies moved into one mask (rfi_model::stale, sync_filters), never with the library it is meant to
check.  Regenerate it only together with a deliberate change of which launch rebuilds which copy, or when.
tests/test_gpu_rebuild_launches.py imports CASES and rebuild_launches from this file.

Models: four rows of tests/derived_copy_cases.py at their first shape -- the plain U-Net, the ResNet-encoder U-Net (its
stride-2 filter forms), the mask head, the ResNet-50-FPN backbone (its per-pass and frozen-BatchNorm rebuilds) -- in
every compute mode.  Three scripts each; `pass` is forward + backward, `step` a training step:
    steps       two steps, the second profiled
    load        a pass, load_state_dict of the row's mid-network weight, a profiled pass
    mode_trip   mode A, a pass, mode B (the next of MODES), a step, mode A again, a profiled pass
Kept per profiled pass: the number of rows, the SHA-256 of the ordered "family,label,mbytes" lines, and the ordered
[label, mbytes] rows of the elementwise family, where every rebuild launch records itself.
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
JSON_PATH = os.path.join(HERE, "rebuild_launches.json")
sys.path[:0] = [p for p in (ROOT, os.path.dirname(HERE)) if p not in sys.path]

import derived_copy_cases as D  # noqa: E402

ROWS = ("unet_f16", "resnet18_f16", "mask_head", "backbone")
SCRIPTS = ("steps", "load", "mode_trip")
CASES = tuple((row, mode, script) for row in ROWS for mode in D.MODES for script in SCRIPTS)


def case_id(row, mode, script):
    return f"{row}-{mode}-{script}"


def _pass(arch, m):
    D._forward_backward(arch, m.train(), D.inputs(arch, 0), {})


def _step(arch, m):
    if arch.kind in D.HAS_LOSS:
        m.train().train_step(*D.inputs(arch, 0), **D.STEP)
    else:
        _pass(arch, m)
        m.apply_gradients(**D.STEP)


def _profiled(fn):
    """-> the [family, label, mbytes] rows of the launches of fn()"""
    from rfi_toolbox_amd.runtime import Context
    c = Context.get(0)
    c.profile_reset()
    c.profile(True)
    try:
        fn()
    finally:
        c.profile(False)
    fd, path = tempfile.mkstemp(suffix=".csv")
    os.close(fd)
    try:
        c.profile_dump(path)
        rows = [line.rstrip("\n").split(",") for line in open(path)][1:]
    finally:
        os.remove(path)
        c.profile_reset()
    # index,family,label,ms,gflop,tflops,mbytes,gbs (a label may hold commas: count the numeric columns from the right)
    return [[r[1], ",".join(r[2:-5]), r[-2]] for r in rows]


def rebuild_launches(row, mode, script):
    """-> {"rows": n, "sha256": of the ordered family,label,mbytes lines, "elementwise": [[label, mbytes], ...]}"""
    arch = D.BY_ID[row]
    m = D.build(arch, mode, seed=1000 + D.ARCHS.index(arch))
    if script == "steps":
        _step(arch, m)
        rows = _profiled(lambda: _step(arch, m))
    elif script == "load":
        _pass(arch, m)
        old = D.table_state(m)[arch.mid].numpy()
        new = old * (1.0 + 0.25 * np.random.default_rng(77).standard_normal(old.shape))
        D.table_load(m, {arch.mid: new.astype(np.float32)})
        rows = _profiled(lambda: _pass(arch, m))
    else:
        _pass(arch, m)
        m.set_compute_dtype(D.MODES[(D.MODES.index(mode) + 1) % len(D.MODES)])
        _step(arch, m)
        m.set_compute_dtype(mode)
        rows = _profiled(lambda: _pass(arch, m))
    text = "".join(",".join(r) + "\n" for r in rows)
    return {"rows": len(rows), "sha256": hashlib.sha256(text.encode()).hexdigest(),
            "elementwise": [r[1:] for r in rows if r[0] == "elementwise"]}


if __name__ == "__main__":
    out = {case_id(*c): rebuild_launches(*c) for c in CASES}
    with open(JSON_PATH, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {JSON_PATH}: {len(out)} passes, {sum(v['rows'] for v in out.values())} launches")
