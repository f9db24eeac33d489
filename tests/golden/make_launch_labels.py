#!/usr/bin/env python3
"""Generate tests/golden/launch_labels.json: which contraction kernels one forward + backward pass of every network
launches, in order -- the (family, label) columns of the context profile for the rows of the conv_igemm_mfma,
wgrad_igemm_mfma and conv_direct_valu families.  A label names the kernel, the shape, the arithmetic and the split count
(the direct kernels carry none: their row says that they ran).

Run from the repository root on an MI355X:

    python tests/golden/make_launch_labels.py

The committed fixture is a regression pin of the kernel choice: it was written with the library of the commit BEFORE
conv / wgrad kernel selection moved into csrc/dispatch.cpp (that commit's librfi_hip.so, picked with RFI_HIP_LIB), never
with the library it is meant to check.  Regenerate it only together with a deliberate change of a gate, a tile or a plan.
tests/test_gpu_launch_labels.py imports CASES and launch_labels from this file.

Cases: Cnn3, the ResNet-encoder U-Net, the mask head, the RPN head, the box head and the ResNet-50-FPN backbone, each at the
smallest case its own GPU test file uses, in every compute mode.  The U-Net and the backbone already span maps from 32
pixels down to 2 and 1 there, so both ends of the tile and small-map gates are taken; the ResNet-encoder U-Net also runs
at 16 features, the narrowest width with the bfloat16 plane flow.  Cnn3 and that U-Net run at 32 features too, where the
first layer takes the stem kernels, whose weight gradient sizes its grid (the "split" of its label) to the slab workspace
the whole model asked for.  The networks with ONE map size cannot hold a 32-pixel
and a sub-8-pixel map in one pass: they get a second shape at 32+ pixels and a third under 8.  RPNHead takes anchor
counts in multiples of 4, so its 5 A outputs always satisfy the width half of ConvHeadModel::head_on_mfma(); the other side
of that gate is taken by the float32_mfma mode (here) and by the mask head's single output channel.
"""
import json
import os
import sys
import tempfile
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
JSON_PATH = os.path.join(HERE, "launch_labels.json")

MODES = ("float32", "float32_mfma", "bfloat16", "float32_planes", "bfloat16_regs")
FAMILIES = ("conv_igemm_mfma", "wgrad_igemm_mfma", "conv_direct_valu")

Case = namedtuple("Case", "model args shape")       # shape: (n, h, w) of the input map; box head: (rois,)
NETS = (
    Case("cnn3", (3, 1, 16), (4, 32, 32)), Case("cnn3", (3, 1, 16), (1, 40, 36)), Case("cnn3", (3, 1, 16), (2, 6, 5)),
    Case("cnn3", (3, 1, 32), (4, 32, 32)),
    Case("resnet_unet", (3, 1, 8), (3, 32, 32)), Case("resnet_unet", (3, 1, 16), (2, 64, 64)), Case("resnet_unet", (3, 1, 32), (2, 64, 64)),
    Case("mask_head", (16, 1, 4), (5, 14, 14)), Case("mask_head", (16, 1, 4), (2, 32, 32)), Case("mask_head", (16, 1, 4), (3, 3, 3)),
    Case("rpn_head", (16, 4, 1), (2, 8, 8)), Case("rpn_head", (16, 4, 1), (1, 24, 40)), Case("rpn_head", (16, 4, 1), (2, 4, 4)),
    Case("box_head", (8, 3, 32, 5), (37,)), Case("box_head", (16, 7, 64, 2), (96,)),
    Case("backbone", (3, 8, 16), (2, 64, 64)),
)
CASES = tuple((c, mode) for c in NETS for mode in MODES)


def case_id(case, mode):
    return f"{case.model}{'_'.join(map(str, case.args))}-{'x'.join(map(str, case.shape))}-{mode}"


def _pass(case, mode):
    """-> a callable that runs one forward + backward pass of the case (the model is built and loaded outside the profile)"""
    from rfi_toolbox_amd import models as M
    rng = np.random.default_rng(7)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    if case.model == "box_head":
        c, res, hid, k1 = case.args
        m = M.BoxHead(c, res, hid, k1).train().set_compute_dtype(mode)
        x, d = f32(case.shape[0], res, res, c), f32(case.shape[0], 5 * k1)
        return lambda: (m.forward_rois(x), m.backward(x, d))
    n, h, w = case.shape
    if case.model == "rpn_head":
        c, a, layers = case.args
        m = M.RPNHead(c, a, layers).train().set_compute_dtype(mode)
        x, d = f32(n, h, w, c), f32(n, h, w, 5 * a)
        return lambda: (m.forward_nhwc(x), m.backward(x, d))
    if case.model == "backbone":
        m = M.ResNet50FPN(*case.args).set_compute_dtype(mode)
        x = f32(n, h, w, case.args[0])
        d = [f32(n, h >> (2 + i), w >> (2 + i), case.args[2]) for i in range(5)]
        return lambda: (m.forward_features(x), m.backward(x, d))
    cls = {"cnn3": M.SimpleCNN, "resnet_unet": M.UNetResNet18, "mask_head": M.MaskHead}[case.model]
    m = cls(*case.args).train().set_compute_dtype(mode)
    up = 2 if case.model == "mask_head" else 1
    x, y = f32(n, h, w, case.args[0]), (rng.random((n, up * h, up * w)) > 0.7).astype(np.uint8)
    return lambda: m.forward_backward(x, y)


def launch_labels(case, mode):
    """-> the ordered [family, label] rows of the contraction families for one forward + backward pass"""
    from rfi_toolbox_amd.runtime import Context
    fn = _pass(case, mode)
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
    return [[r[1], r[2]] for r in rows if r[1] in FAMILIES]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    out = {case_id(c, mode): launch_labels(c, mode) for c, mode in CASES}
    with open(JSON_PATH, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {JSON_PATH}: {len(out)} passes, {sum(len(v) for v in out.values())} launches")
