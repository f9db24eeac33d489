"""The detector's three small networks stage by stage: the mask head and the RPN head (ConvHeadModel, model_mask.cpp) and the box head
(BoxHeadModel, model_mlp.cpp).  Importable without a GPU: test_head_stages_host.py runs the checker on a CPU stand-in and on
mutations of it, test_gpu_head_stages.py runs it on the tensors the device leaves behind (``debug_tensor``: "y.<i>", "u", "dy.<i>",
"du", "dx", "logits", "dlogits").  Method, criteria and constants are those of tests/unet_bf16_stages.py (EPS, K_CONTRACTION, Criteria,
Finding, wgrad_stage, rne ...), imported and not restated.

METHOD: teacher forcing.  Every launch of forward_pass / backward_pass reads its inputs from HBM and all of them are stored, so a
float64 oracle of ONE launch, fed the device's own stored inputs, differs from the stored output by that launch's own rounding.

THE STAGE TABLE is ``stage_table(case, mode)``, one row per launch in launch order (<i> = 0 .. L-1; "up" rows: the mask head only):

  conv.<i>          y.<i> = conv3x3 (FC: 1x1) of relu(y.<i-1>) (i = 0: x) + bias                                   f32
  up                u = ConvTranspose2d(k 2, s 2) of relu(y.<L-1>) + bias                                          f32
  head              logits = W relu(u | y.<L-1>) + b: the per-pixel kernel (head_fwd_vec) or, where
                    head_on_mfma(), a 1x1 conv on the conv kernels                                                  f32
  loss_bwd          dlogits of the mask head's own loss (mean BCE with logits = focal, gamma 0), held to
                    loss_step_cases.grad_bound, the bound test_gpu_loss_step.py holds that backward to.           loss
                    (RPN / box head, mask head with K > 1: dlogits is a stored input; row "dlogits": the copy is exact)
  head_bwd:dw :db   dW = dlogits^T relu(.), db = column sums of dlogits                                            f32 / sums
  head_bwd:da       du | dy.<L-1> = (u | y.<L-1> > 0) * (dlogits W): head input gradient + relu_bwd                f32, 0 where masked
  up_bwd:db :dw     channel sums of du; the transposed conv's weight gradient from relu(y.<L-1>) and du            sums / f32
  up_bwd:da         dy.<L-1> = (y.<L-1> > 0) * adjoint of the transposed conv applied to du                        f32, 0 where masked
  conv_bwd.<i>:db :dw   channel sums of dy.<i>; weight gradient from relu(y.<i-1>) | x and dy.<i>                  sums / f32
  conv_bwd.<i>:da   dy.<i-1> = (y.<i-1> > 0) * dgrad of dy.<i>;  i = 0: dx = dgrad of dy.0 (no mask)               f32, 0 where masked

relu_bwd_kernel tests ``y > 0`` on the STORED float32 raw output, scale = 1 and shift = 0, so every mask is decided exactly: no
undecided element can exist, and the masked rows demand an exact 0 where the mask is 0.  A random float32 conv output is never
exactly 0, so `>` and `>=` could not be told apart: init_params() makes output channel 1 of every 3x3 / FC / transposed layer DEAD
(zero filter, zero bias).  Its stored raw output is exactly 0 while the gradient that arrives there is not; ``Checker.zeros`` counts
those elements and the tests assert that there are some.

PER-MODE ORACLES.  "bfloat16": float32 storage, operands rounded to bfloat16 in registers -- the oracle rounds BOTH operands of
every contraction (RNE) and then applies the same f32 criterion.  The per-pixel head kernels (head_fwd_vec / head_bwd_vec) read
float32 and round nothing, in every mode; bias adds and channel sums are float32 everywhere.  "float32" (3 x bf16 pieces) and
"float32_mfma" (native float32 MFMA): operands unrounded.

CRITERIA: f32 and sums |g - e| <= k eps S with k = K_CONTRACTION = 16 (e the float64 value, S the sum of the absolute values of
its terms), the project's own limit; above 64 is certainly a bug.  loss: max |dlogits - g64| / grad_bound <= 1.

SEQUENCES (``SEQUENCES``): one model run at several RoI counts / map sizes and back; every run stage-checked, the last run equal
to the first bit for bit; the RPN head's accumulated gradient against the float64 sum of the per-run oracles within the summed
bounds.

MEASURED on an MI355X (the HEADSTAGES lines of test_gpu_head_stages.py): the worst ratio per class and the tensor it belongs to,
next to the CPU stand-in's (another summation order).  loss: max |dlogits - g64| over loss_step_cases.grad_bound.
  run                                   f32 (k 16): device / stand-in        sums (k 16): device / stand-in     loss | dlogits copy
  mask_c16_k1_l4_5x14x14/float32        n/a / 4.33                           n/a / 0.98                         loss n/a / 0.50
  mask_c16_k1_l4_5x14x14/float32_mfma   n/a / 4.33                           n/a / 0.98                         loss n/a / 0.50
  mask_c32_k1_l2_3x14x14/float32        n/a / 3.95                           n/a / 0.56                         loss n/a / 0.48
  mask_c32_k1_l2_3x14x14/bfloat16       n/a / 2.54                           n/a / 0.64                         loss n/a / 0.46
  mask_c8_k1_l1_2x14x14/float32         n/a / 2.81                           n/a / 0.25                         loss n/a / 0.45
  mask_c12_k3_l2_2x10x6/float32         n/a / 2.61                           n/a / 0.51                         copy exact
  mask_c16_k8_l1_1x7x7/float32          n/a / 2.98                           n/a / 0.93                         copy exact
  mask_c16_k8_l1_1x7x7/bfloat16         n/a / 1.31                           n/a / 0.58                         copy exact
  mask_c16_k8_l1_1x7x7/float32_mfma     n/a / 2.98                           n/a / 0.93                         copy exact
  mask_c64_k1_l8_1x8x8/float32          n/a / 5.14                           n/a / 1.34                         loss n/a / 0.37
  rpn_c16_a4_l1_2x8x8/float32           n/a / 3.77                           n/a / 0.73                         copy exact
  rpn_c16_a4_l1_2x8x8/float32_mfma      n/a / 3.77                           n/a / 0.73                         copy exact
  rpn_c16_a4_l1_2x8x8/bfloat16          n/a / 1.47                           n/a / 0.66                         copy exact
  rpn_c32_a4_l2_1x24x20/float32         n/a / 3.54                           n/a / 1.02                         copy exact
  rpn_c8_a4_l1_2x4x4/float32            n/a / 2.73                           n/a / 1.15                         copy exact
  rpn_c16_a8_l1_2x1x1/float32           n/a / 2.15                           n/a / 0.00                         copy exact
  rpn_c16_a8_l1_2x2x2/float32           n/a / 2.21                           n/a / 1.28                         copy exact
  box_c16_r7_h64_k2_96/float32          n/a / 4.40                           n/a / 2.19                         copy exact
  box_c16_r7_h64_k2_96/float32_mfma     n/a / 4.40                           n/a / 2.19                         copy exact
  box_c16_r7_h64_k2_96/bfloat16         n/a / 2.91                           n/a / 1.35                         copy exact
  box_c8_r3_h32_k5_37/float32           n/a / 3.21                           n/a / 0.85                         copy exact
  box_c8_r3_h32_k5_37/bfloat16          n/a / 2.70                           n/a / 0.95                         copy exact
  box_c4_r1_h4_k2_1/float32             n/a / 1.08                           n/a / 0.00                         copy exact
  box_c4_r3_h36_k2_31/float32           n/a / 3.01                           n/a / 1.50                         copy exact
  box_c4_r3_h36_k2_32/float32           n/a / 2.85                           n/a / 0.68                         copy exact
  box_c4_r3_h36_k2_33/float32           n/a / 2.92                           n/a / 0.80                         copy exact

FOUND: nothing on the CPU stand-in.  The device columns above read n/a until the HEADSTAGES lines of a run on an MI355X are copied in;
a ratio above 16 there is a finding to explain from the code, not a bound to raise.

MUTATIONS of the stand-in (``MUTATIONS``; test_head_stages_host.py has the table of which of them the whole-head criteria of
test_gpu_mask_head.py would have noticed).
"""
import re
from collections import OrderedDict, namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import loss_step_cases as LS
import unet_bf16_stages as S
from unet_bf16_stages import EPS, K_CONTRACTION, K_ELEM, Criteria, Finding, rne, trunc_bf16, wgrad_stage  # noqa: F401

TAG = "HEADSTAGES"
MODES = ("float32", "float32_mfma", "bfloat16")
Case = namedtuple("Case", "id head args shape modes seed covers")
F32, MF, BF = "float32", "float32_mfma", "bfloat16"

CASES = [
    # mask head (C, K, L), R x h x w
    Case("mask_c16_k1_l4_5x14x14", "mask", (16, 1, 4), (5, 14, 14), (F32, MF), 0, ("conv_ws:yes", "up_gemm_ws:no", "depth:4", "ragged:yes")),
    Case("mask_c32_k1_l2_3x14x14", "mask", (32, 1, 2), (3, 14, 14), (F32, BF), 1, ("up_gemm_ws:yes", "depth:2", "head:pixel1")),
    Case("mask_c8_k1_l1_2x14x14", "mask", (8, 1, 1), (2, 14, 14), (F32,), 2, ("c16:no", "conv_ws:no", "depth:1")),
    Case("mask_c12_k3_l2_2x10x6", "mask", (12, 3, 2), (2, 10, 6), (F32,), 3, ("ragged:yes", "map:sub8", "classes:3", "head:pixelK")),
    Case("mask_c16_k8_l1_1x7x7", "mask", (16, 8, 1), (1, 7, 7), (F32, BF, MF), 4, ("map:sub8", "classes:8", "head:conv", "head:pixelK")),
    Case("mask_c64_k1_l8_1x8x8", "mask", (64, 1, 8), (1, 8, 8), (F32,), 5, ("depth:8", "map:tile8", "conv_ws:yes")),
    # RPN head (C, A, L), n x h x w
    Case("rpn_c16_a4_l1_2x8x8", "rpn", (16, 4, 1), (2, 8, 8), (F32, MF, BF), 6, ("head:conv", "head:pixelK", "map:tile8")),
    Case("rpn_c32_a4_l2_1x24x20", "rpn", (32, 4, 2), (1, 24, 20), (F32,), 7, ("ragged:yes", "depth:2")),
    Case("rpn_c8_a4_l1_2x4x4", "rpn", (8, 4, 1), (2, 4, 4), (F32,), 8, ("map:sub8", "c16:no")),
    Case("rpn_c16_a8_l1_2x1x1", "rpn", (16, 8, 1), (2, 1, 1), (F32,), 9, ("map:1x1",)),
    Case("rpn_c16_a8_l1_2x2x2", "rpn", (16, 8, 1), (2, 2, 2), (F32,), 10, ("map:2x2",)),
    # box head (C, res, hidden, K1), R
    Case("box_c16_r7_h64_k2_96", "box", (16, 7, 64, 2), (96,), (F32, MF, BF), 11, ("layout:32", "fc_gemm_ws:yes")),
    Case("box_c8_r3_h32_k5_37", "box", (8, 3, 32, 5), (37,), (F32, BF), 12, ("layout:rows", "in16:no")),
    Case("box_c4_r1_h4_k2_1", "box", (4, 1, 4, 2), (1,), (F32,), 13, ("rows:1", "layout:rows", "fc_gemm_ws:no")),
    Case("box_c4_r3_h36_k2_31", "box", (4, 3, 36, 2), (31,), (F32,), 14, ("hidden16:no", "layout:rows")),
    Case("box_c4_r3_h36_k2_32", "box", (4, 3, 36, 2), (32,), (F32,), 14, ("hidden16:no", "layout:32")),
    Case("box_c4_r3_h36_k2_33", "box", (4, 3, 36, 2), (33,), (F32,), 14, ("hidden16:no", "layout:rows")),
]
BY_ID = OrderedDict((c.id, c) for c in CASES)
RUNS = [(c.id, m) for c in CASES for m in c.modes]

# (base case, the shapes one model runs in order; the last equals the first)
SEQUENCES = OrderedDict([
    ("mask", ("mask_c16_k1_l4_5x14x14", [(5, 14, 14), (37, 14, 14), (1, 14, 14), (5, 14, 14)])),
    ("box", ("box_c16_r7_h64_k2_96", [(96,), (37,), (1,), (96,)])),
    ("rpn", ("rpn_c16_a4_l1_2x8x8", [(2, 16, 16), (2, 8, 8), (2, 1, 1), (2, 16, 16)])),
])

ALL_GATE_VALUES = ["mode:float32", "mode:float32_mfma", "mode:bfloat16", "head:pixel1", "head:pixelK", "head:conv",
                   "conv_ws:yes", "conv_ws:no", "up_gemm_ws:yes", "up_gemm_ws:no", "fc_gemm_ws:yes", "fc_gemm_ws:no", "c16:no",
                   "in16:no", "hidden16:no", "map:sub8", "map:tile8", "map:1x1", "map:2x2", "ragged:yes", "classes:1", "classes:3",
                   "classes:8", "depth:1", "depth:2", "depth:4", "depth:8", "layout:32", "layout:rows", "rows:1"]


# ------------------------------------------------------------------------------------------------------------ geometry
def depth(c):
    return 2 if c.head == "box" else c.args[2]


def out_channels(c):
    return c.args[1] if c.head == "mask" else 5 * c.args[1] if c.head == "rpn" else 5 * c.args[3]


def widths(c):
    """(input channels of layer 0, hidden width)."""
    return (c.args[0] * c.args[1] ** 2, c.args[2]) if c.head == "box" else (c.args[0], c.args[0])


def head_on_mfma(c, mode):
    """ConvHeadModel::head_on_mfma(): out_ch >= 8 && out_ch % 4 == 0 && in_ch % 4 == 0 && arith != F32 (the box head: never)."""
    o = out_channels(c)
    return c.head != "box" and o >= 8 and o % 4 == 0 and mode != MF


def gate_values(c):
    v = {"depth:%d" % depth(c)}
    o, (cin, hid) = out_channels(c), widths(c)
    for mode in c.modes:
        v.add("mode:" + mode)
        v.add("head:conv" if head_on_mfma(c, mode) else "head:pixel1" if o == 1 else "head:pixelK")
    if c.head == "box":
        r = c.shape[0]
        v.add("layout:32" if r % 32 == 0 else "layout:rows")                 # layout_of(rows)
        v.add("fc_gemm_ws:yes" if hid % 16 == 0 else "fc_gemm_ws:no")        # gemm_ws_eligible of fc7: Cin % 16
        if cin % 16:
            v.add("in16:no")
        if hid % 16:
            v.add("hidden16:no")
        if r == 1:
            v.add("rows:1")
        return v
    n, h, w = c.shape
    v.add("conv_ws:yes" if h >= 8 and w >= 8 and cin % 16 == 0 else "conv_ws:no")      # conv_ws_eligible
    if cin % 16:
        v.add("c16:no")
    if h < 8 or w < 8:
        v.add("map:sub8")
    if (h, w) in ((8, 8), (1, 1), (2, 2)):
        v.add({8: "map:tile8", 1: "map:1x1", 2: "map:2x2"}[h])
    if max(h, w) >= 8 and (h % 8 or w % 8):
        v.add("ragged:yes")
    if c.head == "mask":
        v.add("up_gemm_ws:yes" if cin % 32 == 0 else "up_gemm_ws:no")       # gemm_ws_eligible, transposed forward: Cout % 32
        v.add("classes:%d" % o)
    return v


def own_loss(c):
    """The mask head with one class computes its own loss; every other head is driven by a given dlogits."""
    return c.head == "mask" and c.args[1] == 1


def keys(c):
    """Parameter keys of the checker (library layout) -> the library's entry names."""
    out = OrderedDict()
    for i in range(depth(c)):
        nm = {"mask": "mask_fcn%d" % (i + 1), "rpn": "conv.%d.0" % i, "box": "fc%d" % (6 + i)}[c.head]
        out["w.%d" % i], out["b.%d" % i] = nm + ".weight", nm + ".bias"
    if c.head == "mask":
        out["up.w"], out["up.b"] = "conv5_mask.weight", "conv5_mask.bias"
    hd = "mask_fcn_logits" if c.head == "mask" else "head"
    out["head.w"], out["head.b"] = hd + ".weight", hd + ".bias"
    return out


def tensor_names(c):
    L = depth(c)
    up = ["u", "du"] if c.head == "mask" else []
    return ["y.%d" % i for i in range(L)] + ["dy.%d" % i for i in range(L)] + up + ["logits", "dlogits", "dx"]


def shape_of(c, name, shape=None):
    shape = shape or c.shape
    cin, hid = widths(c)
    n, h, w = (shape[0], 1, 1) if c.head == "box" else shape
    base = name.split(".")[0]
    if base in ("x", "dx"):
        return (n, h, w, cin)
    if base in ("u", "du"):
        return (n, 2 * h, 2 * w, hid)
    if base in ("logits", "dlogits"):
        s = 2 if c.head == "mask" else 1
        return (n, s * h, s * w, out_channels(c))
    return (n, h, w, hid)


# ------------------------------------------------------------------------------------------------------------ parameters, inputs
def to_lib(c, d):
    """Tensors under the torch modules' names (parameters or their gradients) -> the checker's keys in the library's layout:
    the RPN / box predictors stacked into one head, fc6's columns from (c, h, w) to (h, w, c) order, FC weights as 1x1 filters."""
    d = {k: torch.as_tensor(v) for k, v in d.items()}
    out = OrderedDict()
    for k, nm in keys(c).items():
        if k.startswith("head.") and c.head != "mask":
            a, b = ("cls_logits", "bbox_pred") if c.head == "rpn" else ("cls_score", "bbox_pred")
            suffix = nm[len("head"):]
            t = torch.cat([d[a + suffix], d[b + suffix]], 0)
        else:
            t = d[nm]
        if c.head == "box" and t.ndim == 2:
            if k == "w.0":
                C, r = c.args[0], c.args[1]
                t = t.reshape(t.shape[0], C, r, r).permute(0, 2, 3, 1).reshape(t.shape[0], -1)
            t = t[:, :, None, None]
        elif k == "head.w":
            t = t.reshape(t.shape[0], -1, 1, 1)
        out[k] = np.ascontiguousarray(t.detach().numpy())
    return out


def init_params(c, dead=True):
    """-> (state under the oracle modules' names, the same in the library's layout).  Output channel 1 of every hidden layer is
    dead (module docstring); dead=False: the modules' default initialisation, as test_gpu_mask_head.py draws it."""
    from oracle import mask_head_ref as mref
    if c.head == "mask":
        st = mref.init_state(*c.args, seed=c.seed)
    elif c.head == "rpn":
        st = mref.rpn_init_state(*c.args, seed=c.seed)
    else:
        torch.manual_seed(c.seed)
        st = OrderedDict((k, v.detach().clone()) for k, v in mref.BoxHeadModule(*c.args).state_dict().items())
    for k, nm in keys(c).items():
        if k.startswith("head.") or not dead:
            continue
        if k == "up.w":
            st[nm][:, 1] = 0                     # ConvTranspose2d: [cin][cout][2][2]
        else:
            st[nm][1] = 0
    return st, to_lib(c, st)


def inputs(c, shape=None, seed_offset=0):
    """x NHWC (box head: [R, res, res, C]) and what drives the backward pass: labels "y" (mask head, one class), a given
    "dlogits" (mask head, several classes), the samplers' "labels" / "targets" (RPN, box)."""
    shape = shape or c.shape
    rng = np.random.default_rng(1000 + c.seed + 100 * seed_offset)
    if c.head == "box":
        C, res, _, k1 = c.args
        r = shape[0]
        lab = rng.integers(0, k1, r).astype(np.int32)
        lab[0] = 1
        return {"x": rng.standard_normal((r, res, res, C)).astype(np.float32), "labels": lab,
                "targets": (rng.standard_normal((r, 4)) * 0.3).astype(np.float32)}
    n, h, w = shape
    out = {"x": rng.standard_normal((n, h, w, c.args[0])).astype(np.float32)}
    if c.head == "rpn":
        a = c.args[1]
        lab = rng.choice(np.array([-1] * 8 + [0, 0, 1], np.int8), n * h * w * a)
        lab[:3] = (1, 0, -1)
        out["labels"], out["targets"] = lab, (rng.standard_normal((n * h * w * a, 4)) * 0.3).astype(np.float32)
    elif own_loss(c):
        out["y"] = (rng.random((n, 2 * h, 2 * w)) > 0.6).astype(np.uint8)
    else:
        k = c.args[1]
        out["dlogits"] = (rng.standard_normal((n, 2 * h, 2 * w, k)) / (n * 4 * h * w * k)).astype(np.float32)
    return out


def flat_x(c, x):
    """The input as the library sees it: the box head's RoI features flattened in (h, w, c) order to [R, 1, 1, D]."""
    x = np.asarray(x, np.float32)
    return np.ascontiguousarray(x.reshape(x.shape[0], 1, 1, -1)) if c.head == "box" else x


# ------------------------------------------------------------------------------------------------------------ float64 stage functions
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).permute(0, 3, 1, 2).contiguous()


def _n(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _p(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def conv_stage(x, w, b, pad):
    xt, wt, bt = _t(x), _p(w), _p(b)
    return _n(F.conv2d(xt, wt, bt, padding=pad)), _n(F.conv2d(xt.abs(), wt.abs(), bt.abs(), padding=pad))


def dgrad_stage(dy, w, pad):
    dt, wt = _t(dy), _p(w)
    return _n(F.conv_transpose2d(dt, wt, padding=pad)), _n(F.conv_transpose2d(dt.abs(), wt.abs(), padding=pad))


def convt_stage(a, w, b):
    at, wt, bt = _t(a), _p(w), _p(b)
    return _n(F.conv_transpose2d(at, wt, bt, stride=2)), _n(F.conv_transpose2d(at.abs(), wt.abs(), bt.abs(), stride=2))


def convt_dgrad_stage(du, w):
    dt, wt = _t(du), _p(w)
    return _n(F.conv2d(dt, wt, stride=2)), _n(F.conv2d(dt.abs(), wt.abs(), stride=2))


def convt_wgrad_stage(du, a, wshape):
    dt, at = _t(du), _t(a)
    return (torch.nn.grad.conv2d_weight(dt, wshape, at, stride=2).numpy(),
            torch.nn.grad.conv2d_weight(dt.abs(), wshape, at.abs(), stride=2).numpy())


def relu(a):
    return np.maximum(np.asarray(a, np.float32), np.float32(0))


# ------------------------------------------------------------------------------------------------------------ the checker
Row = namedtuple("Row", "stage launch ins outs klass")


def stage_table(c, mode):
    L, up, conv = depth(c), c.head == "mask", head_on_mfma(c, mode)
    k = "FC (1x1 conv)" if c.head == "box" else "conv3x3"
    rows = [Row("conv.%d" % i, k, ["y.%d" % (i - 1) if i else "x", "w.%d" % i, "b.%d" % i], ["y.%d" % i], "f32") for i in range(L)]
    top = "y.%d" % (L - 1)
    hin, hd = ("u", "du") if up else (top, "dy.%d" % (L - 1))
    if up:
        rows.append(Row("up", "transposed conv", [top, "up.w", "up.b"], ["u"], "f32"))
    rows.append(Row("head", "conv1x1" if conv else "head_fwd", [hin, "head.w", "head.b"], ["logits"], "f32"))
    if own_loss(c):
        rows.append(Row("loss_bwd", "focal_bwd", ["logits", "(labels)"], ["dlogits"], "loss"))
    else:
        rows.append(Row("dlogits", "copy", ["(given)"], ["dlogits"], "elem"))
    name = "wgrad1x1 / channel_sum / conv1x1" if conv else "head_bwd"
    rows.append(Row("head_bwd:dw", name, [hin, "dlogits"], ["grad head.w"], "f32"))
    rows.append(Row("head_bwd:db", name, ["dlogits"], ["grad head.b"], "sums"))
    rows.append(Row("head_bwd:da", name + " + relu_bwd", ["dlogits", "head.w", hin], [hd], "f32"))
    if up:
        rows.append(Row("up_bwd:db", "channel_sum", ["du"], ["grad up.b"], "sums"))
        rows.append(Row("up_bwd:dw", "transposed-conv wgrad", [top, "du"], ["grad up.w"], "f32"))
        rows.append(Row("up_bwd:da", "transposed-conv dgrad + relu_bwd", ["du", "up.w", top], ["dy.%d" % (L - 1)], "f32"))
    for i in range(L - 1, -1, -1):
        below = "y.%d" % (i - 1) if i else "x"
        rows.append(Row("conv_bwd.%d:db" % i, "channel_sum", ["dy.%d" % i], ["grad b.%d" % i], "sums"))
        rows.append(Row("conv_bwd.%d:dw" % i, "wgrad", [below, "dy.%d" % i], ["grad w.%d" % i], "f32"))
        rows.append(Row("conv_bwd.%d:da" % i, "dgrad + relu_bwd" if i else "dgrad", ["dy.%d" % i, "w.%d" % i] + ([below] if i else []),
                        ["dy.%d" % (i - 1) if i else "dx"], "f32"))
    return rows


class Checker(Criteria):
    """Runs the stage table of one (case, mode) over a tensor dictionary T (device or stand-in): T[name] NHWC float32 arrays under
    the debug_tensor names and "x" (as flat_x gives it), T["grad"][key] the gradients in the library's layout, T["given"] the
    dlogits handed to the backward pass or T["y"] the labels.  ``P``: the parameters in the library's layout."""
    TAG = TAG

    def __init__(self, case, mode, P, T, run_id=None):
        super().__init__()
        self.c, self.mode, self.P, self.T = case, mode, P, T
        self.id = run_id or "%s/%s" % (case.id, mode)
        self.bf = mode == BF
        self.zeros = 0                    # stored raw outputs that are exactly 0 (the dead channels): where > and >= differ
        self.oracle = OrderedDict()       # gradient key -> (e, S) of this run
        self.nonfinite = [k for k in tensor_names(case) if not np.isfinite(T[k]).all()]
        self.nonfinite += ["grad " + k for k, v in T["grad"].items() if not np.isfinite(v).all()]

    def r(self, a, rounded=True):
        """An operand as the contraction reads it: bfloat16 (RNE) in the bfloat16 mode, else the float32 value."""
        a = np.asarray(a, np.float32)
        return (rne(a) if self.bf and rounded else a).astype(np.float64)

    def _grad(self, stage, klass, key, e, S):
        self.oracle[key] = (e, S)
        self.close(stage, klass, "grad " + key, self.T["grad"][key], e, S)

    def _masked(self, stage, out, raw, e, S):
        m = np.asarray(self.T[raw], np.float32) > 0
        self.zeros += int((np.asarray(self.T[raw]) == 0).sum())
        self.close(stage, "f32", out, self.T[out], e * m, S * m)

    def run(self):
        c, T, P, L = self.c, self.T, self.P, depth(self.c)
        pad = 0 if c.head == "box" else 1
        up, conv = c.head == "mask", head_on_mfma(c, self.mode)
        ax = (0, 1, 2)
        # ---- forward
        ins = [T["x"]] + [relu(T["y.%d" % i]) for i in range(L)]
        for i in range(L):
            e, S_ = conv_stage(self.r(ins[i]), self.r(P["w.%d" % i]), P["b.%d" % i], pad)
            self.close("conv.%d" % i, "f32", "y.%d" % i, T["y.%d" % i], e, S_)
        if up:
            e, S_ = convt_stage(self.r(ins[L]), self.r(P["up.w"]), P["up.b"])
            self.close("up", "f32", "u", T["u"], e, S_)
        hin_name, hd_name = ("u", "du") if up else ("y.%d" % (L - 1), "dy.%d" % (L - 1))
        a = self.r(relu(T[hin_name]), conv)
        W = self.r(P["head.w"].reshape(out_channels(c), -1), conv)
        b = P["head.b"].astype(np.float64)
        self.close("head", "f32", "logits", T["logits"], a @ W.T + b, np.abs(a) @ np.abs(W).T + np.abs(b))
        # ---- the loss turn-around
        if own_loss(c):
            x64, t64 = torch.from_numpy(T["logits"].reshape(-1).astype(np.float64)), torch.from_numpy(T["y"].reshape(-1).astype(np.float64))
            g64 = LS.focal_ref(x64, t64, -1.0, 0.0)[1].numpy()
            g32 = LS.focal_ref(x64.float(), t64.float(), -1.0, 0.0)[1].double().numpy()
            bound = LS.grad_bound(float(np.abs(g32 - g64).max()), g64)
            d = np.asarray(T["dlogits"], np.float64).reshape(-1)
            self._add("loss_bwd", "loss", "dlogits", float(np.abs(d - g64).max()) / bound if np.isfinite(d).all() else np.inf, 1.0)
        else:
            self.exact("dlogits", "dlogits", T["dlogits"], np.asarray(T["given"], np.float32).reshape(T["dlogits"].shape))
        # ---- the head's backward
        dl32 = np.asarray(T["dlogits"], np.float32)
        dl = self.r(dl32, conv).reshape(-1, out_channels(c))
        a2 = a.reshape(-1, a.shape[-1])
        self._grad("head_bwd:dw", "f32", "head.w", (dl.T @ a2).reshape(P["head.w"].shape), (np.abs(dl).T @ np.abs(a2)).reshape(P["head.w"].shape))
        d64 = dl32.astype(np.float64).reshape(-1, out_channels(c))
        self._grad("head_bwd:db", "sums", "head.b", d64.sum(0), np.abs(d64).sum(0))
        shp = T[hin_name].shape
        self._masked("head_bwd:da", hd_name, hin_name, (dl @ W).reshape(shp), (np.abs(dl) @ np.abs(W)).reshape(shp))
        # ---- the transposed conv
        if up:
            du = np.asarray(T["du"], np.float64)
            self._grad("up_bwd:db", "sums", "up.b", du.sum(ax), np.abs(du).sum(ax))
            e, S_ = convt_wgrad_stage(self.r(T["du"]), self.r(ins[L]), P["up.w"].shape)
            self._grad("up_bwd:dw", "f32", "up.w", e, S_)
            e, S_ = convt_dgrad_stage(self.r(T["du"]), self.r(P["up.w"]))
            self._masked("up_bwd:da", "dy.%d" % (L - 1), "y.%d" % (L - 1), e, S_)
        # ---- the 3x3 / FC layers
        for i in range(L - 1, -1, -1):
            dy = np.asarray(T["dy.%d" % i], np.float64)
            st = "conv_bwd.%d" % i
            self._grad(st + ":db", "sums", "b.%d" % i, dy.sum(ax), np.abs(dy).sum(ax))
            e, S_ = wgrad_stage(self.r(ins[i]), self.r(T["dy.%d" % i]), P["w.%d" % i].shape, 1, pad)
            self._grad(st + ":dw", "f32", "w.%d" % i, e, S_)
            e, S_ = dgrad_stage(self.r(T["dy.%d" % i]), self.r(P["w.%d" % i]), pad)
            if i:
                self._masked(st + ":da", "dy.%d" % (i - 1), "y.%d" % (i - 1), e, S_)
            else:
                self.close(st + ":da", "f32", "dx", T["dx"], e, S_)
        return self

    def unchecked_rows(self):
        """Rows of the stage table without a finding, and findings without a row: both must be empty."""
        want, got = {r.stage for r in stage_table(self.c, self.mode)}, {f.stage for f in self.findings}
        return sorted(want ^ got)

    def report(self):
        return [f.line(self.id, self.TAG) for f in self.worst_per_class().values()]


def check(case, mode, P, T, run_id=None):
    return Checker(case, mode, P, T, run_id).run()


def check_accumulated(c, mode, runs, total):
    """The gradient accumulated over `runs` (Checkers of the single passes) against the float64 sum of their oracles, within the
    summed bounds.  -> a Criteria with one finding per parameter."""
    out = Criteria()
    for k in runs[0].oracle:
        e, S_ = sum(r.oracle[k][0] for r in runs), sum(r.oracle[k][1] for r in runs)
        out.close("accumulate", "sums" if k.startswith("b.") or k.endswith(".b") else "f32", "grad " + k, total[k], e, S_)
    return out


# ------------------------------------------------------------------------------------------------------------ the stand-in
def _bf32(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _trunc32(t):
    return torch.from_numpy(trunc_bf16(t.numpy()).copy())


def loss_and_dlogits(c, logits, inp):
    """float32, on the CPU: the loss value(s) and d loss / d logits of a head whose loss is not given.  logits NHWC torch."""
    from oracle import mask_head_ref as mref
    if own_loss(c):
        t = torch.from_numpy(inp["y"].reshape(-1).astype(np.float32))
        loss, g = LS.focal_ref(logits.reshape(-1), t, -1.0, 0.0)
        return (float(loss),), g.reshape(logits.shape)
    if c.head == "mask":
        return (), torch.from_numpy(inp["dlogits"])
    lg = logits.detach().clone().requires_grad_(True)
    if c.head == "rpn":
        a, b = mref.rpn_loss_torch(lg, inp["labels"], inp["targets"], c.args[1])
    else:
        k1 = c.args[3]
        o = lg.reshape(-1, 5 * k1)
        a, b = mref.fastrcnn_loss_torch(o[:, :k1], o[:, k1:], inp["labels"], inp["targets"])
    g, = torch.autograd.grad(a + b, lg)
    return (float(a.detach()), float(b.detach())), g


MUTATIONS = OrderedDict([
    # name -> (what is wrong, the stages that must turn red -- a regular expression over the failed stage names)
    ("head_da_overwritten", ("the per-pixel head overwrites da instead of accumulating it for o > 0", r"head_bwd$")),
    ("relu_bwd_ge", ("relu_bwd masks with >= instead of >", r"(head_bwd|up_bwd|conv_bwd\.[1-9])$")),
    ("bias_before_mask", ("a bias gradient summed before the mask", r"(up_bwd|conv_bwd\.\d)$")),
    ("convt_taps_swapped", ("the transposed conv's taps written at each other's pixels", r"up$")),
    ("rpn_rows_swapped", ("the stacked RPN output with the cls / bbox rows swapped at A", r"head$")),
    ("fc6_chw", ("fc6 read in (c, h, w) instead of (h, w, c) order", r"conv\.0$")),
    ("operand_truncation", ("bfloat16 operands truncated instead of rounded to nearest even", r"(conv\.\d|up|head|head_bwd|up_bwd|conv_bwd\.\d)$")),
    ("box_rows_permuted", ("the box head's rows permuted by the [R / 32] x 32 layout", r"conv\.0$")),
    ("truncation_in_one_launch", ("bfloat16 operands truncated in ONE launch, the input gradient of layer 0", r"conv_bwd\.0$")),
])


class StandIn:
    """The same flow in float32 torch on the CPU, launch by launch, storing what the device stores.  ``mutate``: a name of
    MUTATIONS -- the value of ONE kind of launch is wrong, everything downstream is computed from the wrong stored tensor (as
    on a device with that bug), so the checker must turn red in that launch's rows and nowhere else."""

    def __init__(self, case, mode, P, inp, mutate=None):
        assert mutate is None or mutate in MUTATIONS
        self.c, self.mode, self.P, self.inp, self.mut = case, mode, P, inp, mutate
        self.loss = ()

    def run(self):
        c, mut, L = self.c, self.mut, depth(self.c)
        P = {k: torch.from_numpy(v) for k, v in self.P.items()}
        pad = 0 if c.head == "box" else 1
        up, conv, O = c.head == "mask", head_on_mfma(c, self.mode), out_channels(c)
        rb = (lambda t: t) if self.mode != BF else _trunc32 if mut == "operand_truncation" else _bf32
        rh = rb if conv else (lambda t: t)
        mask = (lambda y: (y >= 0).float()) if mut == "relu_bwd_ge" else (lambda y: (y > 0).float())
        nchw = lambda a: torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()  # noqa: E731
        T = {"x": flat_x(c, self.inp["x"]), "grad": OrderedDict()}
        for k in ("y", "dlogits"):
            if k in self.inp:
                T["y" if k == "y" else "given"] = self.inp[k]
        put = lambda name, t: T.__setitem__(name, np.ascontiguousarray(t.permute(0, 2, 3, 1).numpy()))  # noqa: E731
        # ---- forward
        acts, ys = [nchw(T["x"])], []
        for i in range(L):
            w = P["w.%d" % i]
            if mut == "fc6_chw" and i == 0 and c.head == "box":
                C, r = c.args[0], c.args[1]
                w = w.reshape(-1, r, r, C).permute(0, 3, 1, 2).reshape(w.shape).contiguous()       # the torch module's column order
            y = F.conv2d(rb(acts[i]), rb(w), P["b.%d" % i], padding=pad)
            if mut == "box_rows_permuted" and i == 0 and c.head == "box" and y.shape[0] % 32 == 0:
                y = y.reshape(-1, 32, *y.shape[1:]).transpose(0, 1).reshape(y.shape).contiguous()
            ys.append(y)
            acts.append(torch.relu(y))
            put("y.%d" % i, y)
        hin_raw = ys[-1]
        if up:
            wu = P["up.w"].flip(-1) if mut == "convt_taps_swapped" else P["up.w"]
            hin_raw = F.conv_transpose2d(rb(acts[L]), rb(wu), P["up.b"], stride=2)
            put("u", hin_raw)
        a = torch.relu(hin_raw)
        Wh = P["head.w"]
        logits = F.conv2d(rh(a), rh(Wh), P["head.b"])
        if mut == "rpn_rows_swapped" and c.head == "rpn":
            A = c.args[1]
            logits = torch.cat([logits[:, A:], logits[:, :A]], 1)
        put("logits", logits)
        self.loss, g = loss_and_dlogits(c, logits.permute(0, 2, 3, 1).contiguous(), self.inp)
        if not own_loss(c):
            T["given"] = np.ascontiguousarray(g.numpy())
        dl = g.reshape(T["logits"].shape).permute(0, 3, 1, 2).contiguous().float()
        put("dlogits", dl)
        # ---- the head's backward
        G = T["grad"]
        G["head.w"] = torch.nn.grad.conv2d_weight(rh(a), Wh.shape, rh(dl)).numpy()
        G["head.b"] = dl.sum((0, 2, 3)).numpy()
        if mut == "head_da_overwritten" and not conv and O > 1:
            da = dl[:, O - 1:O] * Wh[O - 1].reshape(1, -1, 1, 1)
        else:
            da = torch.nn.grad.conv2d_input(a.shape, rh(Wh), rh(dl))
        before = mut == "bias_before_mask"
        if up:
            du = da * mask(hin_raw)
            put("du", du)
            G["up.b"] = (da if before else du).sum((0, 2, 3)).numpy()
            G["up.w"] = torch.nn.grad.conv2d_weight(rb(du), P["up.w"].shape, rb(acts[L]), stride=2).numpy()
            da = F.conv2d(rb(du), rb(P["up.w"]), stride=2)
        for i in range(L - 1, -1, -1):
            dy = da * mask(ys[i])
            put("dy.%d" % i, dy)
            w = P["w.%d" % i]
            G["b.%d" % i] = (da if before else dy).sum((0, 2, 3)).numpy()
            G["w.%d" % i] = torch.nn.grad.conv2d_weight(rb(acts[i]), w.shape, rb(dy), padding=pad).numpy()
            r0 = _trunc32 if mut == "truncation_in_one_launch" and i == 0 and self.mode == BF else rb
            da = torch.nn.grad.conv2d_input(acts[i].shape, r0(w), r0(dy), padding=pad)
        put("dx", da)
        self.T = T
        return T


# ------------------------------------------------------------------------------------------------------------ the whole-head criteria
def _box_forward(st, x):
    """BoxHeadModule's forward on a state dictionary; under unet_ref.bf16_operands() the two FC layers round their operands
    (the predictors run on the per-pixel kernel, which rounds nothing)."""
    from oracle import unet_ref
    h = x.flatten(1)
    for nm in ("fc6", "fc7"):
        if unet_ref._BF16_OPERANDS:
            h = unet_ref._ConvBF16.apply(h[:, :, None, None], st[nm + ".weight"][:, :, None, None], st[nm + ".bias"], 0).flatten(1)
        else:
            h = F.linear(h, st[nm + ".weight"], st[nm + ".bias"])
        h = torch.relu(h)
    return F.linear(h, st["cls_score.weight"], st["cls_score.bias"]), F.linear(h, st["bbox_pred.weight"], st["bbox_pred.bias"])


def oracle(c, st, inp, dtype=torch.float32, bf16=False):
    """oracle/mask_head_ref.py through autograd -> {"loss": tuple, "logits": NHWC, "grad": checker keys, "dx": as flat_x}."""
    import contextlib
    from oracle import mask_head_ref as mref, unet_ref
    leaves = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in st.items())
    x = torch.from_numpy(inp["x"]).permute(0, 3, 1, 2).contiguous().to(dtype).requires_grad_(True)
    with (unet_ref.bf16_operands() if bf16 else contextlib.nullcontext()):
        if c.head == "mask":
            lg = mref.forward(leaves, x).permute(0, 2, 3, 1)
            if own_loss(c):
                loss = (mref.mask_loss(lg, torch.from_numpy(inp["y"]).to(dtype)),)
                total = loss[0]
            else:
                loss, total = (), (lg * torch.from_numpy(inp["dlogits"]).to(dtype)).sum()
        elif c.head == "rpn":
            lg = mref.rpn_forward(leaves, x)
            loss = mref.rpn_loss_torch(lg, inp["labels"], inp["targets"], c.args[1])
            total = loss[0] + loss[1]
        else:
            if bf16:
                cls, box = _box_forward(leaves, x)
            else:
                cls, box = torch.func.functional_call(mref.BoxHeadModule(*c.args).to(dtype), dict(leaves), (x,))
            lg = torch.cat([cls, box], 1)[:, None, None, :]
            loss = mref.fastrcnn_loss_torch(cls, box, inp["labels"], inp["targets"])
            total = loss[0] + loss[1]
        grads = torch.autograd.grad(total, list(leaves.values()) + [x])
    return {"loss": tuple(float(v.detach()) for v in loss), "logits": lg.detach().numpy(),
            "grad": to_lib(c, OrderedDict(zip(leaves.keys(), grads[:-1]))), "dx": flat_x(c, grads[-1].permute(0, 2, 3, 1).contiguous().numpy())}


def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def bf16_notices(c, st, inp, T, loss):
    """test_bf16_operand_mode's criterion: the loss to rel 2e-3, per gradient rel_same <= max(1.1 rel_arith, 1e-2) against the
    oracle under unet_ref.bf16_operands().  -> what it flags."""
    ob, o32 = oracle(c, st, inp, bf16=True), oracle(c, st, inp)
    out = ["loss.%d" % i for i, (g, w) in enumerate(zip(loss, ob["loss"])) if abs(g - w) > 2e-3 * abs(w)]
    got = dict(T["grad"], input=T["dx"])
    for k, g in dict(ob["grad"], input=ob["dx"]).items():
        rel_same, rel_arith = _rel(got[k], g), _rel(dict(o32["grad"], input=o32["dx"])[k], g)
        if not rel_same <= max(1.1 * rel_arith, 1e-2):
            out.append("grad " + k)
    return out


def whole_head_notices(c, mode, st, inp, T, loss):
    """The criteria test_gpu_mask_head.py holds each head to, evaluated on a tensor dictionary: test_gradients_vs_oracle (mask),
    test_rpn_head_step_and_proposals, test_box_head_step_vs_oracle, test_bf16_operand_mode in "bfloat16".  -> what they flag."""
    if mode == BF:
        return bf16_notices(c, st, inp, T, loss)
    o32 = oracle(c, st, inp)
    got = dict(T["grad"], input=T["dx"])
    want32 = dict(o32["grad"], input=o32["dx"])
    out = []
    lg, wl = np.asarray(T["logits"]).ravel(), o32["logits"].ravel()
    if c.head == "mask":
        o64 = oracle(c, st, inp, torch.float64)
        out += ["loss"] if loss and abs(loss[0] - o32["loss"][0]) > 5e-6 else []
        out += ["logits"] if np.abs(lg - wl).max() > 1e-5 * max(1.0, float(np.abs(wl).max())) else []
        for k, w64 in dict(o64["grad"], input=o64["dx"]).items():
            if not _rel(got[k], w64) <= max(4 * _rel(want32[k], w64), 1e-3):
                out.append("grad " + k)
        return out
    atol, rtol = (3e-5 * float(np.abs(wl).max()), 1e-4) if c.head == "rpn" else (5e-5 * max(1.0, float(np.abs(wl).max())), 2e-4)
    out += ["logits"] if np.abs(lg - wl).max() > atol else []
    out += ["loss.%d" % i for i, (g, w) in enumerate(zip(loss, o32["loss"])) if abs(g - w) > 1e-5 * abs(w) + 1e-7]
    for k, w in want32.items():
        if np.linalg.norm(np.asarray(got[k]).ravel() - w.ravel()) > rtol * np.linalg.norm(w.ravel()) + 1e-9:
            out.append("grad " + k)
    return out


# ------------------------------------------------------------------------------------------------------------ the device side
def read_device(m, c, inp, shape=None):
    """Every stored tensor of the last pass of model `m` and its gradients (library layout) as the checker's dictionary."""
    from rfi_toolbox_amd.models.unet import HipSegmenter
    T = {"x": flat_x(c, inp["x"]), "grad": OrderedDict()}
    for name in tensor_names(c):
        T[name] = m.debug_tensor(name).reshape(shape_of(c, name, shape))
    for k, nm in keys(c).items():
        T["grad"][k] = HipSegmenter.grad(m, nm)
    if "y" in inp:
        T["y"] = inp["y"]
    return T


def kernel_expectations(c, mode):
    """What the context profile's contraction labels must show for this run: (what, regular expression, must it match a label)."""
    cin, hid = widths(c)
    o = out_channels(c)
    out = []
    if c.head == "box":
        ws = mode == F32 and hid % 16 == 0
        out.append(("fc7 on gemm_ws", r"^gemm_ws 1x1 .* %d->%d " % (hid, hid), ws))
        return out
    n, h, w = c.shape
    ws = mode != MF and h >= 8 and w >= 8 and cin % 16 == 0
    out.append(("3x3 layers on conv_ws", r"^conv_ws N%d %dx%d %d->%d " % (n, h, w, cin, cin), ws))
    mfma = cin % 16 == 0          # (narrower layers may fall to the direct kernel, whose profile rows carry no label)
    if mfma:
        out.append(("3x3 layers on the MFMA kernel", r"^conv R3S1 N%d %dx%d %d->%d\b" % (n, h, w, cin, cin), not ws))
    if c.head == "mask":
        gw = mode == F32 and cin % 32 == 0
        out.append(("transposed conv on gemm_ws", r"^gemm_ws convT ", gw))
        if mfma:
            out.append(("transposed conv on the MFMA kernel", r"^conv R1S1 .* z4\b", not gw))
    s = 2 if c.head == "mask" else 1
    if mfma or not head_on_mfma(c, mode):
        out.append(("head on the conv kernels", r"^(conv R1S1|gemm_ws 1x1) N%d %dx%d %d->%d\b" % (n, s * h, s * w, cin, o), head_on_mfma(c, mode)))
    return out


def kernel_mismatches(c, mode, labels):
    return [what for what, rx, want in kernel_expectations(c, mode) if any(re.search(rx, l) for l in labels) != want]
