"""The plain U-Net's bfloat16 data flow, stage by stage (model_planes.cpp: forward_planes / backward_planes).  Importable
without a GPU: test_unet_bf16_stages_host.py runs the checker on a CPU stand-in and on mutations of it,
test_gpu_unet_bf16_stages.py runs it on the tensors the device leaves behind (``UNet.debug_tensor``).

METHOD: teacher forcing.  Every launch of the flow reads its inputs from HBM and all of them are stored, so a float64 oracle
of ONE launch, fed the device's own stored inputs, differs from the device's stored output by that launch's own rounding only:
no rounding flip propagates, and each stage is held to rounding level instead of the whole-model bounds of test_gpu_bf16.py.

THE STAGE TABLE is ``stage_table(case)``: one row per launch, in launch order, from ``act_split`` of the input to the last
encoder weight gradient, with the stored inputs, the stored outputs and the gate that selects the form:

  feat % 4   y16_flow      raw conv outputs are bfloat16 tensors, BatchNorm statistics out of the conv epilogue
  feat % 16  g16_flow      the gradient tensors the input-gradient convs / the head / the max-pool backward write are bfloat16,
                           BatchNorm-backward sums out of their epilogues; the round-1 transposed conv writes bf16 directly
  feat % 32  convt_planes  the transposed convs on the plane kernels (upin, zblocks), bfloat16 dconcat / gBottA

The loss turn-around (logits -> dlogits) is not in the table: test_gpu_loss_step.py holds it to float64 closed forms on the
device's own logits; here ``dlogits`` is a stored input.

WHAT CANNOT BE READ.  The decoder phase and the encoder phase of the backward pass share gA.<l> / gB.<l>: after the pass they
hold the encoder's gradients.  The decoder's gB.<l> (input gradient of its second conv) and gA.<l>, l > 1 (input gradient of the
transposed conv above) are therefore checked THROUGH the BatchNorm backward that consumes them: the float64 oracle of the
contraction gives e and the bound b of the contraction criterion, and since dY is linear in dA with the factor gamma * invstd *
act'(z), the stored dY must lie within |gamma invstd act'| b + its own rounding of the oracle's dY ("composite" rows).  The
head's gA.1 needs no such detour: it is dlogits * w, one float32 product (rounded to bf16 with g16_flow), reproduced bit for bit.

CRITERIA (eps = 2^-24; e the float64 value, S the sum of the absolute values of its terms, g the device's value)
  elem    act_split, bn_relu_pool_planes, the BatchNorm-backward apply, pool_bwd_merge, BatchNorm scale / shift: the kernels form
          y * scale + shift with product and sum rounded separately (-ffp-contract=off) and round to bf16 once, so g must equal
          the same float32 expression in NumPy BIT FOR BIT (values; -0 == 0).  pooled == the 2x2 max of the device's own skip,
          xin == round-to-nearest-even of the input.
  conv16  contractions with a bf16 result (conv, input gradient, the three transposed-conv forms): finite, representable, and
          |g - e| <= 1/2 ulp_bf16(max(|g|, |e|)) + k eps S.  The half ulp is what makes truncation fail.
  f32     float32 results (logits, weight gradients, gradients / conv outputs at widths that keep them float32):
          |g - e| <= k eps S.
  sums    per-channel sums over the pixels (c1, c2, dgamma, dbeta, bias gradients): |g - e| <= k eps S.
  stats   BatchNorm mean within k eps mean|y|, invstd to rtol 2e-5 (test_bn_statistics' tolerance for the variance).
  pad     every padding lane of every plane / bfloat16 tensor is zero, after the forward and after the backward pass.
  k = 16 for conv16 / f32 / sums / stats (the bound test_gpu_ops.py holds the plane kernels to at K = 288; the cases reach
  K = 1152), k = 4 for the composite rows' own float32 rounding.  A ratio above 64 would be a finding, not a bound to raise.

WHICH VALUES THE SUMS ARE OF (read in the code, and tested exactly so; the oracle has both):
  * conv epilogue (conv_planes.hip, finish_quarter): with a bf16 output (y16 / round_y) the value is rounded FIRST and p1 += v,
    p2 += v * v run on the ROUNDED values -- the statistics are those of the stored tensor, not of the accumulators.
  * BatchNorm-backward sums in an input-gradient conv's epilogue (PConvArgs::bwd_*), in head_bwd_vec and pool_bwd_merge_vec
    (da16): of the values AS STORED (bf16-rounded dA).  bn_bwd_reduce reads the stored tensors anyway.
  * the conv-bias gradient out of bn_bwd_apply: the sum of the float32 dY BEFORE its rounding to bf16 (accumulator).
  * the transposed conv's bias gradient (channel_sum): of the stored dconcat.

OPERANDS ROUNDED IN REGISTERS (the round-1 transposed conv at widths without upin): an element of act(y * scale + shift)
is undecided if its float64 value lies within 4 eps (|y scale| + |shift|) of a bf16 rounding boundary; each undecided element
widens the bound of the outputs it feeds by |w| times its bf16 gap, decided elements add nothing.

MASKS AND ROUTES are decided in float64 from the device's Y, scale, shift.  A pre-activation within 4 eps (|y scale| + |shift|)
of 0, or a pooling window whose top two candidates are that close without being equal, is UNDECIDED; the GPU test asserts zero
undecided per case (pick another seed).  Exact ties (bf16 values, ReLU zeros) are decided: the gradient goes to the first
maximum in row-major window order (torch's convention, pool_bwd_merge's strict `>`).

MEASURED on an MI355X (the UNETBF16 lines of test_gpu_unet_bf16_stages.py): the worst ratio of each class against its k, and
the tensor it belongs to.  conv16 counts what is left of |g - e| after the half ulp, in units of eps S (0: every element within
half an ulp of the float64 value).  elem: 0 differing elements and pad: 0 non-zero lanes in every row; undecided masks / routes:
0 in every row; undecided operand elements (they only widen a bound): 9, 2, 6, 3 in rows 2-5.  No class needs more than k = 16
at K = 1152 (the longest contraction, bott.conv2 of f32_d2: 9 x 128); the CPU stand-in, another summation order, shows
conv16 0.48, f32 5.1, sums 0.89, stats 0.90 over the same cases.

  case                              conv16 (k 16)       f32 (k 16)                          sums (k 16)                      stats (k 16)
  f32_d2_1x24x40                    0.31  dconcat.2     2.36 bottleneck.conv.3.weight       1.30 bottleneck.conv.4.weight    0.87 chan.4.mean
  f16_d2_2x24x40                    0.40  gB.2          2.03 dconcat.1                      0.75 bottleneck.conv.1.weight    0.89 chan.4.mean
  f20_d1_1x16x24                    0.02  encY2.1       2.24 dconcat.1                      0.73 bottleneck.conv.4.weight    0.65 chan.2.mean
  in5_f12_d2_3x16x16                0.05  decY1.1       2.06 gB.1                           1.02 bottleneck.conv.1.weight    0.76 chan.9.mean
  in1_f8_d3_1x32x32                 0     -             2.38 bottleneck.conv.0.weight       1.39 chan.6.c2                   0.76 chan.12.mean
  f6_d1_1x16x24                     0     -             1.82 dconcat.1                      0.41 bottleneck.conv.4.weight    1.17 chan.2.mean
  f32_d1_leaky                      0.44  up.1          2.10 bottleneck.conv.3.weight       0.69 chan.3.c2                   0.77 chan.2.mean
  in4_f32_d1_1x16x16                0.14  gB.1          2.62 bottleneck.conv.3.weight       1.08 chan.3.c2                   1.16 chan.5.mean
  f32_d2 at 1x24x40 after 1x48x80   0.43  encY2.2       2.20 bottleneck.conv.3.weight       1.31 bottleneck.conv.1.weight    0.91 chan.2.mean
  f32_d2 at 1x48x80 after 1x24x40   0.67  gB.1          2.31 bottleneck.conv.3.weight       0.67 chan.4.c2                   0.82 chan.3.mean

FOUND: nothing.  Every stage of every case holds its contract as read from the code; no kernel was changed.

MUTATIONS (deliberately wrong builds, value-only, never committed; the whole of test_gpu_unet_bf16_stages.py and
test_gpu_bf16.py::test_bf16_data_flow_other_shapes on an MI355X):
  * act_split truncating to bf16 instead of rounding to nearest: every act_split line of every case turns red and nothing else
    (xin, a1e.<l>, a1b, a1d.<l>, upin.<l> at feat 32, up.<l> where it converts the float32 up-conv output); all eight cases and
    the reshape run fail.  test_bf16_data_flow_other_shapes notices this one too (5 of 5 red): truncating EVERY activation is a
    bias of a quarter ulp on all operands, large enough for the whole-model bounds.
  * the plane conv's epilogue leaving the channels of the last partial 16-channel chunk out of the BatchNorm statistics: the
    `<block>.conv<i>:stats` lines (chan.<i>.mean / invstd) of every layer with a partial chunk turn red in f20_d1, in5_f12_d2,
    in1_f8_d3 and f6_d1 (mean 0, invstd 316: the activations then grow layer by layer and the backward pass reaches NaN, so
    the later lines of those cases are red as well -- a non-finite value never passes); the four cases whose widths are whole
    chunks rightly stay green.  test_bf16_data_flow_other_shapes: red at widths 8, 12 and 6, green at 16 (2 of 5).
  * pool_bwd_merge routing a tied window to its LAST maximum: `enc<l>.pool_bwd_merge` (gA.<l>) turns red at every level of
    every case and in both reshape runs, and no other line does.  test_bf16_data_flow_other_shapes stays GREEN on all five
    shapes: the gap this module closes.
"""
from collections import OrderedDict, namedtuple

import numpy as np
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
K_CONTRACTION = 16.0          # conv16 / f32 / sums / stats
K_ELEM = 4.0                  # the float32 rounding of an element-wise expression that cannot be reproduced bit for bit
BN_EPS = 1e-5
INVSTD_RTOL = 2e-5

Case = namedtuple("Case", "id in_ch feat depth n h w slope seed covers")

CASES = [
    Case("f32_d2_1x24x40", 3, 32, 2, 1, 24, 40, 0.0, 0, ("y16:yes", "g16:yes", "convt:planes", "ragged:yes", "depth:2")),
    Case("f16_d2_2x24x40", 3, 16, 2, 2, 24, 40, 0.0, 0, ("y16:yes", "g16:yes", "convt:direct16", "ragged:yes", "batch:2")),
    Case("f20_d1_1x16x24", 3, 20, 1, 1, 16, 24, 0.0, 0, ("y16:yes", "g16:no", "convt:f32_split", "chunk:partial", "depth:1")),
    Case("in5_f12_d2_3x16x16", 5, 12, 2, 3, 16, 16, 0.0, 0, ("y16:yes", "g16:no", "chunk:narrow", "in:padded", "batch:3")),
    Case("in1_f8_d3_1x32x32", 1, 8, 3, 1, 32, 32, 0.0, 0, ("y16:yes", "g16:no", "depth:3", "map:4x4", "convt:direct16")),
    Case("f6_d1_1x16x24", 3, 6, 1, 1, 16, 24, 0.0, 0, ("y16:no", "g16:no", "convt:f32_split", "chunk:narrow")),
    Case("f32_d1_leaky", 3, 32, 1, 1, 16, 24, 0.1, 0, ("slope:leaky", "convt:planes", "depth:1")),
    Case("in4_f32_d1_1x16x16", 4, 32, 1, 1, 16, 16, 0.0, 0, ("in:true4", "convt:planes", "depth:1")),
]
BY_ID = OrderedDict((c.id, c) for c in CASES)
# the one-model-several-shapes run (PlaneBuf::ensure's zero area and the padding after a shape change)
RESHAPE_BASE = "f32_d2_1x24x40"
RESHAPE_SEQUENCE = [(1, 48, 80), (1, 24, 40), (1, 48, 80)]

ALL_GATE_VALUES = ["y16:yes", "y16:no", "g16:yes", "g16:no", "convt:planes", "convt:direct16", "convt:f32_split", "chunk:partial",
                   "chunk:narrow", "in:padded", "in:true4", "slope:leaky", "slope:relu", "ragged:yes", "depth:1", "depth:2",
                   "depth:3", "map:4x4", "batch:2", "batch:3", "tiles:multi"]


def gates(c):
    """The three gates of prepare_planes as predicates of the width."""
    return {"y16": c.feat % 4 == 0, "g16": c.feat % 16 == 0, "ctp": c.feat % 32 == 0}


def gate_values(c):
    g = gates(c)
    v = {"y16:yes" if g["y16"] else "y16:no", "g16:yes" if g["g16"] else "g16:no", "depth:%d" % c.depth,
         "slope:leaky" if c.slope else "slope:relu"}
    for l in range(1, c.depth + 1):
        C = c.feat << (l - 1)
        v.add("convt:planes" if g["ctp"] else "convt:direct16" if C % 16 == 0 else "convt:f32_split")
        if C % 16:
            v.add("chunk:partial" if C > 16 else "chunk:narrow")
        hh, ww = c.h >> (l - 1), c.w >> (l - 1)
        # ragged against the 8 x 32, 16 x 16 and 8 x 8 output tiles of the plane conv kernel
        if any(hh % th or ww % tw for th, tw in ((8, 32), (16, 16), (8, 8))):
            v.add("ragged:yes")
        if hh * ww > 16 * 16:
            v.add("tiles:multi")
    if c.in_ch % 16:
        v.add("in:true4" if c.in_ch == 4 else "in:padded")
    if (c.h >> c.depth) <= 4 and (c.w >> c.depth) <= 4:
        v.add("map:4x4")
    if c.n > 1:
        v.add("batch:%d" % c.n)
    return v


# ------------------------------------------------------------------------------------------------------------ bf16 helpers
def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def rne(a):
    """float32 -> the nearest bf16 value (ties to even), as float32."""
    b = f32(a).view(np.uint32)
    r = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def trunc_bf16(a):
    return (f32(a).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def is_bf16(a):
    return (f32(a).view(np.uint32) & np.uint32(0xFFFF)) == 0


def ulp_bf16(v):
    """Spacing of the bf16 values at magnitude |v| (0 at 0)."""
    v = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(v)
    return np.where(v > 0, np.ldexp(1.0, e - 8), 0.0)


def other_neighbour(g, e):
    """The bf16 neighbour of g on the other side of e (what a wrong rounding direction would store)."""
    g = np.asarray(g, np.float64)
    return np.where(e >= g, g + ulp_bf16(np.maximum(np.abs(g), np.abs(e))), g - ulp_bf16(np.maximum(np.abs(g), np.abs(e))))


# ------------------------------------------------------------------------------------------------------------ names
def conv_prefix(c, i):
    """state_dict prefix and conv / bn sub-index of convs[i] (enc1.c1, enc1.c2, ..., bott.c1, bott.c2, decD.c1, ..., dec1.c2)."""
    D = c.depth
    which = i & 1
    if i < 2 * D:
        p = "encoder%d.conv.conv" % (i // 2 + 1)
    elif i < 2 * D + 2:
        p = "bottleneck.conv"
    else:
        p = "decoder%d.conv.conv" % (D - (i - 2 * D - 2) // 2)
    return p, (3 if which else 0), (4 if which else 1)


def conv_index(c, block, which):
    """block: ("enc", l) | ("bott",) | ("dec", l); which: 0 / 1."""
    D = c.depth
    if block[0] == "enc":
        return 2 * (block[1] - 1) + which
    if block[0] == "bott":
        return 2 * D + which
    return 2 * D + 2 + 2 * (D - block[1]) + which


def block_names(block):
    """(Y1, A1, Y2, dYa, dYb) tensor names of a DoubleConv."""
    if block[0] == "enc":
        l = block[1]
        return "encY1.%d" % l, "a1e.%d" % l, "encY2.%d" % l, "dYaE.%d" % l, "dYbE.%d" % l
    if block[0] == "bott":
        return "bottY1", "a1b", "bottY2", "dYbottA", "dYbottB"
    l = block[1]
    return "decY1.%d" % l, "a1d.%d" % l, "decY2.%d" % l, "dYa.%d" % l, "dYb.%d" % l


def plane_names(c):
    """Every tensor with padding lanes a case can have: name -> channels."""
    g, D = gates(c), c.depth
    out = OrderedDict()
    out["xin"] = c.in_ch
    for l in range(1, D + 1):
        C = c.feat << (l - 1)
        for b in ("a1e", "skip", "pooled", "up", "a1d", "dYa", "dYb", "dYaE", "dYbE"):
            out["%s.%d" % (b, l)] = C
        if g["ctp"]:
            out["upin.%d" % l] = 2 * C
        if g["y16"]:
            for b in ("encY1", "encY2", "decY1"):
                out["%s.%d" % (b, l)] = C
        if g["y16"] and l == 1:
            out["decY2.1"] = C
    Cb = c.feat << D
    for b in ("a1b", "dYbottA", "dYbottB"):
        out[b] = Cb
    if g["y16"]:
        out["bottY1"] = Cb
    return out


def tensor_names(c):
    """Every tensor the checker reads besides logits / dlogits / chan.<i> / the gradients."""
    g, D = gates(c), c.depth
    names = ["xin"]
    for l in range(1, D + 1):
        names += ["%s.%d" % (b, l) for b in ("encY1", "a1e", "encY2", "skip", "pooled", "up", "decY1", "a1d", "decY2", "dYa", "dYb",
                                             "dconcat", "gA", "dYaE", "gB", "dYbE", "dpool")]
        if g["ctp"]:
            names.append("upin.%d" % l)
        elif (c.feat << (l - 1)) % 16:
            names.append("upf.%d" % l)
    names += ["bottY1", "a1b", "bottY2", "gBottA", "dYbottA", "gBottB", "dYbottB"]
    return names


def shape_of(c, name, n=None, h=None, w=None):
    n, h, w = n or c.n, h or c.h, w or c.w
    base, _, idx = name.partition(".")
    D = c.depth
    if base in ("xin",):
        return (n, h, w, c.in_ch)
    if base in ("logits", "dlogits"):
        return (n, h, w, 1)
    if idx:
        l = int(idx)
        C = c.feat << (l - 1)
        hh, ww = h >> (l - 1), w >> (l - 1)
        if base in ("pooled", "dpool"):
            return (n, hh // 2, ww // 2, C)
        if base == "upin":
            return (n, hh // 2, ww // 2, 2 * C)
        if base == "dconcat":
            return (n, hh, ww, 2 * C)
        return (n, hh, ww, C)
    return (n, h >> D, w >> D, c.feat << D)


# ------------------------------------------------------------------------------------------------------------ inputs
def init_state(c):
    from oracle import unet_ref
    st = unet_ref.init_state(c.in_ch, 1, c.feat, depth=c.depth, seed=c.seed)
    # BatchNorm weights and biases away from (1, 0), so that gamma, beta and a wrong sign of either show
    g = torch.Generator().manual_seed(c.seed + 500)
    for k in st:
        if k.endswith((".1.weight", ".4.weight")):
            st[k] = 0.5 + torch.rand(st[k].shape, generator=g)
        elif k.endswith((".1.bias", ".4.bias")):
            st[k] = 0.4 * torch.rand(st[k].shape, generator=g) - 0.2
    return st


def inputs(c, n=None, h=None, w=None, seed_offset=0):
    n, h, w = n or c.n, h or c.h, w or c.w
    g = torch.Generator().manual_seed(c.seed + 1000 + seed_offset)
    x = torch.randn(n, h, w, c.in_ch, generator=g)
    y = (torch.rand(n, h, w, generator=g) > 0.8).to(torch.uint8)
    return x, y


# ------------------------------------------------------------------------------------------------------------ float64 stage functions
# Written from the definition of the operation (torch CPU float64), not from the kernel.  Each returns (e, S) as NHWC
# (activations) or reference-layout (parameters) float64 arrays.
def _t(a):                      # NHWC numpy -> NCHW float64 torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).permute(0, 3, 1, 2).contiguous()


def _n(t):                      # NCHW torch -> NHWC numpy
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _w(w):                      # a float32 parameter as the bf16 operand the contraction reads
    return torch.from_numpy(rne(np.asarray(w, np.float32)).astype(np.float64))


def conv3x3_stage(x, w, b):
    """y = conv3x3(x, bf16(w), pad 1) + b."""
    xt, wt, bt = _t(x), _w(w), torch.from_numpy(np.asarray(b, np.float64))
    return _n(F.conv2d(xt, wt, bt, padding=1)), _n(F.conv2d(xt.abs(), wt.abs(), bt.abs(), padding=1))


def dgrad3x3_stage(dy, w):
    """dx = the adjoint of conv3x3 applied to dy."""
    dt, wt = _t(dy), _w(w)
    return _n(F.conv_transpose2d(dt, wt, padding=1)), _n(F.conv_transpose2d(dt.abs(), wt.abs(), padding=1))


def wgrad_stage(x, dy, wshape, stride=1, padding=1):
    xt, dt = _t(x), _t(dy)
    return (torch.nn.grad.conv2d_weight(xt, wshape, dt, stride=stride, padding=padding).numpy(),
            torch.nn.grad.conv2d_weight(xt.abs(), wshape, dt.abs(), stride=stride, padding=padding).numpy())


def convt_stage(a, w, b, gap=None):
    """ConvTranspose2d(k2, s2): up = scatter(a, bf16(w)) + b; `gap`: the bf16 gap of the undecided elements of a (else 0) ->
    also the widening |w| * gap of every output."""
    at, wt, bt = _t(a), _w(w), torch.from_numpy(np.asarray(b, np.float64))
    e = _n(F.conv_transpose2d(at, wt, bt, stride=2))
    S = _n(F.conv_transpose2d(at.abs(), wt.abs(), bt.abs(), stride=2))
    wide = _n(F.conv_transpose2d(_t(gap), wt.abs(), stride=2)) if gap is not None else 0.0
    return e, S, wide


def convt_dgrad_stage(dup, w):
    dt, wt = _t(dup), _w(w)
    return _n(F.conv2d(dt, wt, stride=2)), _n(F.conv2d(dt.abs(), wt.abs(), stride=2))


def convt_wgrad_stage(dup, a, wshape, gap=None):
    dt, at = _t(dup), _t(a)
    e = torch.nn.grad.conv2d_weight(dt, wshape, at, stride=2).numpy()
    S = torch.nn.grad.conv2d_weight(dt.abs(), wshape, at.abs(), stride=2).numpy()
    wide = torch.nn.grad.conv2d_weight(dt.abs(), wshape, _t(gap), stride=2).numpy() if gap is not None else 0.0
    return e, S, wide


def head_stage(Y, scale, shift, slope, w, b):
    """logits = b + sum_c act(Y scale + shift) w (the head reads the float32 activation: no bf16 rounding of it)."""
    Y = np.asarray(Y, np.float64)
    z = Y * scale + shift
    a = np.where(z > 0, z, z * slope)
    w = np.asarray(w, np.float64).reshape(-1)
    e = (a * w).sum(-1, keepdims=True) + float(b)
    S = ((np.abs(Y * scale) + np.abs(shift)) * np.abs(w)).sum(-1, keepdims=True) + abs(float(b))
    return e, S


def stats_stage(Y):
    """Batch mean and 1 / sqrt(biased variance + eps) per channel, and mean |y|."""
    Y = np.asarray(Y, np.float64).reshape(-1, Y.shape[-1])
    mean = Y.mean(0)
    var = ((Y - mean) ** 2).mean(0)
    return mean, 1.0 / np.sqrt(var + BN_EPS), np.abs(Y).mean(0)


def preact(Y, scale, shift):
    """z = Y scale + shift in float64 and the band 4 eps (|y scale| + |shift|) inside which float32 cannot be trusted."""
    Y = np.asarray(Y, np.float64)
    return Y * scale + shift, 4 * EPS * (np.abs(Y * scale) + np.abs(shift))


def relu_mask(Y, scale, shift):
    """(z > 0, number of undecided elements)."""
    z, tol = preact(Y, scale, shift)
    return z > 0, int(((np.abs(z) <= tol) & (tol > 0) & (z != 0)).sum())


def pool_routes(Y, scale, shift, slope):
    """The window position (0..3, row-major) each pooled pixel's gradient goes to: the FIRST maximum of the activation.
    -> (arg [N, H/2, W/2, C], undecided windows, windows with an exact tie at the maximum)."""
    z, tol = preact(Y, scale, shift)
    a = np.where(z > 0, z, z * slope)
    N, H, W, C = a.shape
    win = lambda t: t.reshape(N, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, C, 4)  # noqa: E731
    aw, tw = win(a), win(tol)
    arg = aw.argmax(-1)                                          # numpy: the first maximum
    top = np.take_along_axis(aw, arg[..., None], -1)
    order = np.sort(aw, -1)
    second = order[..., 2:3]
    ties = int((second == top).sum())
    close = (np.abs(top - second) <= 2 * tw.max(-1, keepdims=True)) & (second != top)
    return arg, int(close.sum()), ties


def route(dpool, arg):
    """Scatter dpool [N, H/2, W/2, C] to the window position arg -> [N, H, W, C] (zeros elsewhere)."""
    N, Hp, Wp, C = dpool.shape
    out = np.zeros((N, Hp, Wp, C, 4), dpool.dtype)
    np.put_along_axis(out, arg[..., None], dpool[..., None], -1)
    return out.reshape(N, Hp, Wp, C, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(N, 2 * Hp, 2 * Wp, C)


def operand_in_registers(Y, scale, shift, slope):
    """act(Y scale + shift) rounded to bf16 in registers: (decided values, bf16 gap of the undecided elements, their count)."""
    z, tol = preact(Y, scale, shift)
    act = lambda t: np.where(t > 0, t, t * slope)  # noqa: E731
    lo, hi = rne(act(z - tol).astype(np.float32)), rne(act(z + tol).astype(np.float32))
    gap = (hi.astype(np.float64) - lo.astype(np.float64))
    return lo.astype(np.float64), gap, int((gap != 0).sum())


# float32 expressions of the element-wise kernels, operation by operation (NumPy rounds each product and sum separately)
def act32(Y, scale, shift, slope):
    z = f32(Y) * f32(scale) + f32(shift)
    return np.where(z > 0, z, z * np.float32(slope) if slope else np.float32(0) * z).astype(np.float32), z


def bn_coeffs32(gamma, beta, mean, invstd):
    sc = f32(gamma) * f32(invstd)
    return sc, f32(beta) - f32(mean) * sc


def bn_apply32(dA, Y, chan, gamma, slope):
    """dY = (gamma invstd) (dz - c1 - xhat c2) in float32, before its rounding to bf16."""
    z = f32(Y) * chan["scale"] + chan["shift"]
    dA = f32(dA)
    dz = np.where(z > 0, dA, dA * np.float32(slope)).astype(np.float32)
    xh = (f32(Y) - chan["mean"]) * chan["invstd"]
    g = f32(gamma) * chan["invstd"]
    return g * ((dz - chan["c1"]) - xh * chan["c2"])


def split_chan(v, C):
    v = np.asarray(v, np.float32).reshape(8, C)
    return dict(zip(("running_mean", "running_var", "mean", "invstd", "scale", "shift", "c1", "c2"), v))


# ------------------------------------------------------------------------------------------------------------ the checker
class Finding(namedtuple("Finding", "stage klass tensor ratio limit ok detail")):
    def line(self, case_id, tag="UNETBF16"):
        return "%s %s %s %.3g %s" % (tag, case_id, self.klass, self.ratio, self.tensor)


# a conv + BatchNorm layer as bn_backward_layer needs it: its place in `convs`, the names of its parameters (b: None without a
# conv bias), stride and padding of the conv
Layer = namedtuple("Layer", "i w b gamma beta stride pad")


class Criteria:
    """The criteria of the module docstring and the report / failure machinery, shared by the stage checkers of both encoders
    (tests/resnet_bf16_stages.py has the other): one Finding per (stage, output)."""
    TAG = "UNETBF16"

    def __init__(self):
        self.findings = []
        self.undecided = 0                # ReLU masks and pooling routes float32 cannot be trusted to decide
        self.tie_windows = 0

    def _add(self, stage, klass, tensor, ratio, limit, detail=""):
        ok = bool(np.isfinite(ratio)) and ratio <= limit
        self.findings.append(Finding(stage, klass, tensor, float(ratio), float(limit), ok, detail))

    def exact(self, stage, tensor, got, want):
        got, want = np.asarray(got), np.asarray(want)
        if got.shape != want.shape:
            got = got.reshape(want.shape)
        bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
        detail = ""
        if bad.any():
            i = np.argwhere(bad)[0]
            detail = "%d of %d differ, first at %s: %r != %r" % (bad.sum(), bad.size, tuple(i), got[tuple(i)], want[tuple(i)])
        self._add(stage, "elem", tensor, float(bad.sum()), 0.0, detail)

    def close(self, stage, klass, tensor, got, e, S, half_ulp=False, extra=0.0, k=K_CONTRACTION):
        got = np.asarray(got, np.float64).reshape(np.shape(e))
        e, S = np.asarray(e, np.float64), np.asarray(S, np.float64)
        err = np.abs(got - e) - extra
        if half_ulp:
            err = err - 0.5 * ulp_bf16(np.maximum(np.abs(got), np.abs(e)))
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err <= 0, 0.0, err / (EPS * S))
        r = np.where(np.isfinite(got), r, np.inf)
        if half_ulp:
            r = np.where(is_bf16(got.astype(np.float32)), r, np.inf)      # (not representable: not a bf16 result at all)
        r = np.nan_to_num(r, nan=np.inf)
        worst = float(r.max()) if r.size else 0.0
        detail = ""
        if worst > k:
            i = np.unravel_index(int(r.argmax()), r.shape)
            detail = "worst at %s: got %r, want %r, S %r (%d elements over)" % (i, got[i], e[i], S[i], int((r > k).sum()))
        self._add(stage, klass, tensor, worst, k, detail)

    def stats(self, stage, i, ch, Y):
        """chan.<i>'s mean / invstd against those of the STORED values Y (conv_planes.hip: rounded first, then summed)."""
        mean, invstd, mabs = stats_stage(Y)
        self.close(stage + ":stats", "stats", "chan.%d.mean" % i, ch["mean"], mean, mabs)
        self._add(stage + ":stats", "stats", "chan.%d.invstd" % i, float(np.abs(ch["invstd"] / invstd - 1).max()) / INVSTD_RTOL * K_CONTRACTION,
                  K_CONTRACTION)

    # -- access
    def chan(self, i):
        return self.T["chan"][i]

    def param(self, name):
        return self.st[name]

    def grad(self, name):
        return self.T["grad"][name]

    def _mask(self, Y, ch):
        m, und = relu_mask(Y, ch["scale"].astype(np.float64), ch["shift"].astype(np.float64))
        self.undecided += und
        return m

    def bn_backward_layer(self, stage, L, dA, Y_name, x, dY_name, dA_bound=None, slope=None):
        """BatchNorm backward of layer L (a Layer record) + its conv's weight and bias gradients.  dA: the stored gradient w.r.t.
        the activated output (exact), or with dA_bound the float64 oracle of a gradient that cannot be read (composite row).
        slope: the activation slope of the layer's output (default: the model's; 1: no activation of its own -- no mask to decide)."""
        c, T = self.c, self.T
        slope = c.slope if slope is None else slope
        ch, Y = self.chan(L.i), np.asarray(T[Y_name], np.float64)
        gamma = self.param(L.gamma)
        mask = self._mask(T[Y_name], ch) if slope != 1 else np.ones(Y.shape, bool)
        f = np.where(mask, 1.0, slope)
        dz = np.asarray(dA, np.float64) * f
        xh = (Y - ch["mean"].astype(np.float64)) * ch["invstd"].astype(np.float64)
        M = Y.size // Y.shape[-1]
        ax = (0, 1, 2)
        b = np.zeros_like(dz) if dA_bound is None else np.asarray(dA_bound, np.float64) * f
        s1, s2, S1, S2 = dz.sum(ax), (dz * xh).sum(ax), np.abs(dz).sum(ax), np.abs(dz * xh).sum(ax)
        w1, w2 = b.sum(ax), (b * np.abs(xh)).sum(ax)
        st = stage + ":sums"
        self.close(st, "sums", "chan.%d.c1" % L.i, ch["c1"], s1 / M, S1 / M, extra=w1 / M)
        self.close(st, "sums", "chan.%d.c2" % L.i, ch["c2"], s2 / M, S2 / M, extra=w2 / M)
        self.close(st, "sums", L.beta, self.grad(L.beta), s1, S1, extra=w1)
        self.close(st, "sums", L.gamma, self.grad(L.gamma), s2, S2, extra=w2)
        dY = T[dY_name]
        if dA_bound is None:
            o = bn_apply32(dA, T[Y_name], ch, gamma, slope)
            self.exact(stage + ":apply", dY_name, dY, rne(o))
            o64 = o.astype(np.float64)
            if L.b:
                self.close(stage + ":apply", "sums", L.b, self.grad(L.b), o64.sum(ax), np.abs(o64).sum(ax))
        else:
            gi = gamma.astype(np.float64) * ch["invstd"].astype(np.float64)
            c1, c2 = ch["c1"].astype(np.float64), ch["c2"].astype(np.float64)
            o = gi * (dz - c1 - xh * c2)
            So = np.abs(gi) * (np.abs(dz) + np.abs(c1) + np.abs(xh * c2))
            wide = np.abs(gi) * b
            # (its own rounding: a handful of float32 operations, k = 4 of S, then one rounding to bf16)
            self.close(stage + ":apply(composite)", "conv16", dY_name, dY, o, So, half_ulp=True, extra=wide, k=K_ELEM)
            if L.b:
                self.close(stage + ":apply(composite)", "sums", L.b, self.grad(L.b), o.sum(ax),
                           np.abs(o).sum(ax) + So.sum(ax) * K_ELEM / K_CONTRACTION,
                           extra=wide.sum(ax))
        e, S = wgrad_stage(x, dY, self.param(L.w).shape, L.stride, L.pad)
        self.close(stage + ":wgrad", "f32", L.w, self.grad(L.w), e, S)

    def padding(self):
        for when in ("pad_fwd", "pad_bwd"):
            for name, v in self.T.get(when, {}).items():
                nz = int(np.count_nonzero(np.nan_to_num(np.asarray(v), nan=1.0)))
                self._add("%s" % when, "pad", name + ":pad", float(nz), 0.0, "%d non-zero padding lanes" % nz if nz else "")

    # -- reporting
    def failures(self):
        return [f for f in self.findings if not f.ok]

    def failed_stages(self):
        return sorted({f.stage.split(":")[0] for f in self.failures()})

    def worst_per_class(self):
        out = OrderedDict()
        for f in self.findings:
            if f.klass not in out or f.ratio > out[f.klass].ratio:
                out[f.klass] = f
        return out

    def report(self):
        return [f.line(self.c.id, self.TAG) for f in self.worst_per_class().values()]


class Checker(Criteria):
    """Runs the stage table of one case over a tensor dictionary T (device or stand-in):
       T[name]            NHWC float32 arrays under the debug_tensor names, "logits", "dlogits", "x"
       T["chan"][i]       split_chan(chan.<i>)
       T["grad"][name]    the gradients in the reference's layout
       T["pad_fwd"] / T["pad_bwd"][name]   the padding lanes after the forward / the backward pass
    ``state``: the parameters.  findings: one Finding per (stage, output)."""

    def __init__(self, case, state, T):
        self.c, self.T = case._replace(slope=float(np.float32(case.slope))), T      # (the slope as the device's float holds it)
        self.st = {k: v.numpy() if hasattr(v, "numpy") else np.asarray(v) for k, v in state.items()}
        self.g = gates(case)
        super().__init__()
        self.operand_undecided = 0        # elements of an operand rounded in registers next to a bf16 boundary (they widen bounds)
        self.rows = []

    # -- stages
    def conv_bn(self, stage, block, which, segs, out_name):
        """conv3x3 + bias of [segs] -> out_name, its BatchNorm statistics and coefficients."""
        c, T = self.c, self.T
        i = conv_index(c, block, which)
        p, ci, bi = conv_prefix(c, i)
        x = np.concatenate([T[s] for s in segs], -1)
        e, S = conv3x3_stage(x, self.param("%s.%d.weight" % (p, ci)), self.param("%s.%d.bias" % (p, ci)))
        Y = T[out_name]
        if self.g["y16"]:
            self.close(stage, "conv16", out_name, Y, e, S, half_ulp=True)
        else:
            self.close(stage, "f32", out_name, Y, e, S)
        ch = self.chan(i)
        self.stats(stage, i, ch, Y)
        sc, sh = bn_coeffs32(self.param("%s.%d.weight" % (p, bi)), self.param("%s.%d.bias" % (p, bi)), ch["mean"], ch["invstd"])
        self.exact(stage + ":coeffs", "chan.%d.scale" % i, ch["scale"], sc)
        self.exact(stage + ":coeffs", "chan.%d.shift" % i, ch["shift"], sh)

    def act_split(self, stage, src, i, out_name):
        ch = self.chan(i)
        a, _ = act32(self.T[src], ch["scale"], ch["shift"], self.c.slope)
        self.exact(stage, out_name, self.T[out_name], rne(a))

    def forward(self):
        c, T, g, D = self.c, self.T, self.g, self.c.depth
        self.exact("act_split(x)", "xin", T["xin"], rne(T["x"]))
        cur = "xin"
        for l in range(1, D + 1):
            b = ("enc", l)
            Y1, A1, Y2, _, _ = block_names(b)
            self.conv_bn("enc%d.conv1" % l, b, 0, [cur], Y1)
            self.act_split("enc%d.act_split" % l, Y1, conv_index(c, b, 0), A1)
            self.conv_bn("enc%d.conv2" % l, b, 1, [A1], Y2)
            ch = self.chan(conv_index(c, b, 1))
            a, _ = act32(T[Y2], ch["scale"], ch["shift"], c.slope)
            skip = rne(a)
            st = "enc%d.bn_relu_pool_planes" % l
            self.exact(st, "skip.%d" % l, T["skip.%d" % l], skip)
            N, H, W, C = a.shape
            mx = lambda t: t.reshape(N, H // 2, 2, W // 2, 2, C).max((2, 4))  # noqa: E731
            self.exact(st, "pooled.%d" % l, T["pooled.%d" % l], rne(mx(a)))
            self.exact(st + ":max_of_skip", "pooled.%d" % l, T["pooled.%d" % l], mx(f32(T["skip.%d" % l])))
            cur = "pooled.%d" % l
        b = ("bott",)
        Y1, A1, Y2, _, _ = block_names(b)
        self.conv_bn("bott.conv1", b, 0, [cur], Y1)
        self.act_split("bott.act_split", Y1, conv_index(c, b, 0), A1)
        self.conv_bn("bott.conv2", b, 1, [A1], Y2)
        prevY, prevI = Y2, conv_index(c, b, 1)
        for l in range(D, 0, -1):
            up_w, up_b = self.param("decoder%d.up.weight" % l), self.param("decoder%d.up.bias" % l)
            ch = self.chan(prevI)
            st = "dec%d.up" % l
            if g["ctp"]:
                self.act_split("dec%d.act_split(upin)" % l, prevY, prevI, "upin.%d" % l)
                e, S, _ = convt_stage(T["upin.%d" % l], up_w, up_b)
                self.close(st + ":planes", "conv16", "up.%d" % l, T["up.%d" % l], e, S, half_ulp=True)
            else:
                a, gap, und = operand_in_registers(T[prevY], ch["scale"].astype(np.float64), ch["shift"].astype(np.float64), c.slope)
                self.operand_undecided += und
                e, S, wide = convt_stage(a, up_w, up_b, gap)
                if "upf.%d" % l in T:                         # float32 output + one conversion pass
                    self.close(st + ":regs_f32", "f32", "upf.%d" % l, T["upf.%d" % l], e, S, extra=wide)
                    self.exact("dec%d.act_split(upf)" % l, "up.%d" % l, T["up.%d" % l], rne(T["upf.%d" % l]))
                else:                                         # the direct bf16 write
                    self.close(st + ":regs", "conv16", "up.%d" % l, T["up.%d" % l], e, S, half_ulp=True, extra=wide)
            b = ("dec", l)
            Y1, A1, Y2, _, _ = block_names(b)
            self.conv_bn("dec%d.conv1" % l, b, 0, ["up.%d" % l, "skip.%d" % l], Y1)
            self.act_split("dec%d.act_split" % l, Y1, conv_index(c, b, 0), A1)
            self.conv_bn("dec%d.conv2" % l, b, 1, [A1], Y2)
            prevY, prevI = Y2, conv_index(c, b, 1)
        ch = self.chan(prevI)
        e, S = head_stage(T[prevY], ch["scale"].astype(np.float64), ch["shift"].astype(np.float64), c.slope,
                          self.param("final_conv.weight"), self.param("final_conv.bias")[0])
        self.close("head_fwd", "f32", "logits", T["logits"], e, S)

    def bn_backward(self, stage, block, which, dA, Y_name, x_segs, dY_name, dA_bound=None):
        """BatchNorm backward of convs[i] + its conv's weight and bias gradients (Criteria.bn_backward_layer)."""
        i = conv_index(self.c, block, which)
        p, ci, bi = conv_prefix(self.c, i)
        L = Layer(i, "%s.%d.weight" % (p, ci), "%s.%d.bias" % (p, ci), "%s.%d.weight" % (p, bi), "%s.%d.bias" % (p, bi), 1, 1)
        self.bn_backward_layer(stage, L, dA, Y_name, np.concatenate([self.T[s] for s in x_segs], -1), dY_name, dA_bound)

    def dgrad(self, stage, block, which, dY_name, out_name, half):
        """Input gradient of convs[i] from its stored dY: -> (e, bound) and, if out_name is readable, its check."""
        c = self.c
        p, ci, _ = conv_prefix(c, conv_index(c, block, which))
        e, S = dgrad3x3_stage(self.T[dY_name], self.param("%s.%d.weight" % (p, ci)))
        if out_name is not None:
            self.close(stage, "conv16" if half else "f32", out_name, self.T[out_name], e, S, half_ulp=half)
        bound = K_CONTRACTION * EPS * S
        if half:
            bound = bound + 0.5 * ulp_bf16(np.abs(e) + bound)
        return e, bound

    def backward(self):
        c, T, g, D = self.c, self.T, self.g, self.c.depth
        d = np.asarray(T["dlogits"], np.float64)
        last = conv_index(c, ("dec", 1), 1)
        ch = self.chan(last)
        Yl = T["decY2.1"]
        # head_bwd: dw = sum_m d act(z), db = sum_m d; da = d * w (float32 product; bf16 with g16_flow)
        z, _ = preact(Yl, ch["scale"].astype(np.float64), ch["shift"].astype(np.float64))
        a = np.where(z > 0, z, z * c.slope)
        Sa = np.abs(np.asarray(Yl, np.float64) * ch["scale"]) + np.abs(ch["shift"])
        self.close("head_bwd", "sums", "final_conv.weight", self.grad("final_conv.weight").reshape(-1), (d * a).sum((0, 1, 2)),
                   (np.abs(d) * Sa).sum((0, 1, 2)))
        self.close("head_bwd", "sums", "final_conv.bias", self.grad("final_conv.bias"), d.sum().reshape(1), np.abs(d).sum().reshape(1))
        da = f32(T["dlogits"]) * f32(self.param("final_conv.weight").reshape(-1))
        dA, dA_bound = (rne(da) if g["g16"] else da), None
        for l in range(1, D + 1):
            b = ("dec", l)
            Y1, A1, Y2, dYa, dYb = block_names(b)
            C = c.feat << (l - 1)
            self.bn_backward("dec%d.bn_bwd2" % l, b, 1, dA, Y2, [A1], dYa, dA_bound)
            # the decoder's gB: overwritten by the encoder phase -> through the next BatchNorm backward
            e, bound = self.dgrad("dec%d.dgrad2" % l, b, 1, dYa, None, g["g16"])
            self.bn_backward("dec%d.bn_bwd1" % l, b, 0, e, Y1, ["up.%d" % l, "skip.%d" % l], dYb, bound)
            self.dgrad("dec%d.dgrad1" % l, b, 0, dYb, "dconcat.%d" % l, g["ctp"])
            dcat = T["dconcat.%d" % l]
            dUp = dcat[..., :C]
            self.close("dec%d.channel_sum" % l, "sums", "decoder%d.up.bias" % l, self.grad("decoder%d.up.bias" % l),
                       np.asarray(dUp, np.float64).sum((0, 1, 2)), np.abs(np.asarray(dUp, np.float64)).sum((0, 1, 2)))
            prev_block = ("bott",) if l == D else ("dec", l + 1)
            prevY = block_names(prev_block)[2]
            prevI = conv_index(c, prev_block, 1)
            up_w = self.param("decoder%d.up.weight" % l)
            if g["ctp"]:
                e, S, _ = convt_wgrad_stage(dUp, T["upin.%d" % l], up_w.shape)
                self.close("dec%d.up:wgrad(planes)" % l, "f32", "decoder%d.up.weight" % l, self.grad("decoder%d.up.weight" % l), e, S)
                dUp_op = dUp
            else:
                pch = self.chan(prevI)
                av, gap, und = operand_in_registers(T[prevY], pch["scale"].astype(np.float64), pch["shift"].astype(np.float64), c.slope)
                dUp_op = rne(dUp)                             # (a stored float32 tensor: its rounding in registers is exact to reproduce)
                e, S, wide = convt_wgrad_stage(dUp_op, av, up_w.shape, gap)
                self.close("dec%d.up:wgrad(regs)" % l, "f32", "decoder%d.up.weight" % l, self.grad("decoder%d.up.weight" % l), e, S, extra=wide)
            e, S = convt_dgrad_stage(dUp_op, up_w)
            half = g["ctp"]
            if l == D:
                self.close("dec%d.up:dgrad" % l, "conv16" if half else "f32", "gBottA", T["gBottA"], e, S, half_ulp=half)
                dA, dA_bound = T["gBottA"], None
            else:                                             # the decoder's gA.<l + 1>: overwritten -> composite
                bound = K_CONTRACTION * EPS * S
                if half:
                    bound = bound + 0.5 * ulp_bf16(np.abs(e) + bound)
                dA, dA_bound = e, bound
        b = ("bott",)
        Y1, A1, Y2, dYa, dYb = block_names(b)
        self.bn_backward("bott.bn_bwd2", b, 1, T["gBottA"], Y2, [A1], dYa)
        self.dgrad("bott.dgrad2", b, 1, dYa, "gBottB", g["g16"])
        self.bn_backward("bott.bn_bwd1", b, 0, T["gBottB"], Y1, ["pooled.%d" % D], dYb)
        self.dgrad("bott.dgrad1", b, 0, dYb, "dpool.%d" % D, g["g16"])
        for l in range(D, 0, -1):
            b = ("enc", l)
            Y1, A1, Y2, dYa, dYb = block_names(b)
            C = c.feat << (l - 1)
            ch = self.chan(conv_index(c, b, 1))
            arg, und, ties = pool_routes(T[Y2], ch["scale"].astype(np.float64), ch["shift"].astype(np.float64), c.slope)
            self.undecided += und
            self.tie_windows += ties
            merged = f32(T["dconcat.%d" % l][..., C:]) + route(f32(T["dpool.%d" % l]), arg)
            self.exact("enc%d.pool_bwd_merge" % l, "gA.%d" % l, T["gA.%d" % l], rne(merged) if g["g16"] else merged)
            self.bn_backward("enc%d.bn_bwd2" % l, b, 1, T["gA.%d" % l], Y2, [A1], dYa)
            self.dgrad("enc%d.dgrad2" % l, b, 1, dYa, "gB.%d" % l, g["g16"])
            self.bn_backward("enc%d.bn_bwd1" % l, b, 0, T["gB.%d" % l], Y1, ["xin" if l == 1 else "pooled.%d" % (l - 1)], dYb)
            if l > 1:
                self.dgrad("enc%d.dgrad1" % l, b, 0, dYb, "dpool.%d" % (l - 1), g["g16"])

    def run(self):
        self.forward()
        self.backward()
        self.padding()
        return self


def stage_table(c):
    """One row per launch of forward_planes / backward_planes: (launch, stored inputs, stored outputs, gate)."""
    g, D = gates(c), c.depth
    y = "bf16" if g["y16"] else "f32"
    gg = "bf16" if g["g16"] else "f32"
    rows = [("act_split", ["x"], ["xin"], "-")]

    def dconv(tag, block, segs):
        Y1, A1, Y2, _, _ = block_names(block)
        i1, i2 = conv_index(c, block, 0), conv_index(c, block, 1)
        rows.append(("pconv+stats %s.conv1" % tag, segs, [Y1 + ":" + y, "chan.%d" % i1], "y16_flow" if g["y16"] else "float32 Y"))
        rows.append(("act_split %s" % tag, [Y1, "chan.%d" % i1], [A1], "-"))
        rows.append(("pconv+stats %s.conv2" % tag, [A1], [Y2 + ":" + y, "chan.%d" % i2], "y16_flow" if g["y16"] else "float32 Y"))
    cur = "xin"
    for l in range(1, D + 1):
        dconv("enc%d" % l, ("enc", l), [cur])
        rows.append(("bn_relu_pool_planes enc%d" % l, ["encY2.%d" % l, "chan.%d" % conv_index(c, ("enc", l), 1)], ["skip.%d" % l, "pooled.%d" % l], "-"))
        cur = "pooled.%d" % l
    dconv("bott", ("bott",), [cur])
    prev = "bottY2"
    for l in range(D, 0, -1):
        C = c.feat << (l - 1)
        if g["ctp"]:
            rows.append(("act_split dec%d.upin" % l, [prev], ["upin.%d" % l], "convt_planes"))
            rows.append(("pconv(zblocks) dec%d.up" % l, ["upin.%d" % l], ["up.%d" % l], "convt_planes"))
        elif C % 16 == 0:
            rows.append(("conv(k2s2) dec%d.up" % l, [prev], ["up.%d:bf16" % l], "direct bf16 write (operand rounded in registers)"))
        else:
            rows.append(("conv(k2s2) dec%d.up" % l, [prev], ["upf.%d" % l], "float32 output (operand rounded in registers)"))
            rows.append(("act_split dec%d.up" % l, ["upf.%d" % l], ["up.%d" % l], "-"))
        dconv("dec%d" % l, ("dec", l), ["up.%d" % l, "skip.%d" % l])
        prev = "decY2.%d" % l
    rows.append(("head_fwd", ["decY2.1"], ["logits"], "vec: feat % 4"))
    rows.append(("loss turn-around", ["logits"], ["dlogits"], "test_gpu_loss_step.py"))
    rows.append(("head_bwd(+bn sums)", ["dlogits", "decY2.1"], ["grad final_conv.*", "gA.1 (decoder's: overwritten)"], "g16_flow: da16 + records"))

    def dback(tag, block, dA, segs, dx1, dx2):
        Y1, A1, Y2, dYa, dYb = block_names(block)
        rows.append(("bn_bwd_reduce|records + bn_bwd_apply %s.2" % tag, [dA, Y2], [dYa, "c1/c2", "grad bn, conv bias"], "-"))
        rows.append(("pwgrad %s.conv2" % tag, [dYa, A1], ["grad conv2.weight"], "side stream"))
        rows.append(("pconv(dgrad, bwd sums) %s.conv2" % tag, [dYa], [dx2], "g16_flow: bf16 + sums in the epilogue"))
        rows.append(("bn_bwd_apply %s.1" % tag, [dx2, Y1], [dYb, "c1/c2", "grad bn, conv bias"], "-"))
        rows.append(("pwgrad %s.conv1" % tag, [dYb] + segs, ["grad conv1.weight"], "side stream"))
        if dx1:
            rows.append(("pconv(dgrad) %s.conv1" % tag, [dYb], [dx1], "-"))
    for l in range(1, D + 1):
        dback("dec%d" % l, ("dec", l), "gA.%d (decoder's)" % l, ["up.%d" % l, "skip.%d" % l], "dconcat.%d:%s" % (l, "bf16" if g["ctp"] else "f32"),
              "gB.%d (decoder's: overwritten):%s" % (l, gg))
        rows.append(("channel_sum dec%d" % l, ["dconcat.%d" % l], ["grad up.bias"], "-"))
        below = "gBottA" if l == D else "gA.%d (decoder's: overwritten)" % (l + 1)
        if g["ctp"]:
            rows.append(("pwgrad(k2s2) dec%d.up" % l, ["dconcat.%d" % l, "upin.%d" % l], ["grad up.weight"], "convt_planes"))
            rows.append(("pconv(k2s2, bwd sums) dec%d.up" % l, ["dconcat.%d" % l], [below + ":bf16"], "convt_planes"))
        else:
            rows.append(("wgrad(k2s2) dec%d.up" % l, ["dconcat.%d" % l, "bottY2" if l == D else "decY2.%d" % (l + 1)], ["grad up.weight"],
                         "operands rounded in registers"))
            rows.append(("conv(k2s2 dgrad) dec%d.up" % l, ["dconcat.%d" % l], [below + ":f32"], "operand rounded in registers"))
    dback("bott", ("bott",), "gBottA", ["pooled.%d" % D], "dpool.%d:%s" % (D, gg), "gBottB:" + gg)
    for l in range(D, 0, -1):
        rows.append(("pool_bwd_merge(_sums) enc%d" % l, ["encY2.%d" % l, "dconcat.%d" % l, "dpool.%d" % l], ["gA.%d:%s" % (l, gg)], "vec: feat % 4; g16_flow: da16"))
        dback("enc%d" % l, ("enc", l), "gA.%d" % l, ["xin" if l == 1 else "pooled.%d" % (l - 1)], "dpool.%d:%s" % (l - 1, gg) if l > 1 else None,
              "gB.%d:%s" % (l, gg))
    return rows


# ------------------------------------------------------------------------------------------------------------ device reader
def read_device(m, c, x, n=None, h=None, w=None, pads=None):
    """Every tensor of the table from a model that has just run forward_backward(x, y)."""
    T = {"x": np.asarray(x, np.float32)}
    for name in tensor_names(c) + ["logits", "dlogits"]:
        T[name] = m.debug_tensor(name).reshape(shape_of(c, name, n, h, w))
    n_conv = 4 * c.depth + 2
    T["chan"] = [None] * n_conv
    for i in range(n_conv):
        v = m.debug_tensor("chan.%d" % i)
        T["chan"][i] = split_chan(v, v.size // 8)
    T["grad"] = {}
    from oracle import unet_ref
    for name, shape, kind in unet_ref.unet_entries(c.in_ch, 1, c.feat, c.depth):
        if kind == "param":
            T["grad"][name] = m.grad(name)
    T["pad_bwd"] = read_pads(m, c)
    if pads is not None:
        T["pad_fwd"] = pads
    return T


def read_pads(m, c, forward_only=False):
    out = OrderedDict()
    for name, C in plane_names(c).items():
        if forward_only and name.startswith("dY"):
            continue
        v = m.debug_tensor(name + ":pad")
        assert v.size % max(1, (-C) % 16) == 0 and (v.size == 0) == (C % 16 == 0), (name, v.size, C)
        out[name] = v
    return out


# ------------------------------------------------------------------------------------------------------------ the CPU stand-in
class StandIn:
    """A plain float32 emulation of the flow: every named tensor of a case, the accumulation by torch's float32 conv on the
    bf16-rounded operands.  ``mutate``: {name: function(stage inputs ...)} hooks of the host test's mutations."""

    def __init__(self, case, state, x, y, mutate=None):
        self.c, self.g = case._replace(slope=float(np.float32(case.slope))), gates(case)
        self.st = {k: v.numpy() if hasattr(v, "numpy") else np.asarray(v) for k, v in state.items()}
        self.x, self.y = np.asarray(x, np.float32), np.asarray(y)
        self.mut = mutate or {}
        self.T = {"x": self.x, "chan": [None] * self.n_convs(), "grad": {}, "pad_fwd": OrderedDict(), "pad_bwd": OrderedDict()}

    # the layers' places in the device's `convs` (the ResNet-encoder stand-in of tests/resnet_bf16_stages.py has other ones)
    def n_convs(self):
        return 4 * self.c.depth + 2

    def ci(self, block, which):
        return conv_index(self.c, block, which)

    def cp(self, i):
        return conv_prefix(self.c, i)

    # float32 contractions on bf16-rounded operands
    @staticmethod
    def _t32(a):
        return torch.from_numpy(f32(a)).permute(0, 3, 1, 2).contiguous()

    @staticmethod
    def _n32(t):
        return t.permute(0, 2, 3, 1).contiguous().numpy()

    def _wb(self, name):
        return torch.from_numpy(rne(self.st[name]))

    def hook(self, name, value, **kw):
        fn = self.mut.get(name)
        return fn(value, **kw) if fn else value

    def store16(self, name, acc):
        """A contraction's float32 accumulators -> what the flow stores under `name` (rounded to nearest even)."""
        fn = self.mut.get("round:" + name)
        return fn(acc) if fn else rne(acc)

    def conv_bn(self, block, which, segs, out_name):
        c, T = self.c, self.T
        i = self.ci(block, which)
        p, ci, bi = self.cp(i)
        x = np.concatenate([T[s] for s in segs], -1)
        acc = self._n32(F.conv2d(self._t32(x), self._wb("%s.%d.weight" % (p, ci)), torch.from_numpy(self.st["%s.%d.bias" % (p, ci)]), padding=1))
        Y = self.store16(out_name, acc) if self.g["y16"] else acc
        Y = self.hook("out:" + out_name, Y)
        T[out_name] = Y
        src = self.hook("stats_source:" + out_name, Y, acc=acc)
        mean, invstd, _ = stats_stage(src)
        mean, invstd = mean.astype(np.float32), invstd.astype(np.float32)
        sc, sh = bn_coeffs32(self.st["%s.%d.weight" % (p, bi)], self.st["%s.%d.bias" % (p, bi)], mean, invstd)
        C = Y.shape[-1]
        T["chan"][i] = {"running_mean": np.zeros(C, np.float32), "running_var": np.ones(C, np.float32), "mean": mean, "invstd": invstd,
                        "scale": sc, "shift": sh, "c1": np.zeros(C, np.float32), "c2": np.zeros(C, np.float32)}

    def act(self, src, i, out_name):
        ch = self.T["chan"][i]
        a, _ = act32(self.T[src], ch["scale"], ch["shift"], self.c.slope)
        self.T[out_name] = self.hook("out:" + out_name, self.store16(out_name, a))

    def double_conv(self, block, segs):
        Y1, A1, Y2, _, _ = block_names(block)
        self.conv_bn(block, 0, segs, Y1)
        self.act(Y1, self.ci(block, 0), A1)
        self.conv_bn(block, 1, [A1], Y2)
        return Y2, self.ci(block, 1)

    def forward(self):
        c, T, g, D = self.c, self.T, self.g, self.c.depth
        T["xin"] = self.hook("out:xin", self.store16("xin", self.x))
        self.forward_decoder(self.forward_encoder("xin"))
        self.record_pads("pad_fwd", forward_only=True)

    def forward_encoder(self, cur):
        """-> the name of the bottleneck's input; leaves skip.<l>."""
        c, T, D = self.c, self.T, self.c.depth
        for l in range(1, D + 1):
            Y2, i2 = self.double_conv(("enc", l), [cur])
            ch = T["chan"][i2]
            a, _ = act32(T[Y2], ch["scale"], ch["shift"], c.slope)
            N, H, W, C = a.shape
            T["skip.%d" % l] = self.hook("out:skip.%d" % l, rne(a))
            T["pooled.%d" % l] = self.hook("out:pooled.%d" % l, rne(a.reshape(N, H // 2, 2, W // 2, 2, C).max((2, 4))))
            cur = "pooled.%d" % l
        return cur

    def forward_decoder(self, cur):
        c, T, g, D = self.c, self.T, self.g, self.c.depth
        prevY, prevI = self.double_conv(("bott",), [cur])
        for l in range(D, 0, -1):
            ch = T["chan"][prevI]
            a, _ = act32(T[prevY], ch["scale"], ch["shift"], c.slope)
            a16 = rne(a)
            if g["ctp"]:
                T["upin.%d" % l] = self.hook("out:upin.%d" % l, a16)
                a16 = T["upin.%d" % l]
            acc = self._n32(F.conv_transpose2d(self._t32(a16), self._wb("decoder%d.up.weight" % l), torch.from_numpy(self.st["decoder%d.up.bias" % l]),
                                               stride=2))
            if not g["ctp"] and (c.feat << (l - 1)) % 16:
                T["upf.%d" % l] = acc
            T["up.%d" % l] = self.hook("out:up.%d" % l, self.store16("up.%d" % l, acc))
            prevY, prevI = self.double_conv(("dec", l), ["up.%d" % l, "skip.%d" % l])
        ch = T["chan"][prevI]
        a, _ = act32(T[prevY], ch["scale"], ch["shift"], c.slope)
        w = self.st["final_conv.weight"].reshape(-1)
        T["logits"] = ((a * w).sum(-1, keepdims=True, dtype=np.float32) + self.st["final_conv.bias"][0]).astype(np.float32)

    def record_pads(self, when, forward_only=False):
        for name, C in plane_names(self.c).items():
            if forward_only and name.startswith("dY"):
                continue
            shp = shape_of(self.c, name)
            v = np.zeros((int(np.prod(shp[:3])), (-C) % 16), np.float32)
            self.T[when][name] = self.hook("pad:%s:%s" % (when, name), v)

    def loss_turnaround(self):
        from oracle import unet_ref
        lg = torch.from_numpy(self.T["logits"]).permute(0, 3, 1, 2).clone().requires_grad_(True)
        loss = unet_ref.segmentation_loss(lg, torch.from_numpy(self.y.astype(np.float32)).unsqueeze(1))
        (d,) = torch.autograd.grad(loss, lg)
        self.loss = float(loss.detach())
        self.T["dlogits"] = d.permute(0, 2, 3, 1).contiguous().numpy()

    def bn_backward(self, block, which, dA, Y_name, x_segs, dY_name):
        c, T = self.c, self.T
        i = self.ci(block, which)
        p, ci, bi = self.cp(i)
        ch, Y = T["chan"][i], T[Y_name]
        z = f32(Y) * ch["scale"] + ch["shift"]
        dz = np.where(z > 0, f32(dA), f32(dA) * np.float32(c.slope)).astype(np.float64)
        xh = ((f32(Y) - ch["mean"]) * ch["invstd"]).astype(np.float64)
        M = Y.size // Y.shape[-1]
        s1, s2 = dz.sum((0, 1, 2)), (dz * xh).sum((0, 1, 2))
        ch["c1"], ch["c2"] = (s1 / M).astype(np.float32), (s2 / M).astype(np.float32)
        T["grad"]["%s.%d.bias" % (p, bi)] = s1.astype(np.float32)
        T["grad"]["%s.%d.weight" % (p, bi)] = s2.astype(np.float32)
        o = bn_apply32(dA, Y, ch, self.st["%s.%d.weight" % (p, bi)], c.slope)
        o = self.hook("dy32:" + dY_name, o, chan=ch, gamma=self.st["%s.%d.weight" % (p, bi)])
        T["grad"]["%s.%d.bias" % (p, ci)] = o.astype(np.float64).sum((0, 1, 2)).astype(np.float32)
        T[dY_name] = self.hook("out:" + dY_name, self.store16(dY_name, o))
        x = np.concatenate([T[s] for s in x_segs], -1)
        wn = "%s.%d.weight" % (p, ci)
        T["grad"][wn] = torch.nn.grad.conv2d_weight(self._t32(x), self.st[wn].shape, self._t32(T[dY_name]), padding=1).numpy()

    def dgrad(self, block, which, dY_name, out_name, half):
        p, ci, _ = self.cp(self.ci(block, which))
        acc = self._n32(F.conv_transpose2d(self._t32(self.T[dY_name]), self._wb("%s.%d.weight" % (p, ci)), padding=1))
        out = self.store16(out_name, acc) if half else acc
        return self.hook("out:" + out_name, out)

    def backward(self):
        self.loss_turnaround()
        self.backward_decoder("pooled.%d" % self.c.depth)
        self.backward_encoder()
        self.record_pads("pad_bwd")

    def backward_decoder(self, bott_in):
        """Head, decoders, bottleneck -> dconcat.<l>, dpool.<depth>."""
        c, T, g, D = self.c, self.T, self.g, self.c.depth
        d = T["dlogits"]
        ch = T["chan"][self.ci(("dec", 1), 1)]
        a, _ = act32(T["decY2.1"], ch["scale"], ch["shift"], c.slope)
        T["grad"]["final_conv.weight"] = (d.astype(np.float64) * a).sum((0, 1, 2)).astype(np.float32).reshape(self.st["final_conv.weight"].shape)
        T["grad"]["final_conv.bias"] = np.array([d.astype(np.float64).sum()], np.float32)
        da = f32(d) * f32(self.st["final_conv.weight"].reshape(-1))
        dA = rne(da) if g["g16"] else da
        for l in range(1, D + 1):
            b = ("dec", l)
            Y1, A1, Y2, dYa, dYb = block_names(b)
            C = c.feat << (l - 1)
            self.bn_backward(b, 1, dA, Y2, [A1], dYa)
            gB = self.dgrad(b, 1, dYa, "gB_dec.%d" % l, g["g16"])
            self.bn_backward(b, 0, gB, Y1, ["up.%d" % l, "skip.%d" % l], dYb)
            T["dconcat.%d" % l] = self.dgrad(b, 0, dYb, "dconcat.%d" % l, g["ctp"])
            dUp = T["dconcat.%d" % l][..., :C]
            T["grad"]["decoder%d.up.bias" % l] = dUp.astype(np.float64).sum((0, 1, 2)).astype(np.float32)
            prev_block = ("bott",) if l == D else ("dec", l + 1)
            prevY, prevI = block_names(prev_block)[2], self.ci(prev_block, 1)
            if g["ctp"]:
                aop = T["upin.%d" % l]
            else:
                pch = T["chan"][prevI]
                aop = rne(act32(T[prevY], pch["scale"], pch["shift"], c.slope)[0])
            dUp16 = rne(dUp)
            wn = "decoder%d.up.weight" % l
            T["grad"][wn] = torch.nn.grad.conv2d_weight(self._t32(dUp16), self.st[wn].shape, self._t32(aop), stride=2).numpy()
            acc = self._n32(F.conv2d(self._t32(dUp16), self._wb(wn), stride=2))
            below = "gBottA" if l == D else "gA_dec.%d" % (l + 1)
            dA = self.hook("out:" + below, self.store16(below, acc) if g["ctp"] else acc)
            if l == D:
                T["gBottA"] = dA
        b = ("bott",)
        Y1, A1, Y2, dYa, dYb = block_names(b)
        self.bn_backward(b, 1, T["gBottA"], Y2, [A1], dYa)
        T["gBottB"] = self.dgrad(b, 1, dYa, "gBottB", g["g16"])
        self.bn_backward(b, 0, T["gBottB"], Y1, [bott_in], dYb)
        T["dpool.%d" % D] = self.dgrad(b, 0, dYb, "dpool.%d" % D, g["g16"])

    def backward_encoder(self):
        c, T, g, D = self.c, self.T, self.g, self.c.depth
        for l in range(D, 0, -1):
            b = ("enc", l)
            Y1, A1, Y2, dYa, dYb = block_names(b)
            C = c.feat << (l - 1)
            ch = T["chan"][self.ci(b, 1)]
            a, _ = act32(T[Y2], ch["scale"], ch["shift"], c.slope)
            N, H, W, _ = a.shape
            aw = a.reshape(N, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, C, 4)
            arg = self.hook("route:%d" % l, aw.argmax(-1), windows=aw)
            merged = f32(T["dconcat.%d" % l][..., C:]) + route(f32(T["dpool.%d" % l]), arg)
            T["gA.%d" % l] = self.hook("out:gA.%d" % l, self.store16("gA.%d" % l, merged) if g["g16"] else merged)
            self.bn_backward(b, 1, T["gA.%d" % l], Y2, [A1], dYa)
            T["gB.%d" % l] = self.dgrad(b, 1, dYa, "gB.%d" % l, g["g16"])
            self.bn_backward(b, 0, T["gB.%d" % l], Y1, ["xin" if l == 1 else "pooled.%d" % (l - 1)], dYb)
            if l > 1:
                T["dpool.%d" % (l - 1)] = self.dgrad(b, 0, dYb, "dpool.%d" % (l - 1), g["g16"])

    def run(self):
        self.forward()
        self.backward()
        return self.T


def check(case, state, T):
    return Checker(case, state, T).run()
