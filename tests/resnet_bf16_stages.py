"""The ResNet-encoder U-Net's bfloat16 data flow, stage by stage (model_planes.cpp: forward_resnet_planes / backward_resnet_planes).
Importable without a GPU: test_resnet_bf16_stages_host.py runs the checker on a CPU stand-in and on mutations of it,
test_gpu_resnet_bf16_stages.py runs it on the tensors the device leaves behind (``UNetResNet18.debug_tensor``).

METHOD, CRITERIA and constants are those of tests/unet_bf16_stages.py (teacher forcing: a float64 oracle of ONE launch, fed the tensors
the device itself stored as that launch's inputs; classes elem / conv16 / f32 / sums / stats / pad / composite; k = 16 for contractions,
sums and statistics, k = 4 for the float32 rounding of a composite row's own element-wise step; eps = 2^-24), imported and not restated.
The decoder, bottleneck, head and loss rows are the plain U-Net's code and are checked there; here dconcat.<l> and rdpool are stored
INPUTS.

THE STAGE TABLE is ``stage_table(case)``: one row per launch, in launch order, with its stored inputs, stored outputs and kind.
Blocks b = 0..7 (level b // 2 + 1; b = 2, 4, 6 have stride 2 and a 1x1 stride-2 projection).

 forward, all DIRECT
  xin                 elem    = RNE(input); xin:pad zero after the forward and after the backward pass
  stemY, rY1 rYd rY2  conv16  3x3 stride 1 / 3x3 stride 2 read from the full-resolution planes / 1x1 stride 2; no conv bias
  chan.<i> mean, invstd  stats   of the ROUNDED stored values (conv_planes.hip, finish_quarter: the value is rounded first, then p1 += v,
                              p2 += v * v -- one epilogue serves the stride-2 and the 1x1 forms, confirmed by the stats rows here)
  chan.<i> scale, shift  elem
  a0, rA1.<b>         elem    act_split: relu(y * scale + shift), one rounding
  rA.<b>              elem    bn_add_relu16: v = y * sc + sh; u = s (identity) or s * ssc + ssh (projection); fmaxf(v + u, 0); one rounding
  rskip == rA.7       elem    bn_relu_pool_planes with identity scale / shift
  rpool               elem    = 2x2 max of rA.7
  rA.<b>, b = 1, 3, 5 IS the skip tensor decoder b // 2 + 1 reads (make_plane_slots: r.A = pSkip[level]): debug_tensor serves
                      rA.<b> out of pl[pSkip[level]] itself, there is no second tensor to compare it with.  ("concat.<l>" of this
                      model is the float32 path's buffer, which this flow never writes: nothing of this pass can be read there.)
 backward, DIRECT
  all 20 weight gradients  f32   the float64 contraction of the two STORED operands (a_in / rA1 / xin and rdY1 / rdY2 / rdYd / dY0),
                              the stride-2 3x3 and 1x1 forms on the plane weight-gradient kernel included
  block 0 and the stem     rdz.0 -> rdY2.0 elem; rdA1 conv16; bn1's c1 / c2 / dgamma / dbeta out of that launch's epilogue (sums);
                           rdY1.0 elem; rdX conv16; rdz.1 = RNE(rdX + rdz.0) elem; the stem's sums; dY0 elem
  dgamma / dbeta, c1 / c2  sums  wherever the summed tensor is stored (block 0, the stem), else composite (below)
 backward, COMPOSITE (the scratch rdz.* / rdA1 / rdX is overwritten by the later blocks: checked THROUGH the BatchNorm backward)
  dz_7                = mask(rA.7) * pool_bwd_merge(rA.7, rdpool, upper half of dconcat.4): every input is stored and the launch is
                        reproduced bit for bit, so rdY2.7 is an elem row (a composite with bound 0)
  dz_<b-1>, b stride 2  mask(rA.<b-1>) * (bf16(conv2d_input of the 3x3 stride-2 conv from rdY1.<b> + conv2d_input of the 1x1 stride-2
                        conv from rdYd.<b>) + upper half of dconcat.<level-1>), in float64 from stored tensors; bound: the contraction
                        criterion + half a bf16 ulp per stored intermediate (rdX, then dz).  The oracle is torch's conv2d_input,
                        not the class decomposition: this is where the class tables, osy/osx/ooy/oox and the second K segment show
  dz_<b-1>, b stride 1  mask(rA.<b-1>) * (bf16(input gradient of conv1 from rdY1.<b>) + dz_<b>), dz_<b> CARRIED from the previous
                        composite's float64 value with its bound (horizon two launches; the bounds add).  A wrong dz_<b> therefore
                        also shows in block b - 1's rows
  rdY2.<b>, rdYd.<b>  within |gamma invstd| x bound + its own rounding (k = 4) of gamma invstd (dz - c1 - xhat c2) with the device's c1, c2
  same_dz             rdYd.<b> and rdY2.<b> of a stride-2 block come from ONE dz: dz solved from either must agree within the two
                        tensors' own rounding, whatever the chain above did (class "composite", limit 1)
  rdY1.<b>, b > 0     bf16(input gradient of conv2 from rdY2.<b>) -> BatchNorm-backward apply, as the decoder's gB in the U-Net module
  rdz.0               block 0's dz is stored: the composite oracle (dX_1 + dz_1, both unreadable) against the stored tensor

WHAT CANNOT BE READ: dz_<b>, dA1_<b>, dX_<b> of blocks 1..7 and the pool backward's merge (scratch shared by all blocks: composite rows
above); the class filter tables (seen through dz_<b-1>); the float32 accumulators of any contraction.

WHICH VALUES THE SUMS ARE OF (read in the code, tested exactly so)
  * bn2 / the projection's BatchNorm / the stem: bn_bwd_reduce reads the STORED dz (rdz.*) and the stored raw output; slope 1 for
    bn2 and the projection (the residual branches have no activation of their own: no mask), the ReLU mask for the stem.
  * bn1: out of conv2's input-gradient launch (PConvArgs::bwd_*, rec1): of dA1 AS STORED (rounded to bf16 first), masked by
    rY1 * scale + shift > 0.
  * the masks of relu_mask_sum16 read the stored bf16 block output: decided exactly.  The activation derivative inside a BatchNorm
    backward (bn1, the stem) is undecided within 4 eps (|y scale| + |shift|) of 0; the cap is zero undecided per case.

MEASURED on an MI355X (the RESNETBF16 lines of test_gpu_resnet_bf16_stages.py): the worst ratio of each class against its k and the
tensor it belongs to.  conv16 counts what is left of |g - e| after the half ulp, in units of eps S.  elem: 0 differing elements, pad: 0 non-zero
lanes, undecided masks: 0 in every row.  "composite" is same_dz's ratio against its limit 1: the two tensors' rounding errors are
independent and each reaches its half ulp somewhere among thousands of elements, so the worst ratio approaches 1 from below by
construction (0.997 on the CPU stand-in too); a dz that differed between the two branches would show as a ratio of tens.  No class
needs more than k = 16, at K = 4608 (conv2 of blocks 6, 7 of f64_1x32x32: 9 x 512) and on the strided kernels included; the CPU
stand-in, another summation order, shows about conv16 0.7, f32 5.8, sums 1.3, stats 0.95 over the same cases.

  case                              conv16 (k 16)   f32 (k 16)                    sums (k 16)       stats (k 16)        same_dz (1)   ties
  f16_1x32x48                       0.39  rdY1.3    2.83 layer4.1.conv2.weight    1.18 chan.19.c2   0.75 chan.5.mean    0.992         11
  f16_3x16x16                       0.21  rdY1.4    2.14 layer3.1.conv1.weight    1.35 chan.19.c2   0.94 chan.7.mean    0.999         1
  f32_2x32x32                       0.37  rdY2.6    2.99 layer4.1.conv1.weight    1.12 chan.19.c2   0.95 chan.5.mean    0.997         37
  f64_1x32x32                       0.51  rdY1.4    2.91 layer3.1.conv1.weight    1.59 chan.19.c2   0.84 chan.18.mean   0.998         36
  f16 at 1x16x32 after 1x32x64      0.15  rY1.7     2.14 layer3.1.conv1.weight    1.62 chan.19.c2   0.66 chan.4.mean    0.992         0
  f16 at 1x32x64 after 1x16x32      0.81  rdY1.3    2.09 layer4.1.conv1.weight    1.05 chan.19.c2   0.97 chan.7.mean    0.998         31
  (rdY1.<b>, rdY2.<b> under conv16 are composite rows: the contraction's bound carried through the BatchNorm backward, k = 4 for
  its own float32 steps.  The worst ratio is taken over the direct conv16 rows -- stride 1, stride 2, 1x1 -- and these alike.)

FOUND: nothing.  Every stage of every case, and both stage-checked runs after a shape change, hold their contract as read from
the code on the first device run; no kernel was changed.  The library change of this work is the read-only debug branch.

MUTATIONS of the CPU stand-in (value changes only; test_resnet_bf16_stages_host.py asserts each fails and where).  "whole-model":
whether test_gpu_resnet_unet.py's criterion (rel_same <= max(1.1 rel_arith, 1e-2) per gradient, loss to 3e-3, logits) evaluated on
the mutated stand-in against oracle/resnet_unet_ref.py would have noticed.
Evaluated at f32_2x32x32 and f64_1x32x32 (the same verdicts at both, except where noted).
  mutation                                              rows that fail                                      whole-model criterion
  bn_add_relu16 truncates, one block                    block<b>.bn_add_relu16 (rA.<b>) only                GREEN (all eight blocks at once: noticed)
  class 0 without the projection segment, block b       block<b-1>.bn2, carried: block<b-2>.bn2 / .bnd      GREEN at b = 6 (b = 2, 4, 6 at once: noticed)
  classes 1 and 2 written at each other's offsets, b    block<b-1>.bn2, carried: block<b-2>.bn2 / .bnd      b = 6: GREEN at width 64, 2 of 99 gradients at width 32
  relu_mask_sum16 drops the skip-gradient term, b odd   block<b>.bn2, carried: block<b-1>.bn2 / .bnd        noticed
  stride-2 conv reads row 2 y + r                       block<b>.conv1 (rY1.<b>) only                       noticed
  bn1's folded sums over the unrounded accumulators     block0.bn1 (sums) only                              GREEN, also with every block mutated
  pool backward routes ties to the last maximum         block7.bn2, carried: block6.bn2 / .bnd              GREEN
  LIMIT: the folded sums of blocks 1..7 are composite rows (dA1 is overwritten) whose bound, the sum of the per-element bounds of
  dA1, is wider than the difference between rounded and unrounded sums: that mutation is seen at block 0 only, where rdA1 is stored.
  One launch form serves all eight blocks (PConvArgs::bwd_* in the stride-1 3x3 input-gradient kernel).
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import unet_bf16_stages as S
from unet_bf16_stages import (EPS, INVSTD_RTOL, K_CONTRACTION, K_ELEM, Case, Criteria, Layer, act32, bn_apply32, bn_coeffs32, f32, is_bf16,  # noqa: F401
                              rne, route, split_chan, stats_stage, trunc_bf16, ulp_bf16, wgrad_stage)

TAG = "RESNETBF16"
DEPTH = 4
N_ENC_CONVS = 20                # stem + 8 x (conv1, conv2) + 3 projections; the bottleneck's first conv is convs[20]

CASES = [
    Case("f16_1x32x48", 3, 16, DEPTH, 1, 32, 48, 0.0, 0, ("skipgrad:f32", "map:ragged", "map:smaller", "shortcut:identity", "shortcut:projection")),
    Case("f16_3x16x16", 3, 16, DEPTH, 3, 16, 16, 0.0, 2, ("skipgrad:f32", "batch:3", "map:equal", "map:smaller", "pooled:1x1")),
    Case("f32_2x32x32", 3, 32, DEPTH, 2, 32, 32, 0.0, 0, ("skipgrad:bf16", "batch:2", "map:equal")),
    Case("f64_1x32x32", 3, 64, DEPTH, 1, 32, 32, 0.0, 0, ("skipgrad:bf16", "K:4608", "class0:multi_chunk")),
]
# (f16_3x16x16 has seed 2: its bottleneck normalises over 3 values per channel, so the float32 and the bf16-operand oracle differ by
# 30 - 90 % of a gradient's norm between themselves, and the whole-model criterion the host test ties the stand-in to is a
# comparison of two such noises there: seeds 0 and 1 miss it by up to 15 %, seeds 2, 3, 4 hold it.  Every seed passes the stage
# table with zero undecided.)
BY_ID = OrderedDict((c.id, c) for c in CASES)
RESHAPE_BASE = "f16_1x32x48"
RESHAPE_SEQUENCE = [(1, 32, 64), (1, 16, 32), (1, 32, 64)]
ALL_GATE_VALUES = ["skipgrad:f32", "skipgrad:bf16", "shortcut:identity", "shortcut:projection", "map:smaller", "map:equal", "map:ragged",
                   "batch:2", "batch:3", "pooled:1x1", "K:4608", "class0:multi_chunk"]
TILES = ((8, 32), (16, 16), (8, 8))          # the output tiles of the plane conv kernel


def gate_values(c):
    v = {"skipgrad:bf16" if c.feat % 32 == 0 else "skipgrad:f32", "shortcut:identity", "shortcut:projection"}
    for l in range(1, DEPTH + 1):
        hh, ww = c.h >> (l - 1), c.w >> (l - 1)
        if hh < 8 or ww < 8:
            v.add("map:smaller")                                   # smaller than the smallest tile
        elif (hh, ww) in TILES:
            v.add("map:equal")
        elif any(hh % th or ww % tw for th, tw in TILES):
            v.add("map:ragged")
    if c.n > 1:
        v.add("batch:%d" % c.n)
    if (c.h >> DEPTH, c.w >> DEPTH) == (1, 1):
        v.add("pooled:1x1")
    if 9 * (c.feat << 3) == 4608:
        v.add("K:4608")
    if (c.feat << 2) > 128:                                      # class 0 of block 6: two K segments of more than one 128-channel step
        v.add("class0:multi_chunk")
    return v


# ------------------------------------------------------------------------------------------------------------ topology and names
class Block:
    def __init__(self, c, b, first):
        self.b, self.level, self.stride = b, b // 2 + 1, 2 if (b and b % 2 == 0) else 1
        self.cout = c.feat << (self.level - 1)
        self.cin = self.cout // 2 if self.stride == 2 else self.cout
        self.c1, self.c2, self.cd = first, first + 1, (first + 2 if self.stride == 2 else -1)
        p = "layer%d.%d" % (self.level, b & 1)
        self.L1 = Layer(self.c1, p + ".conv1.weight", None, p + ".bn1.weight", p + ".bn1.bias", self.stride, 1)
        self.L2 = Layer(self.c2, p + ".conv2.weight", None, p + ".bn2.weight", p + ".bn2.bias", 1, 1)
        self.Ld = Layer(self.cd, p + ".downsample.0.weight", None, p + ".downsample.1.weight", p + ".downsample.1.bias", 2, 0) if self.stride == 2 else None
        self.a_in = "a0" if b == 0 else "rA.%d" % (b - 1)

    def layers(self):
        return [L for L in (self.L1, self.L2, self.Ld) if L]


STEM = Layer(0, "stem.0.weight", None, "stem.1.weight", "stem.1.bias", 1, 1)


def blocks(c):
    out, first = [], 1
    for b in range(8):
        out.append(Block(c, b, first))
        first += 3 if out[-1].stride == 2 else 2
    assert first == N_ENC_CONVS
    return out


def tensor_names(c):
    """Every encoder tensor the checker reads besides x / chan.<i> / the gradients / dconcat.<l>."""
    names = ["xin", "stemY", "a0", "dY0", "rskip", "rpool", "rdpool", "rdz.0", "rdz.1", "rdA1", "rdX"]
    for k in blocks(c):
        names += ["%s.%d" % (t, k.b) for t in ("rY1", "rY2", "rA1", "rA", "rdY1", "rdY2")]
        if k.stride == 2:
            names += ["rYd.%d" % k.b, "rdYd.%d" % k.b]
    return names


def shape_of(c, name, n=None, h=None, w=None):
    n, h, w = n or c.n, h or c.h, w or c.w
    base, _, idx = name.partition(".")
    if base == "xin":
        return (n, h, w, c.in_ch)
    if base in ("rskip", "rpool", "rdpool"):
        d = DEPTH - 1 if base == "rskip" else DEPTH
        return (n, h >> d, w >> d, c.feat << (DEPTH - 1))
    if base == "dconcat":
        l = int(idx)
        return (n, h >> (l - 1), w >> (l - 1), 2 * (c.feat << (l - 1)))
    if base in ("stemY", "a0", "dY0", "rdz", "rdA1", "rdX"):
        return (n, h, w, c.feat)
    l = int(idx) // 2 + 1
    return (n, h >> (l - 1), w >> (l - 1), c.feat << (l - 1))


# ------------------------------------------------------------------------------------------------------------ inputs
def init_state(c):
    from oracle import resnet_unet_ref
    st = resnet_unet_ref.init_state(c.in_ch, 1, c.feat, seed=c.seed)
    g = torch.Generator().manual_seed(c.seed + 500)
    for k in list(st):                             # BatchNorm weights and biases away from (1, 0), as the U-Net module's
        if st[k].ndim == 1 and k[:-len(k.split(".")[-1])] + "running_mean" in st:
            if k.endswith(".weight"):
                st[k] = 0.5 + torch.rand(st[k].shape, generator=g)
            elif k.endswith(".bias"):
                st[k] = 0.4 * torch.rand(st[k].shape, generator=g) - 0.2
    return st


inputs = S.inputs


# ------------------------------------------------------------------------------------------------------------ float64 stage functions
def conv_stage(x, w, stride, pad):
    """y = conv(x, bf16(w)) (the encoder's convs have no bias) -> (e, S)."""
    xt, wt = S._t(x), S._w(w)
    return S._n(F.conv2d(xt, wt, stride=stride, padding=pad)), S._n(F.conv2d(xt.abs(), wt.abs(), stride=stride, padding=pad))


def conv_input_stage(dy, w, in_hw, stride, pad):
    """dx = torch's conv2d_input: the adjoint of conv(stride, pad) applied to dy."""
    dt, wt = S._t(dy), S._w(w)
    shp = (dt.shape[0], wt.shape[1]) + tuple(in_hw)
    return (S._n(torch.nn.grad.conv2d_input(shp, wt, dt, stride=stride, padding=pad)),
            S._n(torch.nn.grad.conv2d_input(shp, wt.abs(), dt.abs(), stride=stride, padding=pad)))


def contraction_bound(e, Sv, half=True):
    b = K_CONTRACTION * EPS * Sv
    return b + 0.5 * ulp_bf16(np.abs(e) + b) if half else b


def bn_add_relu32(Y2, ch2, s, chd=None):
    """bn_add_relu16 in float32, operation by operation, before its one rounding."""
    v = f32(Y2) * ch2["scale"] + ch2["shift"]
    u = f32(s) if chd is None else f32(s) * chd["scale"] + chd["shift"]
    return np.maximum(v + u, np.float32(0))


def windows(a):
    N, H, W, C = a.shape
    return a.reshape(N, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, C, 4)


# ------------------------------------------------------------------------------------------------------------ the checker
class Checker(Criteria):
    """The encoder's stage table over a tensor dictionary T (device or stand-in): T[name] NHWC float32 arrays under the
    debug_tensor names, "x", "dconcat.<l>"; T["chan"][i]; T["grad"][name]; T["pad_fwd"] / T["pad_bwd"]["xin"]."""
    TAG = TAG

    def __init__(self, case, state, T):
        super().__init__()
        self.c, self.T = case, T
        self.st = {k: v.numpy() if hasattr(v, "numpy") else np.asarray(v) for k, v in state.items()}
        self.blocks = blocks(case)

    def skip_grad(self, level):
        C = self.c.feat << (level - 1)
        return self.T["dconcat.%d" % level][..., C:]

    # -- forward
    def conv_bn(self, stage, L, x_name, out_name):
        T = self.T
        e, Sv = conv_stage(T[x_name], self.param(L.w), L.stride, L.pad)
        self.close(stage, "conv16", out_name, T[out_name], e, Sv, half_ulp=True)
        ch = self.chan(L.i)
        self.stats(stage, L.i, ch, T[out_name])
        sc, sh = bn_coeffs32(self.param(L.gamma), self.param(L.beta), ch["mean"], ch["invstd"])
        self.exact(stage + ":coeffs", "chan.%d.scale" % L.i, ch["scale"], sc)
        self.exact(stage + ":coeffs", "chan.%d.shift" % L.i, ch["shift"], sh)

    def act(self, stage, src, i, out_name):
        ch = self.chan(i)
        self.exact(stage, out_name, self.T[out_name], rne(act32(self.T[src], ch["scale"], ch["shift"], 0.0)[0]))

    def forward(self):
        T = self.T
        self.exact("act_split(x)", "xin", T["xin"], rne(T["x"]))
        self.conv_bn("stem.conv", STEM, "xin", "stemY")
        self.act("stem.act_split", "stemY", 0, "a0")
        for k in self.blocks:
            b, tag = k.b, "block%d" % k.b
            self.conv_bn(tag + ".conv1", k.L1, k.a_in, "rY1.%d" % b)
            if k.Ld:
                self.conv_bn(tag + ".proj", k.Ld, k.a_in, "rYd.%d" % b)
            self.act(tag + ".act_split", "rY1.%d" % b, k.c1, "rA1.%d" % b)
            self.conv_bn(tag + ".conv2", k.L2, "rA1.%d" % b, "rY2.%d" % b)
            o = bn_add_relu32(T["rY2.%d" % b], self.chan(k.c2), T["rYd.%d" % b] if k.Ld else T[k.a_in], self.chan(k.cd) if k.Ld else None)
            self.exact(tag + ".bn_add_relu16", "rA.%d" % b, T["rA.%d" % b], rne(o))
        A = f32(T["rA.7"])
        self.exact("pool.bn_relu_pool_planes", "rskip", T["rskip"], A)
        self.exact("pool.bn_relu_pool_planes", "rpool", T["rpool"], windows(A).max(-1))

    # -- backward
    def masked_sum(self, terms, A):
        """dz = RNE(mask(A) * (float32 sum of the terms)): terms [(e, bound)] in float64 -> (e, bound of the stored value, S, the
        bound without dz's own rounding)."""
        m = np.asarray(A) > 0
        g = sum(np.asarray(e, np.float64) for e, _ in terms)
        Sv = sum(np.abs(np.asarray(e, np.float64)) for e, _ in terms)
        carried = sum(np.asarray(bd, np.float64) * np.ones_like(g) for _, bd in terms)
        own = K_ELEM * EPS * Sv
        total = carried + own
        total = total + 0.5 * ulp_bf16(np.abs(g) + total)
        return m * g, m * total, m * Sv, m * carried

    def block_backward(self, k, dz, dz_bound):
        """The rows of block k from (dz, dz_bound): dz_bound None -> dz is the bit-exact stored value.  -> (dz, bound, S, carried)
        of the block below (the stem's g for block 0)."""
        T, b, tag = self.T, k.b, "block%d" % k.b
        H, W = T[k.a_in].shape[1:3]
        self.bn_backward_layer(tag + ".bn2", k.L2, dz, "rY2.%d" % b, T["rA1.%d" % b], "rdY2.%d" % b, dz_bound, slope=1.0)
        if k.Ld:
            self.bn_backward_layer(tag + ".bnd", k.Ld, dz, "rYd.%d" % b, T[k.a_in], "rdYd.%d" % b, dz_bound, slope=1.0)
            self.same_dz(tag + ".same_dz", k)
        e1, S1 = conv_input_stage(T["rdY2.%d" % b], self.param(k.L2.w), T["rA1.%d" % b].shape[1:3], 1, 1)
        if b == 0:
            self.close(tag + ".dgrad2", "conv16", "rdA1", T["rdA1"], e1, S1, half_ulp=True)
            self.bn_backward_layer(tag + ".bn1", k.L1, T["rdA1"], "rY1.0", T[k.a_in], "rdY1.0")
        else:
            self.bn_backward_layer(tag + ".bn1", k.L1, e1, "rY1.%d" % b, T[k.a_in], "rdY1.%d" % b, contraction_bound(e1, S1))
        eX, SX = conv_input_stage(T["rdY1.%d" % b], self.param(k.L1.w), (H, W), k.stride, 1)
        if k.Ld:
            ep, Sp = conv_input_stage(T["rdYd.%d" % b], self.param(k.Ld.w), (H, W), 2, 0)
            eX, SX = eX + ep, SX + Sp
        if b == 0:
            self.close(tag + ".dgrad1", "conv16", "rdX", T["rdX"], eX, SX, half_ulp=True)
            return None
        first = (eX, contraction_bound(eX, SX))
        if k.stride == 2:                                    # the previous stage's output is also a skip
            second = (np.asarray(self.skip_grad(k.level - 1), np.float64), 0.0)
        else:
            second = (np.asarray(dz, np.float64), 0.0 if dz_bound is None else dz_bound)
        return self.masked_sum([first, second], T["rA.%d" % (b - 1)])

    def same_dz(self, stage, k):
        """dz solved from rdY2.<b> and from rdYd.<b> (both gamma invstd (dz - c1 - xhat c2) of the same dz) must agree."""
        out = []
        for L, yn, dn in ((k.L2, "rY2.%d" % k.b, "rdY2.%d" % k.b), (k.Ld, "rYd.%d" % k.b, "rdYd.%d" % k.b)):
            ch = self.chan(L.i)
            Y, dY = np.asarray(self.T[yn], np.float64), np.asarray(self.T[dn], np.float64)
            gi = self.param(L.gamma).astype(np.float64) * ch["invstd"].astype(np.float64)
            xh = (Y - ch["mean"].astype(np.float64)) * ch["invstd"].astype(np.float64)
            c1, c2 = ch["c1"].astype(np.float64), ch["c2"].astype(np.float64)
            dz = dY / gi + c1 + xh * c2
            # the stored dY: half an ulp of its rounding + k = 4 of its float32 expression, both divided by |gamma invstd|
            tol = (0.5 * ulp_bf16(np.abs(dY) * (1 + 2.0 ** -8)) + K_ELEM * EPS * (np.abs(dY) + np.abs(gi) * (np.abs(dz) + np.abs(c1) + np.abs(xh * c2)))) / np.abs(gi)
            out.append((dz, tol))
        (za, ta), (zb, tb) = out
        r = np.abs(za - zb) / (ta + tb)
        self._add(stage, "composite", "rdYd.%d~rdY2.%d" % (k.b, k.b), float(np.nan_to_num(r, nan=np.inf).max()), 1.0)

    def backward(self):
        T = self.T
        A7 = f32(T["rA.7"])
        aw = windows(A7)
        arg = aw.argmax(-1)                                        # the FIRST maximum in row-major window order (strict `>`)
        top = np.take_along_axis(aw, arg[..., None], -1)
        self.tie_windows += int(((aw == top).sum(-1) > 1).sum())
        merged = rne(f32(self.skip_grad(DEPTH)) + route(f32(T["rdpool"]), arg))
        dz, bound = np.where(A7 > 0, merged, np.float32(0)), None
        carried = None
        for k in reversed(self.blocks):
            if k.b == 0:                                           # block 0's dz is stored: the composite oracle against the tensor
                self.close("block0.dz(composite)", "conv16", "rdz.0", T["rdz.0"], dz, Sdz, half_ulp=True, extra=carried, k=K_ELEM)
                dz, bound = T["rdz.0"], None
            nxt = self.block_backward(k, dz, bound)
            if nxt:
                dz, bound, Sdz, carried = nxt
        g = rne(f32(T["rdX"]) + f32(T["rdz.0"]))
        self.exact("stem.relu_mask_sum16", "rdz.1", T["rdz.1"], g)
        self.bn_backward_layer("stem.bn", STEM, T["rdz.1"], "stemY", T["xin"], "dY0")

    def run(self):
        self.forward()
        self.backward()
        self.padding()
        return self


def check(case, state, T):
    return Checker(case, state, T).run()


def stage_table(c):
    """One row per launch of forward_resnet_planes / backward_resnet_planes: (launch, stored inputs, outputs, kind).  Outputs in
    parentheses are scratch a later launch overwrites (unreachable; checked through the composite rows that name them)."""
    rows = [("act_split", ["x"], ["xin"], "direct"),
            ("pconv+stats stem", ["xin"], ["stemY", "chan.0"], "direct"), ("act_split stem", ["stemY", "chan.0"], ["a0"], "direct")]
    bl = blocks(c)
    for k in bl:
        b = k.b
        rows.append(("pconv(s%d)+stats block%d.conv1" % (k.stride, b), [k.a_in], ["rY1.%d" % b, "chan.%d" % k.c1], "direct"))
        if k.Ld:
            rows.append(("pconv(1x1 s2)+stats block%d.proj" % b, [k.a_in], ["rYd.%d" % b, "chan.%d" % k.cd], "direct"))
        rows.append(("act_split block%d" % b, ["rY1.%d" % b, "chan.%d" % k.c1], ["rA1.%d" % b], "direct"))
        rows.append(("pconv+stats block%d.conv2" % b, ["rA1.%d" % b], ["rY2.%d" % b, "chan.%d" % k.c2], "direct"))
        rows.append(("bn_add_relu16 block%d" % b, ["rY2.%d" % b, "rYd.%d" % b if k.Ld else k.a_in], ["rA.%d" % b], "direct"))
    rows.append(("bn_relu_pool_planes", ["rA.7"], ["rskip", "rpool"], "direct"))
    rows.append(("bottleneck, decoders, head, loss, their backward", ["rpool", "rA.1", "rA.3", "rA.5", "rskip"],
                 ["rdpool"] + ["dconcat.%d" % l for l in range(1, DEPTH + 1)], "tests/unet_bf16_stages.py"))
    rows.append(("pool_bwd_merge", ["rA.7", "rdpool", "dconcat.4"], ["(rdX)"], "unreachable: through rdY2.7 (bound 0)"))
    for k in reversed(bl):
        b = k.b
        src = ["(rdX)"] + (["(rdz)"] if b % 2 == 0 and b < 7 else []) + (["dconcat.%d" % k.level] if b % 2 == 1 and b < 7 else [])
        kind = "direct" if b == 0 else "composite"
        rows.append(("relu_mask_sum16 block%d" % b, src + ["rA.%d" % b], ["rdz.0" if b == 0 else "(rdz)"], "composite"))
        rows.append(("bn_bwd_reduce + bn_bwd_apply block%d.bn2" % b, ["(rdz)" if b else "rdz.0", "rY2.%d" % b], ["rdY2.%d" % b, "chan.%d" % k.c2], kind))
        rows.append(("pwgrad block%d.conv2" % b, ["rdY2.%d" % b, "rA1.%d" % b], ["grad conv2.weight"], "direct"))
        rows.append(("pconv(dgrad, bn1 sums) block%d.conv2" % b, ["rdY2.%d" % b, "rY1.%d" % b], ["rdA1" if b == 0 else "(rdA1)", "chan.%d" % k.c1], kind))
        rows.append(("bn_bwd_apply block%d.bn1" % b, ["rdA1" if b == 0 else "(rdA1)", "rY1.%d" % b], ["rdY1.%d" % b], kind))
        rows.append(("pwgrad(s%d) block%d.conv1" % (k.stride, b), ["rdY1.%d" % b, k.a_in], ["grad conv1.weight"], "direct"))
        if k.Ld:
            rows.append(("bn_bwd_reduce + bn_bwd_apply block%d.proj" % b, ["(rdz)", "rYd.%d" % b], ["rdYd.%d" % b, "chan.%d" % k.cd], "composite"))
            rows.append(("pwgrad(1x1 s2) block%d.proj" % b, ["rdYd.%d" % b, k.a_in], ["grad downsample.0.weight"], "direct"))
            for cl in range(4):
                rows.append(("pconv(2x2, class %d, ooy %d oox %d) block%d" % (cl, cl >> 1, cl & 1, b),
                             ["rdY1.%d" % b] + (["rdYd.%d" % b] if cl == 0 else []), ["(rdX)"], "unreachable: through rdY2.%d" % (b - 1)))
        else:
            rows.append(("pconv(dgrad) block%d.conv1" % b, ["rdY1.%d" % b], ["rdX" if b == 0 else "(rdX)"],
                         "direct" if b == 0 else "unreachable: through rdY2.%d" % (b - 1)))
    rows.append(("relu_mask_sum16 stem", ["rdX", "rdz.0"], ["rdz.1"], "direct"))
    rows.append(("bn_bwd_reduce + bn_bwd_apply stem", ["rdz.1", "stemY"], ["dY0", "chan.0"], "direct"))
    rows.append(("pwgrad stem", ["dY0", "xin"], ["grad stem.0.weight"], "direct"))
    return rows


# ------------------------------------------------------------------------------------------------------------ device reader
def read_device(m, c, x, n=None, h=None, w=None, pad_fwd=None):
    """Every tensor of the table from a model that has just run forward_backward(x, y)."""
    T = {"x": np.asarray(x, np.float32)}
    for name in tensor_names(c) + ["dconcat.%d" % l for l in range(1, DEPTH + 1)]:
        T[name] = m.debug_tensor(name).reshape(shape_of(c, name, n, h, w))
    T["chan"] = []
    for i in range(N_ENC_CONVS):
        v = m.debug_tensor("chan.%d" % i)
        T["chan"].append(split_chan(v, v.size // 8))
    T["grad"] = {}
    for L in [STEM] + [L for k in blocks(c) for L in k.layers()]:
        for name in (L.w, L.gamma, L.beta):
            T["grad"][name] = m.grad(name)
    T["pad_bwd"] = OrderedDict(xin=m.debug_tensor("xin:pad"))
    if pad_fwd is not None:
        T["pad_fwd"] = OrderedDict(xin=pad_fwd)
    return T


# ------------------------------------------------------------------------------------------------------------ the CPU stand-in
class StandIn(S.StandIn):
    """A plain float32 emulation of the flow with the library's rounding points: the encoder of this module around the U-Net
    stand-in's bottleneck / decoder / head (shared code on the device too).  ``mutate`` hooks: see the host test."""

    def __init__(self, case, state, x, y, mutate=None):
        super().__init__(case, state, x, y, mutate)
        self.blocks = blocks(case)
        self.I = {}                                   # the scratch of every block (dz.<b>, dA1.<b>, dX.<b>): what the device overwrites

    def n_convs(self):
        return N_ENC_CONVS + 2 + 2 * DEPTH

    def ci(self, block, which):
        return N_ENC_CONVS + S.conv_index(self.c, block, which) - 2 * DEPTH

    def cp(self, i):
        return S.conv_prefix(self.c, i - N_ENC_CONVS + 2 * DEPTH)

    def record_pads(self, when, forward_only=False):
        v = np.zeros((self.c.n * self.c.h * self.c.w, 16 - self.c.in_ch), np.float32)
        self.T[when]["xin"] = self.hook("pad:%s:xin" % when, v)

    def conv_layer(self, L, x_name, out_name):
        T = self.T
        p = L.pad
        pads = self.hook("halo:" + out_name, (p, p, p, p))           # (left, right, top, bottom)
        xt = F.pad(self._t32(T[x_name]), pads)
        acc = self._n32(F.conv2d(xt, self._wb(L.w), stride=L.stride))
        Y = self.hook("out:" + out_name, self.store16(out_name, acc))
        T[out_name] = Y
        mean, invstd, _ = stats_stage(self.hook("stats_source:" + out_name, Y, acc=acc))
        mean, invstd = mean.astype(np.float32), invstd.astype(np.float32)
        sc, sh = bn_coeffs32(self.st[L.gamma], self.st[L.beta], mean, invstd)
        C = Y.shape[-1]
        T["chan"][L.i] = {"running_mean": np.zeros(C, np.float32), "running_var": np.ones(C, np.float32), "mean": mean, "invstd": invstd,
                          "scale": sc, "shift": sh, "c1": np.zeros(C, np.float32), "c2": np.zeros(C, np.float32)}

    def forward_encoder(self, cur):
        T = self.T
        self.conv_layer(STEM, cur, "stemY")
        self.act("stemY", 0, "a0")
        for k in self.blocks:
            b = k.b
            self.conv_layer(k.L1, k.a_in, "rY1.%d" % b)
            if k.Ld:
                self.conv_layer(k.Ld, k.a_in, "rYd.%d" % b)
            self.act("rY1.%d" % b, k.c1, "rA1.%d" % b)
            self.conv_layer(k.L2, "rA1.%d" % b, "rY2.%d" % b)
            o = bn_add_relu32(T["rY2.%d" % b], T["chan"][k.c2], T["rYd.%d" % b] if k.Ld else T[k.a_in], T["chan"][k.cd] if k.Ld else None)
            T["rA.%d" % b] = self.hook("out:rA.%d" % b, self.store16("rA.%d" % b, o))
            if b & 1:
                T["skip.%d" % k.level] = T["rA.%d" % b]             # (the same tensor on the device)
        T["rskip"] = self.hook("out:rskip", T["rA.7"].copy())
        T["skip.%d" % DEPTH] = T["rskip"]
        T["rpool"] = self.hook("out:rpool", windows(T["rA.7"]).max(-1))
        return "rpool"

    def backward(self):
        self.loss_turnaround()
        self.backward_decoder("rpool")
        self.T["rdpool"] = self.T["dpool.%d" % DEPTH]
        self.backward_encoder()
        self.record_pads("pad_bwd")

    def bn_back(self, L, dA, Y_name, x_name, dY_name, slope, sums_of=None):
        """bn_bwd_reduce (or the folded sums) + bn_bwd_apply + the weight gradient of layer L."""
        T = self.T
        ch, Y = T["chan"][L.i], T[Y_name]
        z = f32(Y) * ch["scale"] + ch["shift"]
        src = f32(dA if sums_of is None else sums_of)
        dz = np.where(z > 0, src, src * np.float32(slope)).astype(np.float64)
        xh = ((f32(Y) - ch["mean"]) * ch["invstd"]).astype(np.float64)
        M = Y.size // Y.shape[-1]
        s1, s2 = dz.sum((0, 1, 2)), (dz * xh).sum((0, 1, 2))
        ch["c1"], ch["c2"] = (s1 / M).astype(np.float32), (s2 / M).astype(np.float32)
        T["grad"][L.beta], T["grad"][L.gamma] = s1.astype(np.float32), s2.astype(np.float32)
        o = bn_apply32(dA, Y, ch, self.st[L.gamma], slope)
        T[dY_name] = self.hook("out:" + dY_name, self.store16(dY_name, o))
        T["grad"][L.w] = torch.nn.grad.conv2d_weight(self._t32(T[x_name]), self.st[L.w].shape, self._t32(T[dY_name]), stride=L.stride,
                                                     padding=L.pad).numpy()

    def conv_input(self, L, dY_name, in_hw):
        dt = self._t32(self.T[dY_name])
        shp = (dt.shape[0], self.st[L.w].shape[1]) + tuple(in_hw)
        return self._n32(torch.nn.grad.conv2d_input(shp, self._wb(L.w), dt, stride=L.stride, padding=L.pad))

    def backward_encoder(self):
        T, I, c = self.T, self.I, self.c
        A7 = T["rA.7"]
        aw = windows(A7)
        arg = self.hook("route", aw.argmax(-1), windows=aw)
        C = c.feat << (DEPTH - 1)
        g0 = self.store16("dX.pool", f32(T["dconcat.%d" % DEPTH][..., C:]) + route(f32(T["rdpool"]), arg))
        g1 = g2 = None
        for k in reversed(self.blocks):
            b = k.b
            terms = self.hook("terms:%d" % b, [t for t in (g0, g1, g2) if t is not None])
            v = f32(terms[0])
            for t in terms[1:]:
                v = v + f32(t)
            dz = self.hook("out:dz.%d" % b, self.store16("dz.%d" % b, np.where(T["rA.%d" % b] > 0, v, np.float32(0))))
            I["dz.%d" % b] = dz
            self.bn_back(k.L2, dz, "rY2.%d" % b, "rA1.%d" % b, "rdY2.%d" % b, 1.0)
            acc = self.conv_input(k.L2, "rdY2.%d" % b, T["rA1.%d" % b].shape[1:3])
            dA1 = self.hook("out:dA1.%d" % b, self.store16("dA1.%d" % b, acc))
            I["dA1.%d" % b] = dA1
            self.bn_back(k.L1, dA1, "rY1.%d" % b, k.a_in, "rdY1.%d" % b, 0.0, sums_of=self.hook("sums_source:dA1.%d" % b, dA1, acc=acc))
            hw = T[k.a_in].shape[1:3]
            acc = self.conv_input(k.L1, "rdY1.%d" % b, hw)
            if k.Ld:
                self.bn_back(k.Ld, dz, "rYd.%d" % b, k.a_in, "rdYd.%d" % b, 1.0)
                # four 2x2 contractions, one per parity class of the input pixel; class 0 (even row, even column) takes the
                # projection as a second K segment of the same float32 accumulator
                acc = self.hook("classes:%d" % b, acc + self.conv_input(k.Ld, "rdYd.%d" % b, hw), main=acc)
            dX = self.hook("out:dX.%d" % b, self.store16("dX.%d" % b, acc))
            I["dX.%d" % b] = dX
            g0, g1, g2 = dX, (dz if k.stride == 1 else None), None
            if k.stride == 2:
                Cs = k.cin
                g2 = T["dconcat.%d" % (k.level - 1)][..., Cs:]
        T["rdz.0"], T["rdA1"], T["rdX"] = I["dz.0"], I["dA1.0"], I["dX.0"]
        T["rdz.1"] = self.hook("out:rdz.1", self.store16("rdz.1", f32(g0) + f32(g1)))
        self.bn_back(STEM, T["rdz.1"], "stemY", "xin", "dY0", 0.0)


def whole_model_notices(case, state, x, y, T, loss):
    """test_gpu_resnet_unet.py::test_bf16_operand_mode_vs_same_arithmetic_oracle's criterion on a tensor dictionary (CPU): -> the
    list of what it would have flagged (empty: it stays green)."""
    from oracle import resnet_unet_ref as rref
    from oracle import unet_ref
    xo, yo = unet_ref.nhwc_to_nchw(x), y.float().unsqueeze(1)
    l32, lg32, g32, _ = rref.loss_and_grads(state, xo, yo)
    with unet_ref.bf16_operands(round_outputs=True):
        lb, lgb, gb, _ = rref.loss_and_grads(state, xo, yo)
    out = []
    if abs(loss - float(lb)) > 3e-3 * abs(float(lb)):
        out.append(("loss", loss, float(lb)))
    want = lgb.permute(0, 2, 3, 1).reshape(-1).numpy()
    w32 = lg32.permute(0, 2, 3, 1).reshape(-1).numpy()
    d_same, d_arith = np.abs(T["logits"].reshape(-1) - want).max(), np.abs(w32 - want).max()
    if d_same > max(0.5 * d_arith, 2e-3 * float(np.abs(want).max())):
        out.append(("logits", d_same, d_arith))
    ratios = []
    for k, g in gb.items():
        if k not in T["grad"] or (k.endswith((".0.bias", ".3.bias")) and "conv" in k):
            continue
        g = g.numpy().ravel()
        nrm = np.linalg.norm(g) + 1e-30
        rel_same = np.linalg.norm(T["grad"][k].ravel() - g) / nrm
        rel_arith = np.linalg.norm(g32[k].numpy().ravel() - g) / nrm
        ratios.append(rel_same / max(rel_arith, 1e-9))
        if rel_same > max(1.1 * rel_arith, 1e-2):
            out.append((k, rel_same, rel_arith))
    if np.median(ratios) > 0.8:
        out.append(("median", float(np.median(ratios)), 0.8))
    return out
