"""The U-Net configuration sweep: one case table and the dispatch gates restated as plain predicates of the layer shapes.
Importable without a GPU: test_unet_cases_host.py pins the table on the CPU, test_gpu_unet_configs.py runs it on the device.

A case is ``(id, in_ch, out_ch, feat, depth, n, h, w, seed, covers)``.  ``seed`` draws the initial state
(``unet_ref.init_state``) and, offset by 1000, the input and the labels (``inputs``).  ``covers`` names the gate values
(``gate_values``) the case exists for; the host test asserts that each is true of the case and that every value of every
gate is hit by some case.

The gates (where they live in rfi_toolbox_amd/csrc, what they select), default float32 (3 x bf16) arithmetic:

  feat % 4          conv_mfma_eligible, wgrad_ws_eligible / wgrad_split_eligible, head_fin_deferred, head_fwd_vec /
                    pool_bwd_merge_vec, deferred bias gradients: MFMA or direct VALU contraction, vector or scalar
                    element kernels (a layer's gate is its own channel count: at feat = 6 the 12- and 24-channel
                    layers are on the matrix cores again)
  % 16, map >= 8x8  conv_ws_eligible, ws_set: the wave-specialised conv / input gradient, or the plain 3 x bf16 kernel
  up-conv % 16/32   gemm_ws_eligible: wave-specialised transposed conv (cin % 16 and cout % 32)
  cin_p 4, cout 32/64   conv_stem_eligible, wgrad_stem_eligible: the K-packed stem kernels (a padded 1-3 channel
                    input or a true 4-channel one)
  in_channels % 4   x_pad / pad_channels_kernel: padded staging, or the caller's tensor read directly
  out_channels > 1  head_fwd_kernel's loop over the output channels (forward only: the training step is defined for 1)
  H != W, ragged    partial tiles in both directions at some level; N (H >> D)(W >> D) small: BatchNorm over 2-4 values

SEEDS.  Every training seed keeps the float32 oracle's gradients within 1e-4 (relative L2 per tensor) of the float64
oracle's: no ReLU input flips side inside the oracle itself.  The MARGIN cases have, in addition, the golden fixtures'
``relu_margin`` property: in the float64 oracle no BatchNorm output lies within 1e-5 of the activation threshold, so
two correct float32 implementations cannot differ by a coin flip and the gradient floor is 5e-5 instead of 2e-2.
Seeds tried and rejected (float32-vs-float64 oracle above 1e-4, or no margin) are not listed;
``python tests/unet_cases.py ID`` prints the two figures for seeds 0..39 of a case.

MEASURED on an MI355X (the UNETCFG lines of test_gpu_unet_configs.py).  dlogit: max |logit - oracle's logit| (for the
shapes_* rows the post-step eval logits); ratio: rel_hip / rel_ref over the gradient tensors, both against float64 (for
bfloat16_regs: distance to the same-arithmetic oracle over that oracle's distance to float32); worst: the tensor of
ratio_max.  A ratio_max above 4 (in2_f6_d3_48x80 4.24, in1_f3_d6 6.96) passes because that tensor's rel_hip is under the
floor of the bound max(4 rel_ref, floor): 5e-5 for the margin cases, 2e-2 otherwise.  The out* cases are forward only.
shapes_*_step1 (1 x 16 x 16, one value per channel at the bottleneck, a shape the reference rejects): the bottleneck's output is relu(beta) with |beta| = 1e-4 after one step, decoder4.up.weight's
gradient has norm 9e-6 / 6e-6, the float32 oracle is within 4.4e-6 / 5.3e-6 of float64 there and the device within 7e-4 /
2e-3 (inside the 2e-2 bound): with a single value, x - mean is a rounding residue that 1 / sqrt(eps) = 316 amplifies next
to so small a beta.

  case                      mode            dlogit    ratio_max  ratio_med  worst tensor
  default_in1_f32_d4        float32         4.53e-06       1.87       1.32  decoder1.up.bias
  default_in1_f32_d4        float32_mfma    2.38e-06       1.86       1.33  decoder1.conv.conv.4.bias
  default_in1_f32_d4        float32_planes  2.80e-06       1.84       1.42  decoder1.up.bias
  in4_f32_d1                float32         1.37e-06       2.14       1.33  encoder1.conv.conv.4.bias
  in4_f32_d1                float32_mfma    1.25e-06       2.32       1.46  encoder1.conv.conv.1.bias
  in4_f32_d1                float32_planes  1.10e-06       2.46       1.32  encoder1.conv.conv.4.bias
  in3_f64_d1                float32         2.21e-06       3.21       1.78  encoder1.conv.conv.4.bias
  in3_f64_d1                float32_mfma    1.87e-06       2.32       1.83  bottleneck.conv.1.bias
  in3_f64_d1                float32_planes  2.15e-06       3.15       1.80  encoder1.conv.conv.4.bias
  in2_f6_d3_48x80           float32         1.49e-06       3.74       1.14  encoder1.conv.conv.1.bias
  in2_f6_d3_48x80           float32_mfma    1.25e-06       4.24       1.12  encoder1.conv.conv.1.bias
  in2_f6_d3_48x80           float32_planes  1.49e-06       4.16       1.28  decoder1.up.bias
  in5_f12_d2_40x24          float32         1.85e-06       2.21       1.17  decoder2.up.bias
  in5_f12_d2_40x24          float32_mfma    1.43e-06       1.88       1.09  encoder2.conv.conv.4.weight
  in5_f12_d2_40x24          float32_planes  1.61e-06       1.88       1.17  bottleneck.conv.4.bias
  in16_f20_d2_36x28         float32         1.96e-06       3.32       1.25  encoder1.conv.conv.4.bias
  in16_f20_d2_36x28         float32_mfma    2.24e-06       3.00       1.23  final_conv.bias
  in16_f20_d2_36x28         float32_planes  2.08e-06       3.21       1.29  encoder1.conv.conv.4.bias
  in3_f48_d2_40x24          float32         2.19e-06       3.61       1.90  decoder1.conv.conv.4.bias
  in3_f48_d2_40x24          float32_mfma    2.44e-06       3.47       1.78  decoder1.conv.conv.4.bias
  in3_f48_d2_40x24          float32_planes  2.03e-06       3.07       1.88  encoder2.conv.conv.4.bias
  in1_f3_d6                 float32         2.50e-06       2.80       1.07  encoder1.conv.conv.4.weight
  in1_f3_d6                 float32_mfma    2.44e-06       2.90       1.11  decoder1.conv.conv.1.weight
  in1_f3_d6                 float32_planes  2.50e-06       6.96       1.23  decoder2.conv.conv.1.bias
  in8_f16_d3_16x16          float32         1.90e-06       1.44       1.12  encoder3.conv.conv.1.bias
  in8_f16_d3_16x16          float32_mfma    1.42e-06       1.79       1.18  decoder3.up.bias
  in8_f16_d3_16x16          float32_planes  1.77e-06       1.26       1.05  bottleneck.conv.1.weight
  in3_f5_d1_b5              float32         8.30e-07       2.11       1.09  decoder1.conv.conv.4.bias
  in3_f5_d1_b5              float32_mfma    3.87e-07       2.02       1.00  bottleneck.conv.4.bias
  in3_f5_d1_b5              float32_planes  8.64e-07       2.67       1.09  decoder1.conv.conv.4.bias
  in3_f24_d2_2x8x16         float32         1.31e-06       1.87       1.37  encoder1.conv.conv.1.weight
  in3_f24_d2_2x8x16         float32_mfma    1.13e-06       1.90       1.45  decoder1.conv.conv.1.weight
  in3_f24_d2_2x8x16         float32_planes  1.19e-06       1.67       1.41  encoder1.conv.conv.1.weight
  default_in1_f32_d4        bfloat16_regs   6.25e-03       1.02       0.55  decoder1.conv.conv.1.weight
  in4_f32_d1                bfloat16_regs   1.61e-06       0.02       0.00  bottleneck.conv.0.weight
  in3_f64_d1                bfloat16_regs   1.05e-03       0.25       0.12  decoder1.conv.conv.4.bias
  in2_f6_d3_48x80           bfloat16_regs   6.06e-04       0.03       0.01  decoder3.up.bias
  in5_f12_d2_40x24          bfloat16_regs   1.93e-05       0.03       0.01  encoder1.conv.conv.1.bias
  in16_f20_d2_36x28         bfloat16_regs   5.42e-03       0.58       0.35  decoder1.up.bias
  in3_f48_d2_40x24          bfloat16_regs   5.22e-03       0.81       0.50  decoder1.conv.conv.4.bias
  in1_f3_d6                 bfloat16_regs   1.41e-02       0.98       0.34  decoder1.conv.conv.1.bias
  in8_f16_d3_16x16          bfloat16_regs   6.10e-03       1.22       0.62  final_conv.bias
  in3_f5_d1_b5              bfloat16_regs   1.19e-07       0.00       0.00  final_conv.bias
  in3_f24_d2_2x8x16         bfloat16_regs   2.38e-07       0.03       0.02  encoder1.conv.conv.1.weight
  out2_f6_d2                float32         1.91e-06          -          -  forward-only
  out2_f6_d2                float32_mfma    1.25e-06          -          -  forward-only
  out2_f6_d2                float32_planes  1.49e-06          -          -  forward-only
  out3_f12_d1               float32         1.37e-06          -          -  forward-only
  out3_f12_d1               float32_mfma    7.15e-07          -          -  forward-only
  out3_f12_d1               float32_planes  1.34e-06          -          -  forward-only
  out8_f32_d1               float32         1.61e-06          -          -  forward-only
  out8_f32_d1               float32_mfma    1.37e-06          -          -  forward-only
  out8_f32_d1               float32_planes  1.31e-06          -          -  forward-only
  out12_f5_d2               float32         1.55e-06          -          -  forward-only
  out12_f5_d2               float32_mfma    1.30e-06          -          -  forward-only
  out12_f5_d2               float32_planes  1.91e-06          -          -  forward-only
  shapes_f16_step0_2x64x64  float32         5.96e-07       3.13       1.28  encoder1.conv.conv.4.bias
  shapes_f16_step1_1x16x16  float32         1.49e-07     161.07       1.54  decoder4.up.weight
  shapes_f16_step2_3x32x80  float32         2.09e-07       2.95       1.16  encoder1.conv.conv.4.bias
  shapes_f16_step3_2x64x64  float32         7.15e-07       3.01       1.22  encoder1.conv.conv.4.bias
  shapes_f16_step4_5x16x48  float32         4.77e-07       2.40       1.22  encoder1.conv.conv.4.bias
  shapes_f6_step0_2x64x64   float32         4.17e-07       2.54       1.06  decoder1.conv.conv.1.bias
  shapes_f6_step1_1x16x16   float32         8.94e-08     378.08       1.41  decoder4.up.weight
  shapes_f6_step2_3x32x80   float32         2.09e-07       2.89       1.04  encoder1.conv.conv.4.weight
  shapes_f6_step3_2x64x64   float32         2.09e-07       3.06       1.08  decoder1.conv.conv.4.bias
  shapes_f6_step4_5x16x48   float32         1.79e-07       2.49       1.06  final_conv.bias

MUTATIONS (deliberately wrong builds, never committed, run through test_training_case_float32 in the float32 mode on an
MI355X).  wgrad_stem zeroing the fourth input channel of its staged halo tile (cin_p == 4 treated as three channels):
in4_f32_d1 alone turns red, encoder1.conv.conv.0.weight at rel_hip 0.53 against rel_ref 4.4e-7; the padded-stem cases
default_in1_f32_d4 and in3_f64_d1 rightly stay green.  conv_ws not storing the last pixel column of a partial tile column
(W % TW != 0): the seven cases whose conv_ws maps have such a width turn red (default_in1_f32_d4, in4_f32_d1, in3_f64_d1,
in2_f6_d3_48x80, in5_f12_d2_40x24, in16_f20_d2_36x28, in3_f48_d2_40x24; the eval-mode logits off by 8e-3 to 4e-2 against
2e-5 in five of them, the loss and a pre-BatchNorm bias gradient in the other two), the four with widths 128, 16, 12 and 16 stay green.
"""
from collections import OrderedDict, namedtuple

Case = namedtuple("Case", "id in_ch out_ch feat depth n h w seed covers")

# ---------------------------------------------------------------------------------------------------------- the cases
TRAIN_CASES = [
    # the bare UNet() default: one input channel padded to four, 32 features -> the stem kernels; levels 4 and 5 under 8 x 8
    Case("default_in1_f32_d4", 1, 1, 32, 4, 1, 32, 48, 0,
         ("stem:padded", "in_pad:yes", "conv_ws:taken", "conv_ws:small_map", "gemm_ws:taken", "feat4:yes")),
    # a true 4-channel input: read in place, and still the stem kernels
    Case("in4_f32_d1", 4, 1, 32, 1, 1, 16, 24, 0, ("stem:true4", "in_pad:no", "gemm_ws:taken", "depth:1")),
    Case("in3_f64_d1", 3, 1, 64, 1, 1, 16, 24, 6, ("stem:padded", "conv_ws:taken", "gemm_ws:taken", "depth:1")),
    # feat = 6: channel counts 6, 12, 24, 48 -- the 6-channel layers run the direct kernels and the scalar element kernels
    Case("in2_f6_d3_48x80", 2, 1, 6, 3, 1, 48, 80, 28,
         ("feat4:no", "in_pad:yes", "ragged:yes", "stem:no", "conv_ws:small_map", "gemm_ws:no", "depth:3")),
    Case("in5_f12_d2_40x24", 5, 1, 12, 2, 1, 40, 24, 10, ("feat4:yes", "in_pad:yes", "gemm_ws:no", "ragged:yes", "depth:2")),
    # a 16-channel input: the FIRST conv on the wave-specialised kernel; feat = 20: every later layer declines it
    Case("in16_f20_d2_36x28", 16, 1, 20, 2, 1, 36, 28, 35, ("in_pad:no", "conv_ws:taken", "gemm_ws:no", "ragged:yes", "depth:2")),
    # feat = 48: conv_ws on ragged maps; the up-conv 96 -> 48 declines gemm_ws (cout % 32), 192 -> 96 takes it
    Case("in3_f48_d2_40x24", 3, 1, 48, 2, 2, 40, 24, 0, ("conv_ws:taken", "gemm_ws:taken", "gemm_ws:no", "ragged:yes", "stem:no")),
    # depth 6 at feat = 3: 3 .. 192 channels, maps down to 1 x 2, four values per channel at the bottleneck
    Case("in1_f3_d6", 1, 1, 3, 6, 2, 64, 128, 14, ("feat4:no", "depth:6", "conv_ws:small_map", "small_bn:yes")),
    # 16 features on 16 x 16: conv_ws at levels 1-2, declined at 4 x 4 and 2 x 2 (temporary split filters there)
    Case("in8_f16_d3_16x16", 8, 1, 16, 3, 3, 16, 16, 17,
         ("conv_ws:taken", "conv_ws:small_map", "gemm_ws:taken", "in_pad:no", "small_bn:no", "ragged:no", "depth:3", "batch:3")),
    Case("in3_f5_d1_b5", 3, 1, 5, 1, 5, 8, 12, 0, ("feat4:no", "conv_ws:none", "depth:1", "batch:5")),
    Case("in3_f24_d2_2x8x16", 3, 1, 24, 2, 2, 8, 16, 0, ("feat4:yes", "conv_ws:small_map", "gemm_ws:no")),
]

# out_channels > 1: forward only
FORWARD_CASES = [
    Case("out2_f6_d2", 3, 2, 6, 2, 1, 16, 24, 0, ("out_multi:yes", "feat4:no")),
    Case("out3_f12_d1", 2, 3, 12, 1, 3, 8, 12, 0, ("out_multi:yes", "feat4:yes")),
    Case("out8_f32_d1", 4, 8, 32, 1, 1, 16, 16, 0, ("out_multi:yes", "stem:true4")),
    Case("out12_f5_d2", 1, 12, 5, 2, 2, 12, 20, 0, ("out_multi:yes", "feat4:no")),
]

CASES = TRAIN_CASES + FORWARD_CASES
BY_ID = OrderedDict((c.id, c) for c in CASES)

# the cases whose seed has the relu_margin property (>= 6, one per row of the gate table that a training case can reach)
MARGIN_IDS = ("in4_f32_d1", "in3_f64_d1", "in2_f6_d3_48x80", "in5_f12_d2_40x24", "in16_f20_d2_36x28",
              "in8_f16_d3_16x16", "in3_f5_d1_b5")

# one model through several shapes (test_one_model_several_shapes): UNet(3, 1, f) from shape_state(f), one train_step per
# shape; the data seed of each step was searched along the float32 oracle's own trajectory so that the oracle stays within
# 2e-5 of float64 at that step and no BatchNorm output of the float64 oracle lies within 5e-6 (f = 16, a million
# pre-activations) or 8e-6 (f = 6) of the threshold; the host test asserts ORACLE_REL and 2e-6, which leaves the margin
# ten times the few 1e-7 by which the trajectory moves with the summation order of the CPU run.
# 1 x 16 x 16 at depth 4 leaves ONE value per channel at the bottleneck.  The reference's BatchNorm raises on that shape in
# training, so this step claims no parity with it: it is there for the workspace that shrinks and grows again.  Its
# BatchNorm output is exactly beta on every implementation, and that layer is left out of the margin there.
SHAPES = ((2, 64, 64), (1, 16, 16), (3, 32, 80), (2, 64, 64), (5, 16, 48))
SHAPE_SEEDS = {16: (147, 0, 9, 1, 6), 6: (11, 2, 0, 32, 3)}


def shape_state(f):
    """the state the several-shapes run starts from (the oracle's initialiser: no device library needed to draw it)"""
    from oracle import unet_ref
    return unet_ref.init_state(3, 1, f, 4, seed=100 + f)


def shape_inputs(seed, n, h, w):
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, 3, generator=g)
    y = (torch.rand(n, h, w, generator=g) > 0.8).to(torch.uint8)
    y[:, :, 2:4] = 1
    return x, y


RELU_MARGIN = 1e-5            # the golden fixtures' bound (tests/golden/make_golden.py)
ORACLE_REL = 1e-4             # float32 oracle vs float64 oracle, relative L2 per gradient tensor


def is_prebn_bias(k):
    """conv bias in front of a BatchNorm: its exact gradient is 0"""
    return "conv" in k and k.endswith((".0.bias", ".3.bias"))


def inputs(case):
    """(x NHWC float32, y uint8) of a case"""
    import torch
    g = torch.Generator().manual_seed(case.seed + 1000)
    x = torch.randn(case.n, case.h, case.w, case.in_ch, generator=g)
    y = (torch.rand(case.n, case.h, case.w, generator=g) > 0.8).to(torch.uint8)
    y[:, :, 2:4] = 1
    return x, y


# ------------------------------------------------------------------------------------------------- the gates, restated
def align4(v):
    return (v + 3) // 4 * 4


def conv_layers(case):
    """The 3x3 conv layers in forward order: dicts of name, cin, cin_p (the first layer's input is padded to a multiple of
    4 channels), pstride of the input tensor, cout, h, w, first."""
    f, D = case.feat, case.depth
    out = []

    def add(name, cin, cout, lvl, first=False):
        cin_p = align4(cin) if first else cin
        out.append(dict(name=name, cin=cin, cin_p=cin_p, pstride=cin_p, cout=cout, h=case.h >> (lvl - 1), w=case.w >> (lvl - 1), first=first))
    cin = case.in_ch
    for l in range(1, D + 1):
        c = f << (l - 1)
        add(f"encoder{l}.conv.conv.0", cin, c, l, first=l == 1)
        add(f"encoder{l}.conv.conv.3", c, c, l)
        cin = c
    add("bottleneck.conv.0", cin, 2 * cin, D + 1)
    add("bottleneck.conv.3", 2 * cin, 2 * cin, D + 1)
    for l in range(D, 0, -1):
        c = f << (l - 1)
        add(f"decoder{l}.conv.conv.0", 2 * c, c, l)          # reads the [up | skip] buffer: 2 c channels, pixel stride 2 c
        add(f"decoder{l}.conv.conv.3", c, c, l)
    return out


def up_layers(case):
    """The transposed convs in forward order: name, cin, cout, h, w of the INPUT map."""
    f, D = case.feat, case.depth
    return [dict(name=f"decoder{l}.up", cin=2 * (f << (l - 1)), cout=f << (l - 1), h=case.h >> l, w=case.w >> l) for l in range(D, 0, -1)]


def stem_eligible(L):                 # conv_stem_eligible / wgrad_stem_eligible
    return L["first"] and L["cin_p"] == 4 and L["pstride"] == 4 and L["cout"] in (32, 64)


def ws_map_ok(h, w):                  # conv_ws_eligible: maps of at least 8 x 8
    return h >= 8 and w >= 8


def conv_fwd_path(L):
    """kernel of a 3x3 forward conv in the default arithmetic: choose_conv's order of preference (csrc/dispatch.cpp)"""
    if stem_eligible(L):
        return "conv_stem"
    if L["cin_p"] % 16 == 0 and ws_map_ok(L["h"], L["w"]):
        return "conv_ws"
    if L["cin_p"] % 4 == 0:           # conv_mfma_eligible (pixel stride == channels in every tensor of the U-Net)
        return "conv_mfma"
    return "direct"


def conv_dgrad_path(L):
    """... of its input gradient: a conv whose input channels are the layer's cout (none for the first layer)"""
    if L["first"]:
        return None
    if L["cout"] % 16 == 0 and ws_map_ok(L["h"], L["w"]):
        return "conv_ws"
    return "conv_mfma" if L["cout"] % 4 == 0 else "direct"


def conv_wgrad_path(L):
    """... of its weight gradient (choose_wgrad).  The stem kernel also asks for a slab workspace of 64 x 9 x 4 x cout
    floats; prepare_shape sizes the workspace by the largest split plan over all layers, which exceeds that for every
    case here (the second conv of level 1 alone: min(512, tiles) x 9 x 32 x 32)."""
    if stem_eligible(L):
        return "wgrad_stem"
    return "wgrad_ws" if L["cin_p"] % 4 == 0 and L["cout"] % 4 == 0 else "direct"


def up_ws(U):                         # refresh_ws_weights' up_ok + gemm_ws_eligible
    return U["cin"] % 16 == 0 and U["cout"] % 32 == 0


def up_fwd_path(U):
    if up_ws(U):
        return "gemm_ws"
    return "conv_mfma" if U["cin"] % 4 == 0 else "direct"


def up_dgrad_path(U):                 # reads the up half of the [up | skip] gradient: cout channels
    if up_ws(U):
        return "gemm_ws"
    return "conv_mfma" if U["cout"] % 4 == 0 else "direct"


def up_wgrad_path(U):
    return "wgrad_ws" if U["cout"] % 4 == 0 and U["cin"] % 4 == 0 else "direct"


def predicted_launches(case):
    """{kernel: launches} of one forward + backward pass in the default arithmetic: what the context profile must show.
    "direct" counts the convs AND the weight gradients of the VALU family."""
    n = {}

    def hit(k):
        if k:
            n[k] = n.get(k, 0) + 1
    for L in conv_layers(case):
        hit(conv_fwd_path(L)); hit(conv_dgrad_path(L)); hit(conv_wgrad_path(L))
    for U in up_layers(case):
        hit(up_fwd_path(U)); hit(up_dgrad_path(U)); hit(up_wgrad_path(U))
    return n


def ws_tile(w):                       # the tile family of conv_ws by map width: 8 x 32, 16 x 16, 8 x 8
    return (8, 32) if w >= 32 else (16, 16) if w >= 16 else (8, 8)


def gate_values(case):
    """the set of gate values that are true of a case"""
    v = set()
    convs, ups = conv_layers(case), up_layers(case)
    v.add("feat4:yes" if case.feat % 4 == 0 else "feat4:no")
    fwd = [conv_fwd_path(L) for L in convs]
    dg = [conv_dgrad_path(L) for L in convs]
    if "conv_ws" in fwd or "conv_ws" in dg:
        v.add("conv_ws:taken")
    if any((L["cin_p"] % 16 == 0 or L["cout"] % 16 == 0) and not ws_map_ok(L["h"], L["w"]) for L in convs):
        v.add("conv_ws:small_map")            # channels would do, the map is under 8 x 8
    if not any(L["cin_p"] % 16 == 0 or L["cout"] % 16 == 0 for L in convs):
        v.add("conv_ws:none")
    for U in ups:
        v.add("gemm_ws:taken" if up_ws(U) else "gemm_ws:no")
    if stem_eligible(convs[0]):
        v.add("stem:true4" if case.in_ch == 4 else "stem:padded")
    else:
        v.add("stem:no")
    v.add("in_pad:no" if case.in_ch % 4 == 0 else "in_pad:yes")
    v.add("out_multi:yes" if case.out_ch > 1 else "out_multi:no")
    ragged = False
    for l in range(1, case.depth + 2):
        h, w = case.h >> (l - 1), case.w >> (l - 1)
        th, tw = ws_tile(w)
        ragged |= h != w and h % th != 0 and w % tw != 0
    v.add("ragged:yes" if ragged else "ragged:no")
    v.add("small_bn:yes" if bottleneck_values(case) <= 4 else "small_bn:no")
    v.add(f"depth:{case.depth}")
    v.add(f"batch:{case.n}")
    return v


def bottleneck_values(case):
    return case.n * (case.h >> case.depth) * (case.w >> case.depth)


# every value a gate can take: each must be hit by at least one case
ALL_GATE_VALUES = ("feat4:yes", "feat4:no", "conv_ws:taken", "conv_ws:small_map", "conv_ws:none", "gemm_ws:taken", "gemm_ws:no",
                   "stem:padded", "stem:true4", "stem:no", "in_pad:yes", "in_pad:no", "out_multi:yes", "out_multi:no",
                   "ragged:yes", "ragged:no", "small_bn:yes", "small_bn:no",
                   "depth:1", "depth:2", "depth:3", "depth:6", "batch:1", "batch:3", "batch:5")


# ------------------------------------------------------------------------------------------------- the oracle's own figures
def to64(state):
    return OrderedDict((k, v.double() if v.dtype.is_floating_point else v.clone()) for k, v in state.items())


def oracle_figures(case, seed=None):
    """(worst float32-vs-float64 relative L2 over the gradient tensors, its tensor, min |BatchNorm output| in the float64
    oracle, number of pre-activations).  The margin comes from the tape: conv output, batch mean and biased variance."""
    from oracle import unet_ref
    if seed is not None:
        case = case._replace(seed=seed)
    st = unet_ref.init_state(case.in_ch, case.out_ch, case.feat, case.depth, seed=case.seed)
    x, y = inputs(case)
    return state_figures(st, x, y)


def state_figures(st, x, y, skip=()):
    """oracle_figures for a given state and batch; BatchNorm layers whose name starts with one of `skip` are left out of
    the margin"""
    import torch
    from oracle import unet_ref
    xo, yo = unet_ref.nhwc_to_nchw(x), y.float().unsqueeze(1)
    _, _, g32, _ = unet_ref.loss_and_grads(st, xo, yo)
    tape = {}
    st64 = to64(st)
    _, _, g64, _ = unet_ref.loss_and_grads(st64, xo.double(), yo.double(), tape=tape)
    worst, worst_k = 0.0, ""
    for k, w in g64.items():
        if is_prebn_bias(k):
            continue
        rel = float(torch.linalg.norm(g32[k].double() - w) / (torch.linalg.norm(w) + 1e-30))
        if rel > worst:
            worst, worst_k = rel, k
    margin, count = float("inf"), 0
    for k, out in tape.items():
        if not k.endswith(".out") or ".up." in k or any(k.startswith(p) for p in skip):
            continue
        conv = k[:-4]                                     # "<prefix>.<conv_idx>"
        prefix, ci = conv.rsplit(".", 1)
        bn = f"{prefix}.{int(ci) + 1}"
        mean, var = tape[f"{bn}.mean"], tape[f"{bn}.var"]
        z = (out.detach() - mean[None, :, None, None]) * torch.rsqrt(var + unet_ref.BN_EPS)[None, :, None, None]
        z = z * st64[f"{bn}.weight"][None, :, None, None] + st64[f"{bn}.bias"][None, :, None, None]
        margin = min(margin, float(z.abs().min()))
        count += z.numel()
    return worst, worst_k, margin, count


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for cid in sys.argv[1:] or [c.id for c in TRAIN_CASES]:
        for s in range(40):
            rel, k, margin, count = oracle_figures(BY_ID[cid], seed=s)
            print(f"{cid} seed={s} rel32={rel:.2e} ({k}) margin={margin:.2e} preacts={count}", flush=True)
