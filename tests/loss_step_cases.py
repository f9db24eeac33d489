"""The loss turn-around and the optimizer step on their own: case tables and float64 references, NumPy / torch on the CPU
only.  test_loss_step_cases_host.py pins the tables without a GPU, test_gpu_loss_step.py runs them on the device.

A. LOSS AND dlogits.  A case is ``LossCase(id, model, shape, labels, loss, logits)``.  The device test reads the logits the
device itself produced, so the network in front does not matter; it only has to deliver logits in the range the case
claims.  ``SETUPS[(model, shape, logits)] = (seed, k, b)``: the oracle's initial state of that seed with the head's weight
scaled by ``k`` and its bias set to ``b`` (``b is None``: kept).  ``k`` and ``b`` of a saturated setup put the median logit
of the float32 oracle at 0 and the farthest one at +-80 (``python tests/loss_step_cases.py`` prints them).  The references
(``bce_dice_ref``, ``focal_ref``, ``through_sigmoid``) are closed forms in log space, written from the definitions

    softplus(x) = max(x, 0) + log1p(exp(-|x|)),  log p = -softplus(-x),  log(1 - p) = -softplus(x)
    BCE + dice:  mean(softplus(x) - x t) + 1 - (2 I + 1) / D,  I = sum p t,  D = sum p + sum t + 1
                 d/dx_i = (p_i - t_i) / N + p_i (1 - p_i) ((2 I + 1) / D^2 - 2 t_i / D)
    focal:       t = 1:  a1 (1-p)^g softplus(-x),   d/dx = -a1 (1-p)^g (g p softplus(-x) + (1 - p))
                 t = 0:  a0 p^g softplus(x),        d/dx =  a0 p^g (g (1-p) softplus(x) + p)
                 a1 = alpha, a0 = 1 - alpha (alpha < 0: both 1), mean over the elements

and never through autograd: autograd of ``(1 - p_t) ** g`` returns NaN at saturated logits for g < 1 even in float64
(0 * inf), where the true derivative is finite.

B. CLIP + ADAM.  An ``AdamCase`` names the step count, the hyper-parameters and how the crafted gradient is drawn;
``adam_inputs`` draws it per named parameter in the reference layout (the device test scatters it into the flat buffer
through the layout map), ``adam_reference`` runs ``unet_ref.adam_update`` in float64 and in float32 with the clip
coefficient formed as the kernel documents it (float32 norm, ``max / (norm + 1e-6)``, clamped at 1).  An ulp below is the
float32 spacing at the float64 value the error is measured against.

MEASURED by test_loss_step_cases_host.py on the float32 CPU oracle's own logits (the device's differ in the last bits).
coverage = fraction below -20 / fraction above +20 / count in |x| < 1 / max |x|.  dloss: the float32 oracle's loss error in
units of 2^-24 max(1, |loss64|), the largest over the labels and losses of the setup (loss values up to 17).  e_ref: max
|g32 - g64| of the float32 oracle's dlogits in units of 2^-24 max |g64|, the largest over the four label planes.  The 20-28
of focal gamma = 2 and 1.5 at saturated logits are 1 - p cancelling in float32, which the kernel shares with torchvision's
formula.

  model    shape       logits     coverage                 dloss  e_ref: bce_dice  focal_a0.25_g2  focal_a-1_g1.5  focal_a0.6_g0  focal_a-1_g0.5
  cnn      1x5x7       default    0.000/0.000/35/0.6        1.25      3.13            2.83            3.62           4.27            3.01
  cnn      1x5x7       saturated  0.171/0.314/2/80.0        1.44      1.19           25.13           19.01           2.15            2.19
  cnn      1x512x520   saturated  0.124/0.115/12636/95.0    1.35      3.73           27.69               -              -               -
  cnn      1x1024x1040 saturated  0.120/0.111/51286/95.0    1.85      3.87           27.69               -              -               -
  cnn      3x33x47     default    0.000/0.000/4653/0.9      0.75      4.39            5.88            6.38           5.61            4.83
  cnn      3x33x47     saturated  0.142/0.163/200/80.0      1.62      3.31           27.64           20.99           2.31            2.92
  overfit  2x16x16     default    0.000/0.000/479/1.8       0.72      4.42            6.05            5.73           4.75            4.48
  overfit  2x16x16     saturated  0.160/0.129/24/80.0       1.77      6.24            7.45            7.08           6.24            6.45
  unet_d1  2x6x10      default    0.000/0.000/117/1.4       1.96      2.67            2.48            2.28           3.28            2.49
  unet_d1  2x6x10      saturated  0.142/0.192/11/80.0       2.22      1.96           22.78           19.88           2.10            1.89

e32: float32 ``adam_update`` against float64 on the sign-coherent rows, in ulp, and the float32 oracle's norm
(``clip_coefficient``) in units of 2^-24.  The update of the rows that clip by 1e-4 and more moves p by less than half
a spacing of p nearly everywhere; what is left after that half spacing is taken off is 0 there.

  Adam case                                      m     v update  norm (2^-24)
  small_t1_wd0_gs1_off                        0.60  2.12   1.03  0.38
  small_t1_wd1e-05_gs0.5_inactive             1.37  2.75   2.50  0.35
  small_t1_wd0.01_gs0.333_active              1.95  3.11   1.77  0.06
  small_t2_wd0_gs0.5_active                   0.55  0.71   0.66  0.54
  small_t2_wd1e-05_gs0.333_off                1.97  2.19   1.07  0.32
  small_t2_wd0.01_gs1_inactive                1.99  2.19   2.11  0.56
  small_t10_wd0_gs0.333_inactive              0.58  1.14   0.71  0.46
  small_t10_wd1e-05_gs1_active                1.24  1.39   0.00  0.14
  small_t10_wd0.01_gs0.5_off                  1.82  2.28   0.94  0.27
  small_t1000_wd0_gs1_off                     0.55  1.14   0.54  0.83
  small_t1000_wd1e-05_gs0.5_inactive          1.82  2.13   1.08  0.97
  small_t1000_wd0.01_gs0.333_active           1.54  2.07   0.72  0.42
  small_t1000000_wd0_gs0.5_active             0.55  0.71   1.29  0.22
  small_t1000000_wd1e-05_gs0.333_off          1.67  2.32   1.56  0.56
  small_t1000000_wd0.01_gs1_inactive          1.66  2.26   1.76  0.03
  small_t10_wd1e-05_gs0.5_below               0.96  1.96   0.00  0.15
  small_t2_wd0.01_gs1_above                   1.88  2.04   1.45  0.84
  large_t1_wd1e-05_gs1_active                 2.19  4.35   4.47  0.17
  large_t1000_wd0_gs0.5_off                   0.53  1.21   3.45  0.49
  large_t10_wd0.01_gs0.333_inactive           2.16  2.54   3.30  0.26
  largest                                     2.19  4.35   4.47  0.97

ON AN MI355X (the LOSSSTEP / ADAMSTEP / PADDING lines of test_gpu_loss_step.py).  Loss: at most 1.52 x 2^-24 max(1, |loss|)
from float64 over the 164 cases (bound 8).  dlogits: at most 0.70 of the bound max(2 e_ref, 4 x 2^-24 max |g64|), 2.5-4.1
x 2^-24 max |g64| where the bound is near its floor; every element finite.  m and v come out bit-equal to the float32
oracle's on every sign-coherent row (the e32 figures above are the device's too), the update at most 4.5 ulp from
float64 and at most 0.78 of its bound, the norm within 1.6 x 2^-24 (bound 4).  No flat gradient or parameter outside the named entries is ever non-zero: UNet(3,1,8)
75 padding floats, UNet(5,1,12,depth=2) 327, UNetResNet18(3,1,16) 1347, SimpleCNN(3,1,8) 75, in all three modes -- the
padded stem lanes multiply staged zeros, a bias-less conv's slot is never written, so neither sumsq nor adam_kernel needs
an exclusion and nothing is zeroed on the hot path.

FOUND with these cases: focal_bwd formed 1 - p as ``1.0f - p``.  For a background pixel the term gamma (1-p) softplus(x)
then carries an error of gamma x 2^-24 relative to the largest gradient (1 - p is 0 from x = 17 on): the nine saturated
gamma = 0.5 cases with background pixels came out at 4.6, 6.3 and 7.5 x 2^-24 max |g64| against bounds of 4.4, 6.0 and 5.6.
The kernel now takes p and 1 - p from one exp without a subtraction from 1 and forms the products around its three
float32 library calls in double, rounded once; the same cases are at 0.5 of the bound and below.

The sigmoid head runs on ``UNetOverfit`` with one level instead of its five (a subclass in the device test that only sets
the depth): 2 x 16 x 16 is not a multiple of 2^5, and the loss kernels do not see the depth.
"""
import math
from collections import OrderedDict, namedtuple

import numpy as np
import torch

U24 = 2.0 ** -24

# ------------------------------------------------------------------------------------------------------------ A: loss
LossCase = namedtuple("LossCase", "id model shape labels loss logits")

MODELS = {                       # name -> (constructor arguments of the oracle's init_state, head prefix)
    "cnn": ((3, 1, 4), "decoder.0"),             # SimpleCNN(3, 1, 4)
    "unet_d1": ((3, 1, 4, 1), "final_conv"),     # UNet(3, 1, 4, depth=1)
    "overfit": ((1, 1, 4, 1), "final_conv"),     # UNetOverfit's sigmoid head on a one-level, 4-feature U-Net
}
SMALL_SHAPES = (("cnn", (1, 5, 7)), ("cnn", (3, 33, 47)), ("unet_d1", (2, 6, 10)), ("overfit", (2, 16, 16)))
LARGE_SHAPES = (("cnn", (1, 512, 520)), ("cnn", (1, 1024, 1040)))
LABELS = ("random", "zeros", "ones", "single")
LOSSES = (("bce_dice",), ("focal", 0.25, 2.0), ("focal", -1.0, 1.5), ("focal", 0.6, 0.0), ("focal", -1.0, 0.5))
RANGES = ("default", "saturated")

# (model, shape, range) -> (seed, k, b)
SETUPS = {
    ("cnn", (1, 5, 7), "default"): (1, 1.0, None),
    ("cnn", (1, 5, 7), "saturated"): (1, 236.6, -27.666),
    ("cnn", (3, 33, 47), "default"): (4, 1.0, None),
    ("cnn", (3, 33, 47), "saturated"): (4, 265.5, -30.8812),
    ("unet_d1", (2, 6, 10), "default"): (3, 1.0, None),
    ("unet_d1", (2, 6, 10), "saturated"): (3, 65.75, -3.54883),
    ("overfit", (2, 16, 16), "default"): (2, 1.0, None),
    ("overfit", (2, 16, 16), "saturated"): (2, 57.6, 5.40761),
    ("cnn", (1, 512, 520), "saturated"): (3, 165.4, 9.3532),          # (median-centred, these two reach 7-9 % per side:
    ("cnn", (1, 1024, 1040), "saturated"): (3, 163.0, 9.2049),        # centred on the 0.54 quantile, farthest logit at 95)
}


def _loss_tag(loss):
    return "bce_dice" if loss[0] == "bce_dice" else f"focal_a{loss[1]:g}_g{loss[2]:g}"


def _case(model, shape, labels, loss, logits):
    n, h, w = shape
    return LossCase(f"{model}_{n}x{h}x{w}_{logits}_{labels}_{_loss_tag(loss)}", model, shape, labels, loss, logits)


LOSS_CASES = [_case(m, s, lab, loss, r) for m, s in SMALL_SHAPES for r in RANGES for lab in LABELS for loss in LOSSES]
LOSS_CASES += [_case(m, s, "random", loss, "saturated") for m, s in LARGE_SHAPES for loss in LOSSES[:2]]


def head_state(model, shape, logits):
    """the oracle's initial state of the setup, head steered by (k, b)"""
    from oracle import cnn_ref, unet_ref
    seed, k, b = SETUPS[(model, shape, logits)]
    args, head = MODELS[model]
    st = cnn_ref.init_state(*args, seed=seed) if model == "cnn" else unet_ref.init_state(*args, seed=seed)
    st[f"{head}.weight"] = st[f"{head}.weight"] * k
    if b is not None:
        st[f"{head}.bias"] = torch.full_like(st[f"{head}.bias"], b)
    return st


def loss_input(model, shape, logits):
    """x (N, H, W, C) float32 of a setup"""
    n, h, w = shape
    g = torch.Generator().manual_seed(SETUPS[(model, shape, logits)][0] + 1000)
    return torch.randn(n, h, w, MODELS[model][0][0], generator=g)


def labels_of(case):
    """(N, H, W) uint8"""
    n, h, w = case.shape
    if case.labels == "zeros":
        return torch.zeros(n, h, w, dtype=torch.uint8)
    if case.labels == "ones":
        return torch.ones(n, h, w, dtype=torch.uint8)
    if case.labels == "single":
        y = torch.zeros(n * h * w, dtype=torch.uint8)
        y[(n * h * w) // 3] = 1
        return y.reshape(n, h, w)
    g = torch.Generator().manual_seed(7 + n * h * w)
    return (torch.rand(n, h, w, generator=g) < 0.15).to(torch.uint8)


def oracle_logits(model, shape, logits):
    """the float32 CPU oracle's train-mode logits of a setup, flat in NHWC order (for the sigmoid head: z, before the
    sigmoid)"""
    from oracle import cnn_ref, unet_ref
    st = head_state(model, shape, logits)
    x = unet_ref.nhwc_to_nchw(loss_input(model, shape, logits))
    with torch.no_grad():
        out = cnn_ref.forward(st, x) if model == "cnn" else unet_ref.forward(st, x, training=True)
    return out.permute(0, 2, 3, 1).reshape(-1)


def coverage(x):
    """(fraction below -20, fraction above +20, count in |x| < 1, max |x|, all finite)"""
    x = np.asarray(x, dtype=np.float64)
    return float((x < -20).mean()), float((x > 20).mean()), int((np.abs(x) < 1).sum()), float(np.abs(x).max()), bool(np.isfinite(x).all())


# ---- float64 closed forms (torch tensors in, torch tensors out; the dtype of x decides the arithmetic, so the same text
# run on a float32 tensor is "the closed form in float32")
def _softplus(x):
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


def bce_dice_ref(x, t):
    """(loss, d loss / d x) of mean BCE-with-logits + dice(smooth 1) over the flat tensors x, t"""
    sp, sn = _softplus(x), _softplus(-x)
    p, q = torch.exp(-sn), torch.exp(-sp)
    n = x.numel()
    inter, d = (p * t).sum(), p.sum() + t.sum() + 1
    num = 2 * inter + 1
    loss = (sp - x * t).sum() / n + 1 - num / d
    pmt = torch.where(t > 0, -q, p)                           # p - t without cancellation
    return loss, pmt / n + p * q * (num / (d * d) - 2 * t / d)


def focal_ref(x, t, alpha, gamma):
    """(loss, d loss / d x) of the sigmoid focal loss, mean over the elements"""
    sp, sn = _softplus(x), _softplus(-x)                      # -log(1-p), -log p
    p, q = torch.exp(-sn), torch.exp(-sp)
    a1, a0 = (alpha, 1 - alpha) if alpha >= 0 else (1.0, 1.0)
    qg, pg = torch.exp(-gamma * sp), torch.exp(-gamma * sn)   # (1-p)^gamma, p^gamma
    pos = t > 0
    loss = torch.where(pos, a1 * qg * sn, a0 * pg * sp)
    grad = torch.where(pos, -a1 * qg * (gamma * p * sn + q), a0 * pg * (gamma * q * sp + p))
    n = x.numel()
    return loss.sum() / n, grad / n


def loss_ref(loss, x, t):
    return bce_dice_ref(x, t) if loss[0] == "bce_dice" else focal_ref(x, t, loss[1], loss[2])


def through_sigmoid(loss, z, t):
    """UNetOverfit: the loss sees x = sigmoid(z) as its logits; (loss, d loss / d z) with dx/dz = p (1 - p) in log space"""
    sp, sn = _softplus(z), _softplus(-z)
    val, gx = loss_ref(loss, torch.exp(-sn), t)
    return val, gx * torch.exp(-sn - sp)


def reference(case, logits, t, dtype=torch.float64):
    """(loss, dlogits) of a case by the closed forms in `dtype` from the given flat logits and labels"""
    x, t = torch.as_tensor(logits).to(dtype), torch.as_tensor(t).to(dtype)
    return through_sigmoid(case.loss, x, t) if case.model == "overfit" else loss_ref(case.loss, x, t)


def oracle_loss_fn(case):
    from oracle import unet_ref
    if case.loss[0] == "bce_dice":
        return unet_ref.segmentation_loss
    return lambda lg, y: unet_ref.focal_loss(lg, y, case.loss[1], case.loss[2])


def autograd(case, logits, t, dtype):
    """(loss, dlogits) of the CPU oracle's loss text (oracle/unet_ref.py) through autograd in `dtype`"""
    x = torch.as_tensor(logits).to(dtype).clone().requires_grad_(True)
    seen = torch.sigmoid(x) if case.model == "overfit" else x
    loss = oracle_loss_fn(case)(seen, torch.as_tensor(t).to(dtype))
    g, = torch.autograd.grad(loss, x)
    return loss.detach(), g


def oracle32(case, logits, t):
    """the float32 CPU oracle on the given logits: autograd, or the closed form in float32 where autograd is not finite"""
    loss, g = autograd(case, logits, t, torch.float32)
    if not bool(torch.isfinite(g).all()):
        g = reference(case, logits, t, torch.float32)[1]
    return loss, g


def loss_figures(case, logits, t):
    """(loss64, g64, e_ref = max |g32 - g64| of the float32 oracle, its loss error) on the given logits"""
    l64, g64 = reference(case, logits, t)
    l32, g32 = oracle32(case, logits, t)
    e_ref = float((g32.double() - g64).abs().max())
    return float(l64), g64.numpy(), e_ref, abs(float(l32) - float(l64))


def loss_bound(l64):
    return 8 * U24 * max(1.0, abs(l64))


def grad_bound(e_ref, g64):
    return max(2 * e_ref, 4 * U24 * float(np.abs(g64).max()))


# ------------------------------------------------------------------------------------------------------------ B: Adam
AdamCase = namedtuple("AdamCase", "id model t wd gs clip kind")      # clip: "off" | "active" | "inactive" | "below" | "above"
ADAM_MODELS = {"small": (3, 1, 4, 1), "large": (3, 1, 16, 4)}       # UNet(3, 1, 4, depth=1), UNet(3, 1, 16)
STEPS, WDS, SCALES, CLIPS = (1, 2, 10, 1000, 10 ** 6), (0.0, 1e-5, 1e-2), (1.0, 0.5, 1.0 / 3.0), ("off", "active", "inactive")
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8


def _pairwise_rows():
    """15 rows from two orthogonal Latin squares: every pair of values of any two of the four factors occurs"""
    rows = []
    for i in range(15):
        a, b = i // 3, i % 3
        rows.append((STEPS[a], WDS[b], SCALES[(a + b) % 3], CLIPS[(a + 2 * b) % 3]))
    return rows


def _acase(model, t, wd, gs, clip, kind="coherent"):
    return AdamCase(f"{model}_t{t}_wd{wd:g}_gs{gs:.3g}_{clip}" + ("" if kind == "coherent" else "_" + kind), model, t, wd, gs, clip, kind)


ADAM_CASES = [_acase("small", *r) for r in _pairwise_rows()]
ADAM_CASES += [_acase("small", 10, 1e-5, 0.5, "below"), _acase("small", 2, 1e-2, 1.0, "above")]
ADAM_CASES += [_acase("large", 1, 1e-5, 1.0, "active"), _acase("large", 1000, 0.0, 0.5, "off"),
               _acase("large", 10, 1e-2, 1.0 / 3.0, "inactive")]
MIXED_CASE = _acase("small", 10, 1e-2, 0.5, "active", kind="mixed")
NAN_CASES = [_acase("small", 2, 1e-5, 1.0, "active", kind="nan"), _acase("small", 2, 1e-5, 1.0, "off", kind="nan")]
NAN_AT = ("bottleneck.conv.0.weight", 5)        # (entry, flat index in the reference layout) of the NaN gradient
ADAM_BY_ID = OrderedDict((c.id, c) for c in ADAM_CASES + [MIXED_CASE] + NAN_CASES)


def adam_shapes(model):
    """OrderedDict name -> shape of the trainable parameters, reference order"""
    from oracle import unet_ref
    return OrderedDict((n, s) for n, s, kind in unet_ref.unet_entries(*ADAM_MODELS[model]) if kind == "param")


def clip_is_active(case):
    return case.clip in ("active", "below")


def adam_inputs(case):
    """{"g", "p", "m", "v"}: OrderedDicts name -> float32 tensor in the reference layout, and "zero": name -> bool mask of
    the elements with g = p = m0 = v0 = 0.  Sign-coherent: one random sign s per element, g = s 10^U (U uniform over
    [-12, 6], [-6, 3] where the clip is active), every 17th g exactly 0, p = s |N(0, 1)|, and for t > 1 m0 = s |g| U(0.25,
    1.75), v0 = g^2 U(0.25, 1.75) (t = 1: the moments start at 0).  Every 34th element is 0 in all four.  kind "mixed":
    p and m0 signed independently of g.  kind "nan": NAN_AT's gradient is NaN."""
    rng = np.random.default_rng(1000 + sorted(ADAM_BY_ID).index(case.id))
    lo, hi = (-6.0, 3.0) if clip_is_active(case) else (-12.0, 6.0)
    out = {k: OrderedDict() for k in ("g", "p", "m", "v", "zero")}
    count = 0
    for name, shape in adam_shapes(case.model).items():
        n = int(np.prod(shape))
        idx = np.arange(count, count + n)
        count += n
        s = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        g = s * 10.0 ** rng.uniform(lo, hi, n)
        g[idx % 17 == 0] = 0.0
        p = s * np.abs(rng.standard_normal(n))
        um, uv = rng.uniform(0.25, 1.75, n), rng.uniform(0.25, 1.75, n)
        g32 = g.astype(np.float32)
        if case.t > 1:
            m0 = s * np.abs(g32.astype(np.float64)) * um
            v0 = g32.astype(np.float64) ** 2 * uv
        else:
            m0, v0 = np.zeros(n), np.zeros(n)
        if case.kind == "mixed":
            p = p * np.where(rng.random(n) < 0.5, -1.0, 1.0)
            m0 = m0 * np.where(rng.random(n) < 0.5, -1.0, 1.0)
        zero = idx % 34 == 0
        p[zero], m0[zero], v0[zero] = 0.0, 0.0, 0.0
        if case.kind == "nan" and name == NAN_AT[0]:
            g32[NAN_AT[1]] = np.nan
        for key, a in (("g", g32), ("p", p), ("m", m0), ("v", v0)):
            out[key][name] = torch.from_numpy(np.asarray(a, dtype=np.float32).reshape(shape).copy())
        out["zero"][name] = zero.reshape(shape)
    return out


def grad_norm64(inp, gs):
    """sqrt(sum g^2) * grad_scale in float64"""
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in inp["g"].values())) * gs


def max_grad_norm(case, inp):
    n = grad_norm64(inp, float(np.float32(case.gs)))
    return {"off": 0.0, "active": 1.0, "inactive": 2.0 * n, "below": 0.99 * n, "above": 1.01 * n}[case.clip]


def kernel_coef(inp, gs, max_norm):
    """(norm, coef) as float32 scalars, formed as adam_kernel documents: norm = float32(sqrt(sum g^2 in double)) * gs,
    coef = min(max_norm / (norm + 1e-6), 1), 1 where max_norm <= 0"""
    f = np.float32
    total = math.sqrt(sum(float((g.double() ** 2).sum()) for g in inp["g"].values()))
    norm = f(f(total) * f(gs))
    if max_norm <= 0:
        return norm, f(1.0)
    coef = f(max_norm) / f(norm + f(1e-6))
    return norm, (coef if not coef > f(1.0) else f(1.0))      # (a NaN stays a NaN, as in the kernel and in clip_grad_norm_)


def adam_reference(case, inp, dtype, max_norm=None):
    """Run unet_ref.adam_update on the case's inputs in `dtype` from step t - 1.  Returns {"p", "m", "v"} (OrderedDicts of
    tensors in `dtype`), "norm" and "coef" (float32 scalars, kernel_coef)."""
    from oracle import unet_ref
    max_norm = max_grad_norm(case, inp) if max_norm is None else max_norm
    gs32 = np.float32(case.gs)
    norm, coef = kernel_coef(inp, gs32, max_norm)
    scale = torch.tensor(float(gs32), dtype=dtype)
    grads = OrderedDict((k, g.to(dtype) * scale) for k, g in inp["g"].items())
    state = OrderedDict((k, v.to(dtype).clone()) for k, v in inp["p"].items())
    adam = {"step": case.t - 1, "m": OrderedDict((k, v.to(dtype).clone()) for k, v in inp["m"].items()),
            "v": OrderedDict((k, v.to(dtype).clone()) for k, v in inp["v"].items())}
    unet_ref.adam_update(state, adam, grads, torch.tensor(float(coef), dtype=dtype), lr=LR, betas=BETAS, eps=EPS,
                         weight_decay=case.wd)
    assert adam["step"] == case.t
    return {"p": state, "m": adam["m"], "v": adam["v"], "norm": norm, "coef": coef}


def _cat(d):
    return np.concatenate([np.asarray(v, dtype=np.float64).ravel() for v in d.values()])


def _ulps(err, want):
    """|err| in units of the float32 spacing at |want| (want != 0)"""
    return np.abs(err) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)


def ulp_errors(got, want64, p0):
    """(m, v, update) errors of `got` ({"p", "m", "v"}: name -> array-like holding float32 values) against the float64
    result, each the largest over the elements in ulp: the float32 spacing at the float64 value.  m and v: over the
    non-zero elements.  update: |(p' - p) - (p'64 - p)| less half a spacing of p'64 (the rounding of the final sum, which
    no implementation can avoid), in ulp of |p'64 - p|, over the elements that move.  Fourth: the number of elements whose
    float64 value (m, v, update) is 0 but `got`'s is not."""
    p0 = _cat(p0)
    res, stray = [], 0
    for key in ("m", "v"):
        g, w = _cat(got[key]), _cat(want64[key])
        nz = w != 0
        stray += int(np.count_nonzero(g[~nz]))
        res.append(float(_ulps(g[nz] - w[nz], w[nz]).max()) if nz.any() else 0.0)
    g, w = _cat(got["p"]), _cat(want64["p"])
    upd_g, upd_w = g - p0, w - p0
    mv = upd_w != 0
    stray += int(np.count_nonzero(upd_g[~mv]))
    half = 0.5 * np.spacing(np.abs(w[mv]).astype(np.float32)).astype(np.float64)
    err = np.maximum(np.abs(upd_g[mv] - upd_w[mv]) - half, 0.0)
    res.append(float(_ulps(err, upd_w[mv]).max()) if mv.any() else 0.0)
    return res[0], res[1], res[2], stray


def adam_bounds(e32):
    """max(2 e32, 2 ulp) per quantity, in ulp"""
    return tuple(max(2.0 * e, 2.0) for e in e32[:3])


def mixed_bounds(case, inp, ref64):
    """Scale-aware first-order bounds for the mixed-sign row, u = 2^-24, per element (flat arrays |dm|, |dv|, |dp'|).

    With G = |g gs coef| + wd |p| (>= |g'|, g' = fma(wd, p, (g gs) coef): three roundings of g gs coef, the scalars gs and
    wd rounded once each: |dg'| <= 4 u G):
      m = fma(w, g' - m0, m0), w = fl(0.1):   |dm| <= w |dg'| + w u (G + |m0|) [the difference] + w u (G + |m0|) [w]
                                                      + u (G + |m0|) [the fma]  <=  4 u (G + |m0|)
      v = fma(fl(c g'), g', fl(b2 v0)), c = fl(1 - b2), all terms >= 0:
                                               |dv| <= c (2 G |dg'| + 2 u G^2) + 2 u b2 v0 + u v  <=  12 u (c G^2 + b2 v0)
      q = (ns m) / den, den = sqrt(v) / bs + eps:
                                               |dden| <= |dv| / (2 sqrt(v) bs) + 3 u sqrt(v) / bs + u eps + u den
                                               |dq| <= |ns| |dm| / den + |q| (|dden| / den + 3 u)
      p' = p + q:                              |dp'| <= |dq| + half a float32 spacing of p'
    """
    b1, b2 = BETAS
    g = np.abs(_cat(inp["g"])) * float(np.float32(case.gs)) * float(ref64["coef"])
    p0, m0, v0 = _cat(inp["p"]), _cat(inp["m"]), _cat(inp["v"])
    G = g + case.wd * np.abs(p0)
    m, v = _cat(ref64["m"]), _cat(ref64["v"])
    dm = 4 * U24 * (G + np.abs(m0))
    dv = 12 * U24 * ((1 - b2) * G * G + b2 * v0)
    ns = LR / (1 - b1 ** case.t)
    bs = math.sqrt(1 - b2 ** case.t)
    sq = np.sqrt(v)
    den = sq / bs + EPS
    with np.errstate(divide="ignore", invalid="ignore"):
        dden = np.where(v > 0, dv / (2 * sq * bs), 0.0) + 3 * U24 * sq / bs + U24 * EPS + U24 * den
    q = ns * np.abs(m) / den
    dq = ns * dm / den + q * (dden / den + 3 * U24)
    dp = dq + 0.5 * np.spacing(np.abs(_cat(ref64["p"])).astype(np.float32)).astype(np.float64)
    return dm, dv, dp


# ------------------------------------------------------------------------------------------------------------ C: padding
# (model, constructor arguments, keyword arguments, shape of the batch)
PADDING_RUNS = (("UNet", (3, 1, 8), {}, (2, 32, 32)), ("UNet", (5, 1, 12), {"depth": 2}, (2, 48, 80)),
                ("UNetResNet18", (3, 1, 16), {}, (2, 32, 32)), ("SimpleCNN", (3, 1, 8), {}, (2, 32, 32)))
PADDING_MODES = ("float32", "float32_mfma", "bfloat16")


def layout_from_gather(gathered, n_flat):
    """`gathered`: name -> what grad(name) returned after arange(n_flat) was written into the flat gradient buffer.
    Returns (name -> int64 array of flat offsets in the shape of the entry, bool mask of the padding offsets); asserts the
    values are integers in range and distinct across all entries."""
    owner = np.zeros(n_flat, dtype=np.int32)
    layout = OrderedDict()
    for name, a in gathered.items():
        idx = np.asarray(a, dtype=np.float64)
        assert np.array_equal(idx, np.round(idx)) and idx.min() >= 0 and idx.max() < n_flat, name
        idx = idx.astype(np.int64)
        np.add.at(owner, idx.ravel(), 1)
        layout[name] = idx
    assert owner.max() <= 1, "two entries share a flat offset"
    return layout, owner == 0


def search_setups():
    """print (k, b) of every saturated setup for the seeds 0..9: median logit at 0, farthest at +-80"""
    for (model, shape) in SMALL_SHAPES + LARGE_SHAPES:
        for seed in range(6):
            SETUPS[(model, shape, "probe")] = (seed, 1.0, 0.0)
            r = oracle_logits(model, shape, "probe").double().numpy()
            med = float(np.median(r))
            k = 80.0 / float(np.abs(r - med).max())
            k = float(f"{k:.4g}")
            b = float(f"{-k * med:.6g}")
            SETUPS[(model, shape, "probe")] = (seed, k, b)
            print(model, shape, "seed", seed, "k", k, "b", b, coverage(oracle_logits(model, shape, "probe").numpy()), flush=True)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    search_setups()
