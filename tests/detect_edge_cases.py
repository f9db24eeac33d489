"""The detector's box, loss and RoIAlign kernels (csrc/rpn_kernels.hip, csrc/detect_kernels.hip) at their edges: case tables,
float64 references and float32 restatements, NumPy on the CPU only.  test_detect_edge_cases_host.py pins the tables without a
GPU, test_gpu_detect_edges.py runs them on the device.  An e_ref is the error of the float32 restatement (the kernel's
expressions in the kernel's order, NumPy's exp / log in place of the device's) against the float64 reference: what float32
costs on these inputs, measured, and the device is allowed twice that or a floor of a few float32 steps.

A. LOSSES.  ``rpn_ref`` / ``frc_ref`` with ``f=np.float64`` are closed forms in log space,

    softplus(x) = max(x, 0) + log1p(exp(-|x|)),   BCE(x, t) = softplus(x) - x t = softplus(-x) [t = 1] | softplus(x) [t = 0]
    d BCE / dx = p - t = -exp(-softplus(x)) [t = 1] | exp(-softplus(-x)) [t = 0]
    CE(x, c) = lse(x) - x_c,  d/dx_j = p_j - [j = c],  p_j = exp(x_j - lse),  the label's own: -sum_{j != c} p_j
    smooth L1 (e = head - target, ae = |e|):  ae < beta: e^2 / (2 beta), slope e / beta;  else ae - beta / 2, slope sign(e)

(the ``ae < beta`` branch as rpn_kernels.hip documents it: a residual of exactly +-beta is on the linear side), beta the
float32 the kernel receives, every term / max(num_sampled, 1) (rpn_loss) or / R (fastrcnn_loss).  With ``f=np.float32`` the
same functions restate the kernels term for term.  Bounds: ``loss_bound`` and ``grad_bound`` of loss_step_cases.py.
Crafted residuals (``residuals``): +-beta, one float32 step inside and outside, 0 and +-1e4, on every third positive row.

B. BOX DECODE / ENCODE.  Reference ``detection_ref.decode_boxes`` in float64; an error is counted in float32 steps at
|pcx| + pw (|pcy| + ph), the bound is max(2 e_ref, 4) of them.

C. EXACT TIES.  Integer boxes below 2048 with sides of at most 10, thresholds from {0.25, 0.5, 0.75}: areas, intersections
and unions are exact in float32 (fused or not), a quotient that equals a threshold is computed exactly, and every other one is at least
1 / (4 x 164) from it (``iou_exactness`` asserts 1e-4), so float32 and float64 decide alike and NOTHING may differ.
A pair of boxes whose union is 0 has no IoU (0 / 0): it never matches -- the anchor keeps IoU "-1" (label 0 unless another
ground truth reaches it), it is never a low-quality match, and in NMS it suppresses nothing.

D. ROIALIGN.  Reference ``detection_ref.roi_align`` / ``roi_align_backward`` (plain loops).  ``roi_align_np`` /
``roi_align_bwd_np`` restate roi_geom, bilin and the per-bin weight sums term for term in ``f``; in float64 they agree with
the loops to 1e-12 (host test), which lets the large cases be compared everywhere and not only on the named rows.  Scales
are powers of two (the products with them are exact); the boundary cases use
dyadic coordinates whose float32 and float64 sample positions are EQUAL, every other case keeps its samples 1e-3 away from
-1, H and W (the only discontinuities of the sampling rule) and has the same adaptive grid in both precisions.

E. MASK TARGETS.  Integer-aligned RoIs with bins of 1 and 2 pixels and 2 x 2 samples on 0/1 masks: every weight is a multiple
of 1/4, every average a multiple of 1/64, exact in float32 -- averages of exactly 0.25, 0.5 and 0.75 occur, and the device
must equal the reference everywhere.

MEASURED on the CPU (python tests/detect_edge_cases.py).  coverage = fraction below -20 / above +20 / count in |x| < 1 /
max |x| of the saturated logits; e_ref in units of 2^-24 max |g64| (A) or 2^-24 max |want| (D), the largest over the cases of
the row; dloss: the float32 restatement's loss error in units of 2^-24 max(1, |loss64|).

  A  rpn_loss         cases  coverage                  e_ref default  saturated  dloss
     P 37 A 4            80  0.358/0.291/27/80.0            1.86         1.44     1.01
     P 37 A 12           20  0.270/0.351/89/80.0            1.71         2.08     0.87
     P 65601 A 4          2  0.299/0.300/52809/80.0         2.22         2.29     0.86
     fastrcnn_loss
     R 1 K1 2, 5, 6      48  (2 .. 6 logits: no coverage)    3.04        15.68     1.82
     R 37 K1 2           16  0.311/0.351/12/80.0            2.96        28.08     0.99
     R 37 K1 5           16  0.216/0.373/32/80.0            2.05        58.90     1.28
     R 37 K1 6           16  0.207/0.378/45/80.0            3.01        44.40     1.22
     R 262400 K1 2        2  0.313/0.388/79269/80.0         6.31        65.84     0.66
  In the saturated fastrcnn rows the label's logit is the largest in rows 0 mod 4 and more than 80 below every other in rows 1
  mod 4.  Their e_ref of 16 .. 66 is lse = mx + log(se) rounded at |mx| = 80: half a step of 80 is 64 x 2^-24, and exp(x - lse)
  carries it into every probability; the kernel's gradient shares it term for term (its loss no longer does, see FOUND).  In
  the all-background single rows the whole float64 gradient lies below 1e-30: float32 gives 0 and e_ref is max |g64| itself.

  B  box_decode       e_ref in float32 steps at |pc| + p
     the table, clipped and not   1.01      1,048,800 random rows   4.34 (the 128 named rows: 1.03)      encode -> decode   1.00

  D  RoIAlign                              e_ref forward  backward
     boundary (10 cases)                        0.84        1.06
     shapes (outside, ten times, sub-pixel)     5.03        3.85
     random 5x9, 1x9, 5x1                       5.52        4.67
     random / adaptive 32x32                   48.94       29.85      (a coordinate near 32 carries 32 x 2^-24 into its weights)
     zero size                                  2.06        1.44
     counts 0, 1, 128, 129, 300                 7.48        5.96
     forward trip 16x20x576 / backward trip 128x132x256   33.50 / 124.13
     multi-level C 4 .. 1024                   14.18       10.72      counts 11.17 / 7.89     64x72 trip 62.69 / 32.55

ON AN MI355X (the DETEDGE lines of test_gpu_detect_edges.py, 278 tests in 5.4 s).  A: rpn_loss at most 1.01 x 2^-24 max(1,
|loss|) from float64 (bound 8) and 2.29 x 2^-24 max |g64| on the gradient, fastrcnn_loss 1.82 and 64.8 (the lse rounding above):
the gradient error is at most 0.52 of the bound and equals the restatement's wherever e_ref exceeds the floor; every element
finite, the zeros exact, second runs identical.  B: at most 1.01 float32 steps (bound 4); clipped boxes lie in [0, clip]
and on the bound bit for bit.  C: no element differs -- 8 images x 6 settings, 65,836 anchors x 3 settings, NMS at 6 sizes x 3
thresholds, 40 sets of 256 x 3 thresholds.  D: the library is built with -ffp-contract=off and the restatement follows the
kernels' order, so forward and backward come out at exactly 0.50 of the bound -- the restatement's own error -- wherever e_ref
exceeds the floor (every random, adaptive, counts, trip and multi-level case), the boundary cases at most 0.26, the zero-size
cases at 0.36 after the fix below; the adjoint identity holds to under 1 % of what the two bounds allow.
E: 2,304 exact outputs, 406 of them averages of exactly 0.5, and 7,840 random ones: no mismatch, none left out.

FOUND with these cases: (1) roi_align_bwd_gather_kernel took its bin range from (pixel - start) / bin size.  An aligned RoI with
x1 == x2 or y1 == y2 has a bin size of 0: the quotient is +-inf or NaN, the conversion to int saturates and the -1 / +1 wrap, the
range came out empty on every pixel but the map's border rows and columns, and the RoI's gradient was dropped -- 3.67 and 2.59
against bounds of 1.4e-6 and 1.1e-6 in the two zero-size cases -- while the forward pass samples the RoI's edge and returns
non-zero outputs.  The kernel now scans every bin of an axis whose bin size is not positive and finite; for every other RoI
the range is computed as before, bit for bit.  (2) fastrcnn_loss_kernel summed lse - x[label] with lse = mx + log(se) already
rounded at the magnitude of mx: with logits of 80 a single row's loss of 0.3133 came out 21.0 x 2^-24 off (bound 8; the eighteen
saturated R = 1 cases with a foreground label).  It now sums (mx - x[label]) + log(se); the same cases are at 0.5 and below.
NOT a defect: the first restatement of the backward summed each RoI's bins before adding the RoI to the pixel; with 300 RoIs on
a 5 x 9 map the kernel's own order (bin by bin) came out at 1.15 and 1.72 of twice that restatement's error.  Restated in the
kernel's order the two agree bit for bit, and the bound is measured from that.
"""
import math
from collections import namedtuple

import numpy as np

from loss_step_cases import U24, coverage, grad_bound, loss_bound   # noqa: F401  (the project's own bounds)

F32, F64 = np.float32, np.float64
RANGES = ("default", "saturated")
BETAS = (1.0 / 9, 0.125)


def _btag(beta):
    return "b8th" if beta == 0.125 else "b9th"


# ------------------------------------------------------------------------------------------------------------ A: losses
RpnCase = namedtuple("RpnCase", "id P A logits beta labels ns")
FrcCase = namedtuple("FrcCase", "id R K1 logits beta labels")
RPN_LABELS = ("random", "none", "all_pos", "all_neg", "one_pos")
FRC_LABELS = ("random", "all_bg", "all_fg", "one_fg")
NS = ("zero", "one", "count", "count7")


def _rpn(P, A, r, beta, lab, ns):
    return RpnCase(f"P{P}_A{A}_{r}_{_btag(beta)}_{lab}_ns{ns}", P, A, r, beta, lab, ns)


def _frc(R, K1, r, beta, lab):
    return FrcCase(f"R{R}_K{K1}_{r}_{_btag(beta)}_{lab}", R, K1, r, beta, lab)


RPN_CASES = [_rpn(37, 4, r, b, lab, ns) for r in RANGES for b in BETAS for lab in RPN_LABELS for ns in NS]
RPN_CASES += [_rpn(37, 12, r, b, lab, NS[(i + j + k) % 4]) for i, r in enumerate(RANGES) for j, b in enumerate(BETAS)
              for k, lab in enumerate(RPN_LABELS)]
RPN_CASES += [_rpn(65601, 4, "default", BETAS[0], "random", "count"), _rpn(65601, 4, "saturated", BETAS[1], "random", "count7")]
FRC_CASES = [_frc(R, K1, r, b, lab) for R in (1, 37) for K1 in (2, 5, 6) for r in RANGES for b in BETAS for lab in FRC_LABELS]
FRC_CASES += [_frc(262400, 2, "default", BETAS[1], "random"), _frc(262400, 2, "saturated", BETAS[0], "random")]


def residuals(beta):
    """the crafted smooth-L1 residuals for the float32 `beta` the kernel receives"""
    b = F32(beta)
    inside, outside = np.nextafter(b, F32(0)), np.nextafter(b, F32(np.inf))
    return np.array([b, -b, inside, -inside, outside, -outside, 0.0, 1e4, -1e4], F32)


def logits_of(n, kind, rng):
    if kind == "default":
        return (rng.standard_normal(n) * 1.5).astype(F32)
    x = rng.uniform(-80.0, 80.0, n)
    near = rng.random(n) < 0.2
    x[near] = rng.standard_normal(int(near.sum())) * 0.5
    x = x.astype(F32)
    x[:2] = (80.0, -80.0)[:n]
    return x


def _craft(rows, beta, deltas, targets):
    """residuals() cycled over the four coordinates of `rows`; -> (rows, 4) intended residuals.  The exact +-0.125 sit on a
    target of 0.25 (0.375 and 0.125 are float32s), every other on a target of 0"""
    res = residuals(beta)
    rr = res[(4 * np.arange(len(rows))[:, None] + np.arange(4)) % len(res)]
    t = np.where((F32(beta) == F32(0.125)) & (np.abs(rr) == F32(0.125)), F32(0.25), F32(0)).astype(F32)
    targets[rows] = t
    deltas[rows] = (t + rr).astype(F32)
    return rr


def rpn_inputs(case):
    """head (P, 5 A), labels (P A,) int8, targets (P A, 4), num_sampled, crafted rows, their intended residuals"""
    n = case.P * case.A
    rng = np.random.default_rng([case.P, case.A, RANGES.index(case.logits)])
    x = logits_of(n, case.logits, rng)
    deltas, targets = (rng.standard_normal((n, 4)) * 0.5).astype(F32), (rng.standard_normal((n, 4)) * 0.3).astype(F32)
    lab = {"none": np.full(n, -1), "all_pos": np.ones(n), "all_neg": np.zeros(n), "one_pos": np.zeros(n),
           "random": np.random.default_rng(n + 7).choice([-1, 0, 1], n, p=[0.5, 0.35, 0.15])}[case.labels].astype(np.int8)
    if case.labels == "one_pos":
        lab[n // 3] = 1
    rows = np.flatnonzero(lab > 0)[::3]
    want = _craft(rows, case.beta, deltas, targets)
    head = np.empty((case.P, 5 * case.A), F32)
    head[:, :case.A], head[:, case.A:] = x.reshape(case.P, case.A), deltas.reshape(case.P, 4 * case.A)
    count = int((lab >= 0).sum())
    return head, lab, targets, {"zero": 0, "one": 1, "count": count, "count7": 7 * count}[case.ns], rows, want


def frc_inputs(case):
    """head (R, 5 K1), labels (R,) int32, targets (R, 4), crafted rows, their intended residuals.  Saturated: in rows 0 mod 4
    the label's logit is 80 and every other at most 79, in rows 1 mod 4 it is -80 and every other at least 0.5"""
    R, K1 = case.R, case.K1
    rng = np.random.default_rng([R, K1, RANGES.index(case.logits)])
    x = logits_of(R * K1, case.logits, rng).reshape(R, K1)
    lab = {"all_bg": np.zeros(R), "all_fg": 1 + np.arange(R) % (K1 - 1), "one_fg": np.zeros(R),
           "random": np.random.default_rng(R + K1).integers(0, K1, R)}[case.labels].astype(np.int32)
    if case.labels == "one_fg":
        lab[R // 3] = K1 - 1
    if case.logits == "saturated":
        own = np.arange(K1)[None, :] == lab[:, None]
        top, bottom = (np.arange(R) % 4 == 0)[:, None], (np.arange(R) % 4 == 1)[:, None]
        x = np.where(top & ~own, np.minimum(x, F32(79)), x)
        x = np.where(bottom & ~own, np.maximum(np.abs(x), F32(0.5)), x)
        x = np.where(top & own, F32(80), np.where(bottom & own, F32(-80), x)).astype(F32)
    deltas, targets = (rng.standard_normal((R, K1, 4)) * 0.5).astype(F32), (rng.standard_normal((R, 4)) * 0.3).astype(F32)
    rows = np.flatnonzero(lab > 0)[::3]
    own_d, own_t = deltas[rows, lab[rows]], targets[rows]                       # (copies: the label's own deltas of the crafted rows)
    want = _craft(np.arange(len(rows)), case.beta, own_d, own_t)
    deltas[rows, lab[rows]], targets[rows] = own_d, own_t
    return np.concatenate([x, deltas.reshape(R, 4 * K1)], 1), lab, targets, rows, want


def _softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def _smooth_l1(e, beta, inv, f):
    """(terms, slopes * inv) in `f`, the kernels' expressions"""
    b, ae = f(F32(beta)), np.abs(e)
    quad = ae < b
    return np.where(quad, f(0.5) * e * e / b, ae - f(0.5) * b), np.where(quad, e / b * inv, np.where(e > 0, inv, -inv))


def _finish(total, inv, f):
    return float(total * float(inv)) if f is F64 else float(F32(total * float(inv)))


def rpn_ref(head, labels, targets, A, beta, num_sampled, f=F64):
    """(objectness loss, box loss, d(sum)/d(head) (P, 5 A)): float64 closed forms, or (f = float32) rpn_loss_kernel's text"""
    head = np.asarray(head, F32).astype(f).reshape(-1, 5 * A)
    P = len(head)
    x, d = head[:, :A].reshape(-1), head[:, A:].reshape(-1, 4)
    lab, t = np.asarray(labels).reshape(-1), np.asarray(targets, F32).astype(f).reshape(-1, 4)
    samp, pos = lab >= 0, lab > 0
    inv = f(1) / f(max(int(num_sampled), 1))
    if f is F64:
        sp, sn = _softplus(x), _softplus(-x)
        bce, dx = np.where(pos, sn, sp), np.where(pos, -np.exp(-sp), np.exp(-sn))
    else:
        tt = pos.astype(f)
        bce = np.maximum(x, f(0)) - x * tt + np.log1p(np.exp(-np.abs(x)))
        dx = f(1) / (f(1) + np.exp(-x)) - tt
    sl1, ge = _smooth_l1(d - t, beta, inv, f)
    g = np.zeros((P, 5 * A), f)
    g[:, :A] = np.where(samp, dx * inv, f(0)).reshape(P, A)
    g[:, A:] = np.where(pos[:, None], ge, f(0)).reshape(P, 4 * A)
    return _finish(bce[samp].astype(F64).sum(), inv, f), _finish(sl1[pos].astype(F64).sum(), inv, f), g


def frc_ref(head, labels, targets, beta, f=F64):
    """(classification loss, box loss, d(sum)/d(head) (R, 5 K1)): float64 closed forms, or fastrcnn_loss_kernel's text"""
    head = np.asarray(head, F32).astype(f)
    R, K1 = head.shape[0], head.shape[1] // 5
    x, d = head[:, :K1], head[:, K1:].reshape(R, K1, 4)
    lab, t = np.asarray(labels).reshape(-1), np.asarray(targets, F32).astype(f).reshape(R, 4)
    own = np.arange(K1)[None, :] == lab[:, None]
    inv = f(1) / f(R)
    mx = x.max(1, keepdims=True)
    if f is F64:
        lse = mx + np.log(np.exp(x - mx).sum(1, keepdims=True))
        p = np.exp(x - lse)
        dcls = np.where(own, -(np.where(own, 0.0, p).sum(1, keepdims=True)), p)
    else:
        se = np.zeros((R, 1), f)
        for j in range(K1):
            se = se + np.exp(x[:, j:j + 1] - mx)
        lg = np.log(se)
        lse = mx + lg
        dcls = np.exp(x - lse) - own.astype(f)
    if f is F64:
        cls = (lse[:, 0] - x[np.arange(R), lab]).sum()
    else:
        cls = ((mx[:, 0] - x[np.arange(R), lab]) + lg[:, 0]).astype(F64).sum()         # (mx - x_c) + log(se): no cancellation against mx
    fg = lab > 0
    sl1, ge = _smooth_l1(d[np.arange(R), lab] - t, beta, inv, f)
    g = np.zeros((R, 5 * K1), f)
    g[:, :K1] = dcls * inv
    gb = np.zeros((R, K1, 4), f)
    gb[np.flatnonzero(fg), lab[fg]] = ge[fg]
    g[:, K1:] = gb.reshape(R, 4 * K1)
    return _finish(cls, inv, f), _finish(sl1[fg].astype(F64).sum(), inv, f), g


def loss_figures(ref, *args):
    """((l1, l2, g) in float64, e_ref = max |g32 - g64|, the float32 restatement's two loss errors)"""
    w, r = ref(*args, f=F64), ref(*args, f=F32)
    return w, float(np.abs(r[2].astype(F64) - w[2]).max()), (abs(r[0] - w[0]), abs(r[1] - w[1]))


# ------------------------------------------------------------------------------------------------------------ B: decode
CLAMP = F32(4.135166556742356)                       # log(1000 / 16), the float32 the kernel clamps at
CLIP = (128.0, 160.0)                                # (H, W)
DECODE_ANCHORS = np.array([[8, 8, 24, 24], [40, 16, 104, 48], [0, 0, 160, 128], [100.5, 60.25, 146, 93.75], [3, 90, 35, 122],
                           [60, 60, 61, 61], [120, 10, 152, 74], [16, 32, 48.5, 64.5], [70, 5, 77.25, 12.5], [0, 100, 45.5, 120],
                           [90, 90, 154, 122], [30, 30, 94, 94]], F32)
DECODE_LARGE = 12 * 87400                            # 1,048,800 rows: 224 of them in the second trip of 4096 x 256 threads


def decode_deltas():
    """the table: one pattern per 12 rows (row i uses anchor i mod 12)"""
    up, down = np.nextafter(CLAMP, F32(np.inf)), np.nextafter(CLAMP, F32(0))
    pats = []
    for v in (CLAMP, up, down, 9.0, -80.0, 0.0):
        pats += [(0.3, -0.7, v, 0.0), (-0.2, 0.4, 0.0, v), (0.1, 0.1, v, v)]
    pats += [(0, 0, 0, 0), (50, 0, 0, 0), (-50, 0, 0, 0), (0, 50, 0, 0), (0, -50, 0, 0), (50, 50, 1.0, 1.0), (-50, -50, 1.0, 1.0)]
    pats += [tuple(r) for r in np.random.default_rng(11).standard_normal((20, 4)) * 0.5]
    return np.repeat(np.asarray(pats, F32), len(DECODE_ANCHORS), axis=0)


def decode_large_deltas():
    return (np.random.default_rng(12).standard_normal((DECODE_LARGE, 4)) * 0.5).astype(F32)


DECODE_LARGE_ROWS = np.concatenate([np.linspace(0, 4096 * 256 - 1, 64).astype(np.int64), 4096 * 256 + np.arange(64) * 3])


def decode32(anchors, deltas, clip=None):
    """box_decode_kernel's text in float32"""
    a, d = np.asarray(anchors, F32), np.asarray(deltas, F32)
    a = a[np.arange(len(d)) % len(a)]
    w, h = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    cx, cy = a[:, 0] + F32(0.5) * w, a[:, 1] + F32(0.5) * h
    dw, dh = np.minimum(d[:, 2], CLAMP), np.minimum(d[:, 3], CLAMP)
    pcx, pcy, pw, ph = d[:, 0] * w + cx, d[:, 1] * h + cy, np.exp(dw) * w, np.exp(dh) * h
    b = np.stack([pcx - F32(0.5) * pw, pcy - F32(0.5) * ph, pcx + F32(0.5) * pw, pcy + F32(0.5) * ph], 1)
    if clip is not None:
        b[:, 0::2], b[:, 1::2] = np.clip(b[:, 0::2], 0, F32(clip[1])), np.clip(b[:, 1::2], 0, F32(clip[0]))
    return b.astype(F32)


def decode_steps(anchors, deltas):
    """(n, 4): one float32 step at |pcx| + pw (columns 0, 2) and at |pcy| + ph (columns 1, 3), from float64"""
    a, d = np.asarray(anchors, F64), np.asarray(deltas, F64)
    a = a[np.arange(len(d)) % len(a)]
    w, h = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    lim = np.log(1000.0 / 16)
    mx = np.abs(d[:, 0] * w + a[:, 0] + 0.5 * w) + np.exp(np.minimum(d[:, 2], lim)) * w
    my = np.abs(d[:, 1] * h + a[:, 1] + 0.5 * h) + np.exp(np.minimum(d[:, 3], lim)) * h
    s = np.spacing(np.stack([mx, my, mx, my], 1).astype(F32)).astype(F64)
    return s


def decode_bound(e_ref_steps):
    return max(2.0 * e_ref_steps, 4.0)


def roundtrip_boxes():
    """(anchors, gt) (40, 4) float32: gt i is anchor i moved by up to 3 % and resized by up to 5 %, so that anchor i matches gt i"""
    rng = np.random.default_rng(13)
    x0, y0 = rng.uniform(0, 900, 40), rng.uniform(0, 900, 40)
    w, h = rng.uniform(8, 120, 40), rng.uniform(8, 120, 40)
    x0, y0 = x0 + 130 * np.arange(40), y0 + 0 * np.arange(40)                # apart: anchor i overlaps gt i only
    a = np.stack([x0, y0, x0 + w, y0 + h], 1)
    gx, gy = x0 + rng.uniform(-0.03, 0.03, 40) * w, y0 + rng.uniform(-0.03, 0.03, 40) * h
    gw, gh = w * rng.uniform(0.95, 1.05, 40), h * rng.uniform(0.95, 1.05, 40)
    return a.astype(F32), np.stack([gx, gy, gx + gw, gy + gh], 1).astype(F32)


def encode32(anchors, gt):
    """the encode of anchor_match_batched_kernel in float32"""
    a, g = np.asarray(anchors, F32), np.asarray(gt, F32)
    aw, ah, gw, gh = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1], g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    h = F32(0.5)
    return np.stack([((g[:, 0] + h * gw) - (a[:, 0] + h * aw)) / aw, ((g[:, 1] + h * gh) - (a[:, 1] + h * ah)) / ah,
                     np.log(gw / aw), np.log(gh / ah)], 1).astype(F32)


# ------------------------------------------------------------------------------------------------------------ C: exact ties
THRESHOLDS = (0.25, 0.5, 0.75)
MATCH_SETTINGS = [(hi, lo, lq) for hi, lo in ((0.75, 0.25), (0.5, 0.25), (0.75, 0.5)) for lq in (True, False)]
G44 = (0, 0, 4, 4)
IN_THIRDS = [(100, 100, 102, 101), (102, 103, 104, 104), (100, 103, 102, 104)]         # three boxes of IoU 2/16 with (100,100,104,104)
# name -> (ground truth, anchors); the IoUs with (0,0,4,4): 4x3 0.75, 4x2 0.5, 4x1 0.25, 3x3 9/16, 1x1 1/16
MATCH_IMAGES = {
    "thresholds": ([G44], [(0, 0, 4, 3), (0, 0, 4, 2), (0, 0, 4, 1), (0, 0, 3, 3), (0, 0, 1, 1), (20, 20, 24, 24)]),
    "identical_gts": ([G44, G44], [G44, (0, 0, 4, 3), (0, 0, 2, 2), (0, 0, 4, 1)]),
    "tied_anchor": ([(0, 0, 4, 3), (0, 1, 4, 4), (0, 0, 4, 3)], [G44, (0, 1, 4, 4), (0, 0, 4, 2)]),
    "low_quality_three": ([(100, 100, 104, 104), G44], IN_THIRDS + [G44, (100, 100, 101, 101)]),
    "lonely_gt": ([(500, 500, 510, 510), G44], [G44, (0, 0, 4, 1), (30, 30, 34, 34)]),
    "no_gt": ([], [G44, (0, 0, 4, 1), (7, 7, 7, 7)]),
    "zero_area": ([(5, 5, 5, 5), G44], [(5, 5, 5, 5), (5, 5, 5, 9), G44, (7, 7, 7, 7), (0, 0, 4, 2), (5, 5, 9, 9)]),
    "zero_area_only": ([(5, 5, 5, 5)], [(5, 5, 5, 5), G44, (5, 5, 9, 9), (5, 3, 5, 7)]),
}
MATCH_LARGE_N = 65836                                # 256 blocks x 256 threads = 65,536: 300 anchors in the second trip
MATCH_LARGE_GT = [G44, (100, 100, 104, 104), (500, 500, 510, 510), (50, 50, 58, 56), (52, 51, 60, 59), (5, 5, 5, 5), G44]


def match_batch():
    """The table as one batch with per-image anchors: anchors (B, n, 4), anchor counts, gt (B, Gmax, 4), gt counts, names.
    The rows behind the counts hold boxes that WOULD match: anchors equal to (0,0,4,4), ground truth equal to it too"""
    names = list(MATCH_IMAGES)
    n = max(len(a) for _, a in MATCH_IMAGES.values()) + 2
    gmax = max(len(g) for g, _ in MATCH_IMAGES.values()) + 1
    anchors, gt = np.tile(np.asarray(G44, F32), (len(names), n, 1)), np.tile(np.asarray(G44, F32), (len(names), gmax, 1))
    ac, gc = np.zeros(len(names), np.int32), np.zeros(len(names), np.int32)
    for i, k in enumerate(names):
        g, a = MATCH_IMAGES[k]
        anchors[i, :len(a)], ac[i], gc[i] = np.asarray(a, F32), len(a), len(g)
        if g:
            gt[i, :len(g)] = np.asarray(g, F32)
    return anchors, ac, gt, gc, names


def match_large_anchors():
    """65,836 integer anchors with sides 0 .. 8 around the ground truths, the table's anchors at both ends"""
    rng = np.random.default_rng(21)
    n = MATCH_LARGE_N
    x0, y0 = rng.integers(0, 120, n), rng.integers(0, 120, n)
    a = np.stack([x0, y0, x0 + rng.integers(0, 9, n), y0 + rng.integers(0, 9, n)], 1).astype(F32)
    table = np.asarray(MATCH_IMAGES["thresholds"][1] + IN_THIRDS + [(5, 5, 5, 5), (50, 50, 58, 56), (500, 500, 505, 510)], F32)
    a[:len(table)] = table
    a[n - len(table):] = table[::-1]
    return a


def _pair_terms(a, b):
    """integer intersections and unions (len(a), len(b)) of integer boxes"""
    a, b = np.asarray(a, np.int64).reshape(-1, 4), np.asarray(b, np.int64).reshape(-1, 4)
    iw = np.clip(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), 0, None)
    ih = np.clip(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), 0, None)
    inter = iw * ih
    area = lambda q: (q[:, 2] - q[:, 0]) * (q[:, 3] - q[:, 1])
    return inter, area(a)[:, None] + area(b)[None, :] - inter


def iou_exactness(a, b):
    """(every pair's IoU equals a threshold exactly or is 1e-4 and more from all of them, pairs on a threshold, pairs
    without an IoU)"""
    a, b = np.asarray(a), np.asarray(b)
    ints = np.array_equal(a, np.round(a)) and np.array_equal(b, np.round(b)) and 0 <= min(a.min(), b.min()) and max(a.max(), b.max()) < 2048
    inter, union = _pair_terms(a, b)
    has = union > 0
    on = np.zeros(inter.shape, bool)
    far = np.ones(inter.shape, bool)
    for k in (1, 2, 3):
        on |= has & (4 * inter == k * union)
        far &= np.abs(inter / np.where(has, union, 1) - k / 4.0) >= 1e-4
    return bool(ints and (on | far | ~has).all()), int(on.sum()), int((~has).sum())


def ref_anchor_match(anchors, gt, hi, lo, lq):
    from oracle import detection_ref
    with np.errstate(invalid="ignore", divide="ignore"):
        return detection_ref.anchor_match(anchors, gt, hi, lo, lq)


def ref_nms(boxes, thr):
    """keep indices of boxes given in descending score order"""
    from oracle import detection_ref
    with np.errstate(invalid="ignore", divide="ignore"):
        return detection_ref.nms(boxes, -np.arange(len(boxes), dtype=F32), thr)


def _tie(thr, off):
    """(a, b) with IoU exactly thr"""
    return (off, off, off + 4, off + 4), (off, off, off + 4, off + int(4 * thr))


def nms_boxes(n, thr, seed=0):
    """n integer boxes in score order: sides 0 .. 8 scattered densely; then, on their own ground, a pair exactly on thr, the
    chain a -> b -> c, a pair of identical boxes and two zero-area boxes at the front, and the same once across every
    64-column word boundary the set has (the suppressor in one word, the suppressed in the next)"""
    rng = np.random.default_rng([n, seed])
    s = 4 + int(math.sqrt(n))
    x0, y0 = rng.integers(0, s, n), rng.integers(0, s, n)
    b = np.stack([x0, y0, x0 + rng.integers(0, 9, n), y0 + rng.integers(0, 9, n)], 1).astype(F32)

    def put(slots, off):
        t0, t1 = _tie(thr, off)
        h, s = {0.25: (8, 4), 0.5: (4, 1), 0.75: (8, 1)}[thr]      # IoU (h - s) / (h + s) > thr one shift apart, (h - 2 s) / (h + 2 s) <= thr two
        fig = [t0, t1, (off + 20, off, off + 24, off + h), (off + 20, off + s, off + 24, off + s + h), (off + 20, off + 2 * s, off + 24, off + 2 * s + h),
               (off + 40, off, off + 44, off + 4), (off + 40, off, off + 44, off + 4), (off + 60, off, off + 60, off + 4)]
        for i, q in zip(slots, fig):
            if 0 <= i < n:
                b[i] = q
    put(range(8), 300)
    for k, w in enumerate(range(64, n, 64)):
        if k < 3 or w + 64 >= n:                     # the first boundaries and the last one
            put([w - 1, w, w - 2, w + 1, w + 2, w - 3, w + 3, w - 4], 400 + 100 * (k % 12))
    return b


NMS_SIZES = (1, 8, 64, 65, 129, 2000)
NMSB_K, NMSB_SETS = 256, 40


def nms_batched_sets(thr):
    """(boxes (40, 256, 4), counts): counts cycle through 0, 1, 255, 256; the rows behind a count repeat its first box"""
    counts = np.array([(0, 1, 255, 256)[i % 4] for i in range(NMSB_SETS)], np.int32)
    boxes = np.stack([nms_boxes(NMSB_K, thr, seed=100 + i) for i in range(NMSB_SETS)])
    for i, c in enumerate(counts):
        boxes[i, c:] = boxes[i, 0]
    return boxes, counts


# ------------------------------------------------------------------------------------------------------------ D: RoIAlign
def roi_geom_np(roi, scale, PH, PW, sr, aligned, f):
    """roi_geom() of detect_kernels.hip in `f`: (image, y1, x1, bin h, bin w, grid h, grid w)"""
    q, s, off = np.asarray(roi, F32).astype(f), f(scale), f(0.5 if aligned else 0.0)
    x1, y1 = q[1] * s - off, q[2] * s - off
    rw, rh = q[3] * s - off - x1, q[4] * s - off - y1
    if not aligned:
        rw, rh = max(rw, f(1)), max(rh, f(1))
    gh = sr if sr > 0 else int(np.ceil(rh / f(PH)))
    gw = sr if sr > 0 else int(np.ceil(rw / f(PW)))
    return int(q[0]), y1, x1, rh / f(PH), rw / f(PW), max(gh, 0), max(gw, 0)


def axis_samples(start, bs, P, g, f):
    """(P, g) sample coordinates along one axis: start + p * bs + (s + 0.5) * bs / g, the kernel's expression"""
    p, s = np.arange(P).astype(f)[:, None], np.arange(g).astype(f)[None, :]
    return ((start + p * bs) + (s + f(0.5)) * bs / f(max(g, 1))).astype(f)


def axis_bilin(v, L, f):
    """axis_of(): (inside [-1, L], p0, p1, weight of p0, weight of p1)"""
    ok = ~((v < f(-1)) | (v > f(L)))
    v = np.where(v <= 0, f(0), v)
    p0 = np.minimum(v, f(2 ** 30)).astype(np.int64)
    top = p0 >= L - 1
    p0 = np.where(top, L - 1, p0)
    p1 = np.where(top, L - 1, p0 + 1)
    v = np.where(top, p0.astype(f), v)
    l = (v - p0.astype(f)).astype(f)
    return ok, p0, p1, (f(1) - l).astype(f), l


def roi_samples(rois, scale, PH, PW, sr, aligned, f):
    """per RoI: (image, y (PH, gh), x (PW, gw)) in `f`"""
    out = []
    for roi in np.asarray(rois, F32).reshape(-1, 5):
        n, y1, x1, bh, bw, gh, gw = roi_geom_np(roi, scale, PH, PW, sr, aligned, f)
        out.append((n, axis_samples(y1, bh, PH, gh, f), axis_samples(x1, bw, PW, gw, f)))
    return out


def roi_align_np(x, rois, scale, output_size, sr=2, aligned=False, f=F32):
    """roi_align_fwd_kernel in `f`: x (N, H, W, C), rois (R, 5) -> (R, PH, PW, C)"""
    PH, PW = output_size
    x = np.asarray(x, F32).astype(f)
    N, H, W, C = x.shape
    rois = np.asarray(rois, F32).reshape(-1, 5)
    out = np.zeros((len(rois), PH, PW, C), f)
    for r, (n, ys, xs) in enumerate(roi_samples(rois, scale, PH, PW, sr, aligned, f)):
        gh, gw = ys.shape[1], xs.shape[1]
        if not 0 <= n < N or gh * gw == 0:
            continue
        oky, y0, y1, hy, ly = axis_bilin(ys, H, f)
        okx, x0, x1, hx, lx = axis_bilin(xs, W, f)
        acc = np.zeros((PH, PW, C), f)
        for iy in range(gh):
            for ix in range(gw):
                a, b = (slice(None), iy), (slice(None), ix)
                w = lambda wy, wx: (wy[a][:, None] * wx[b][None, :])[..., None].astype(f)
                v = lambda py, px: x[n][py[a][:, None], px[b][None, :]]
                term = v(y0, x0) * w(hy, hx) + v(y0, x1) * w(hy, lx) + v(y1, x0) * w(ly, hx) + v(y1, x1) * w(ly, lx)
                acc += np.where((oky[a][:, None] & okx[b][None, :])[..., None], term, f(0))
        out[r] = acc * (f(1) / f(gh * gw))
    return out


def _bin_weights(v, L, f):
    """bin_weight() for every (bin, pixel): (P, L), the samples of a bin summed in order"""
    ok, p0, p1, w0, w1 = axis_bilin(v, L, f)
    wm = np.zeros((v.shape[0], L), f)
    rows = np.arange(v.shape[0])
    for s in range(v.shape[1]):
        add = np.zeros_like(wm)
        add[rows, p0[:, s]] += np.where(ok[:, s], w0[:, s], f(0))
        add[rows, p1[:, s]] += np.where(ok[:, s] & (p1[:, s] != p0[:, s]), w1[:, s], f(0))
        wm += add
    return wm


def roi_align_bwd_np(dout, shape, rois, scale, sr=2, aligned=False, f=F32, base=None):
    """roi_align_bwd_gather_kernel in `f`, in the kernel's order: every pixel adds its RoIs in order, per RoI its bins row by row,
    each as acc += dout * ((wy * wx) * inv) with the product rounded before the sum (the library is built with -ffp-contract=off);
    the result is added to `base` (the multi-level kernel's read-modify-write).  With hundreds of RoIs on one pixel the order of
    the sum IS the float32 error: a restatement that summed per RoI first measured a third of what the kernel's order costs"""
    dout = np.asarray(dout, F32).astype(f)
    N, H, W, C = shape
    PH, PW = dout.shape[1:3]
    dx = np.zeros(shape, f)
    for r, (n, ys, xs) in enumerate(roi_samples(rois, scale, PH, PW, sr, aligned, f)):
        gh, gw = ys.shape[1], xs.shape[1]
        if not 0 <= n < N or gh * gw == 0:
            continue
        wy, wx, inv = _bin_weights(ys, H, f), _bin_weights(xs, W, f), f(1) / f(gh * gw)
        for by in range(PH):
            py = np.flatnonzero(wy[by])
            for bx in range(PW if len(py) else 0):
                px = np.flatnonzero(wx[bx])
                if not len(px):
                    continue
                w = ((wy[by, py][:, None] * wx[bx, px][None, :]).astype(f) * inv).astype(f)
                at = np.ix_(py, px)
                dx[n][at] = dx[n][at] + (dout[r, by, bx][None, None, :] * w[..., None]).astype(f)
    return dx if base is None else (np.asarray(base, F32).astype(f) + dx).astype(f)


def roi_bound(e_ref, want):
    return max(2.0 * e_ref, 4.0 * U24 * float(np.abs(want).max()) if np.size(want) else 0.0)


def samples_clear(rois, scale, PH, PW, sr, aligned, H, W, margin=1e-3):
    """every float64 sample is `margin` from -1, H and W, and the float32 grid (gh, gw) equals the float64 one"""
    s64, s32 = roi_samples(rois, scale, PH, PW, sr, aligned, F64), roi_samples(rois, scale, PH, PW, sr, aligned, F32)
    for (_, y, x), (_, y32, x32) in zip(s64, s32):
        if y.shape != y32.shape or x.shape != x32.shape:
            return False
        for v, L in ((y, H), (x, W)):
            if v.size and min(np.abs(v + 1).min(), np.abs(v - L).min()) < margin:
                return False
    return True


def random_rois(rng, counts, H, W, scale, PH, PW, sr, aligned, lo=0.3, hi=1.2):
    """image-major RoIs (sum(counts), 5) in image coordinates, each accepted by samples_clear"""
    out = []
    for n, c in enumerate(counts):
        while c > 0:
            x1, y1 = rng.uniform(-2.0, W - 0.5), rng.uniform(-2.0, H - 0.5)
            w, h = rng.uniform(lo, hi * W), rng.uniform(lo, hi * H)
            roi = np.array([n, x1 / scale, y1 / scale, (x1 + w) / scale, (y1 + h) / scale], F32)
            if samples_clear(roi, scale, PH, PW, sr, aligned, H, W):
                out.append(roi)
                c -= 1
    return np.asarray(out, F32).reshape(-1, 5)


def edge_values(L):
    """sample coordinates on and next to the validity boundary and the clamp points of an axis of L pixels"""
    return sorted({-1.0, float(np.nextafter(F32(-1), F32(-np.inf))), 0.0, float(L - 1), float(L), float(np.nextafter(F32(L), F32(np.inf)))})


def boundary_rois(H, W, scale, aligned):
    """RoIs whose single sample (PH = PW = 1, sampling ratio 1) is exactly (y, x), with their intended samples: every edge
    value of y at an inner x, every edge value of x at an inner y, and the edge values paired"""
    ys, xs = edge_values(H), edge_values(W)
    my, mx = (1.25 if H > 2 else 0.0), (3.25 if W > 4 else 0.0)
    pts = [(y, mx) for y in ys] + [(my, x) for x in xs] + [(ys[i % len(ys)], xs[i % len(xs)]) for i in range(max(len(ys), len(xs)))]
    lo, hi = (0.25, 0.75) if aligned else (-0.5, 0.5)                            # (aligned: minus the half pixel, a bin of 1/2)
    rois = [[0, (x + lo) / scale, (y + lo) / scale, (x + hi) / scale, (y + hi) / scale] for y, x in pts]
    return np.asarray(rois, F64), np.asarray(pts, F64)


RoiCase = namedtuple("RoiCase", "id kind N H W C scale PH PW sr aligned counts")
MAPS = ((5, 9), (1, 9), (5, 1), (32, 32))
ROI_COUNTS = (0, 1, 128, 129, 300)


def _roi(kind, H, W, *, N=1, C=4, scale=1.0, P=2, sr=2, aligned=False, counts=None, tag=""):
    cid = f"{kind}{tag}_{H}x{W}x{C}_s{scale:g}_p{P}_sr{sr}_{'aligned' if aligned else 'plain'}"
    return RoiCase(cid, kind, N, H, W, C, scale, P, P, sr, aligned, counts)


ROI_CASES = [_roi("boundary", H, W, scale=s, P=1, sr=1, aligned=al) for (H, W), s in zip(MAPS, (1.0, 0.5, 0.25, 0.125)) for al in (False, True)]
ROI_CASES += [_roi("boundary", 5, 9, scale=0.125, P=1, sr=1), _roi("boundary", 32, 32, scale=1.0, P=1, sr=1, aligned=True)]
ROI_CASES += [_roi("shapes", H, W, N=2, scale=s, P=3, aligned=al) for (H, W), s, al in zip(MAPS, (0.5, 1.0, 0.125, 0.25), (False, True, True, False))]
ROI_CASES += [_roi("random", H, W, N=2, scale=0.25, P=2, aligned=al, counts=(9, 11)) for (H, W) in MAPS for al in (False, True)]
ROI_CASES += [_roi("adaptive", 32, 32, N=2, scale=0.25, P=2, sr=0, aligned=al, counts=(6, 6)) for al in (False, True)]
ROI_CASES += [_roi("zero_size", 5, 9, N=2, scale=0.5, aligned=True), _roi("zero_size", 32, 32, N=2, scale=0.25, aligned=True)]
ROI_CASES += [_roi("counts", 5, 9, N=5, scale=0.5, counts=ROI_COUNTS, tag="_empty_first"),
              _roi("counts", 5, 9, N=5, scale=0.5, counts=ROI_COUNTS[::-1], tag="_empty_last")]
ROI_FWD_TRIP = _roi("fwd_trip", 16, 20, N=2, C=576, scale=0.25, P=7, counts=(150, 150))      # 300 x 49 x 144 = 2,116,800 > 8192 x 256
ROI_FWD_TRIP_ROWS = (0, 1, 149, 150, 297, 298, 299)                                         # rows 298, 299 lie in the second trip
ROI_BWD_TRIP = _roi("bwd_trip", 128, 132, N=1, C=256, scale=0.25, P=7, counts=(20,))        # 128 x 132 x 64 = 1,081,344 > 4096 x 256


def roi_inputs(case):
    """x (N, H, W, C), rois (R, 5) sorted by image, dout (R, PH, PW, C)"""
    import zlib
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    H, W, s = case.H, case.W, case.scale
    if case.kind == "boundary":
        rois = boundary_rois(H, W, s, case.aligned)[0]
    elif case.kind == "shapes":
        far = [[0, -50.3, -50.2, -40.1, -40.4], [0, W + 20.3, 1.2, W + 30.1, 3.4], [1, 1.3, H + 20.2, 3.1, H + 31.4],
               [1, -30.3, 1.2, -20.1, 3.4]]                                                                              # outside the map
        big = [[0, -4.5 * W, -4.5 * H, 5.5 * W, 5.5 * H], [1, -0.3 * W, -0.2 * H, 9.7 * W, 9.8 * H]]                    # ten times the map
        tiny = [[0, 2.1, 3.2, 2.4, 3.3], [1, 0.3, 0.2, 0.35, 0.9], [1, W - 0.4, H - 0.7, W - 0.2, H - 0.1]]            # under one pixel
        rois = np.asarray(far + big + tiny, F64)
        rois[:, 1:] /= s
        rois = rois[np.argsort(rois[:, 0], kind="stable")]
    elif case.kind == "adaptive":                     # bins of 2 .. 3 pixels: a 3 x 3 grid per bin
        rois = []
        for n, c in enumerate(case.counts):
            while c > 0:
                x1, y1 = rng.uniform(-1.5, W - 8), rng.uniform(-1.5, H - 8)
                w, h = rng.uniform(2.05, 2.95, 2) * case.PW
                roi = np.array([n, x1 / s, y1 / s, (x1 + w) / s, (y1 + h) / s], F32)
                if samples_clear(roi, s, case.PH, case.PW, 0, case.aligned, H, W):
                    rois.append(roi)
                    c -= 1
        rois = np.asarray(rois)
    elif case.kind == "zero_size":                    # zero width, zero height, both; inside, on a border pixel, in the clamp band
        pts = [(2.3, 1.7), (0.6, 0.55), (W - 0.8, H - 0.9), (W - 0.2, 1.1)]
        rois = [[n, x, y, x + dw, y + dh] for n in (0, 1) for x, y in pts for dw, dh in ((0, 1.5), (1.5, 0), (0, 0))]
        rois = np.asarray(rois, F64)
        rois[:, 1:] /= s
    else:
        rois = random_rois(rng, case.counts, H, W, s, case.PH, case.PW, case.sr, case.aligned)
    rois = np.asarray(rois, F32).reshape(-1, 5)
    x = rng.standard_normal((case.N, H, W, case.C)).astype(F32)
    dout = rng.standard_normal((len(rois), case.PH, case.PW, case.C)).astype(F32)
    return x, rois, dout


MlCase = namedtuple("MlCase", "id N H0 W0 C P sr counts levels")
ML_SCALE0 = 0.25
ML_CASES = [MlCase("ml_c4_16x24", 3, 16, 24, 4, 7, 2, (5, 0, 7), "mixed"), MlCase("ml_c8_12x20_level3_1x2", 2, 12, 20, 8, 7, 2, (6, 6), "mixed"),
            MlCase("ml_c260_12x20", 2, 12, 20, 260, 7, 2, (8, 8), "mixed"), MlCase("ml_c1024_8x16", 2, 8, 16, 1024, 7, 2, (0, 10), "mixed"),
            MlCase("ml_c8_16x24_one_level", 2, 16, 24, 8, 3, 2, (4, 5), 1), MlCase("ml_c8_12x20_counts", 5, 12, 20, 8, 2, 2, ROI_COUNTS, "mixed"),
            MlCase("ml_c8_12x20_counts_empty_last", 5, 12, 20, 8, 2, 2, ROI_COUNTS[::-1], "mixed"),
            MlCase("ml_c8_64x72_trip", 1, 64, 72, 8, 7, 2, (12,), 0)]            # 4608 pixels > 1024 blocks x 4: a second trip at level 0


def ml_inputs(case):
    """feats [4] of (N, H0 >> k, W0 >> k, C), rois (R, 5) image-major, level (R,), img_start (N + 1,), dout (R, P, P, C)"""
    import zlib
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    dims = [(case.H0 >> k, case.W0 >> k) for k in range(4)]
    feats = [rng.standard_normal((case.N, h, w, case.C)).astype(F32) for h, w in dims]
    rois, lv = [], []
    for n, c in enumerate(case.counts):
        for _ in range(c):
            k = len(lv) % 4 if case.levels == "mixed" else int(case.levels)
            h, w = dims[k]
            while True:
                one = random_rois(rng, (1,), h, w, ML_SCALE0 / (1 << k), case.P, case.P, case.sr, False)[0]
                if not case.id.endswith("trip"):
                    break
                y1 = rng.uniform(228, 250)            # in the rows the second trip covers (pixels from 4096 on: rows 57 .. 63)
                one[2], one[4] = y1, y1 + rng.uniform(2, 30)
                if samples_clear(one, ML_SCALE0, case.P, case.P, case.sr, False, h, w):
                    break
            one[0] = n
            rois.append(one)
            lv.append(k)
    rois, lv = np.asarray(rois, F32).reshape(-1, 5), np.asarray(lv, np.int32)
    start = np.concatenate([[0], np.cumsum(case.counts)]).astype(np.int32)
    return feats, rois, lv, start, rng.standard_normal((len(rois), case.P, case.P, case.C)).astype(F32)


def ml_reference(case, feats, rois, lv, dout, base, f=F64, loops=False):
    """(out (R, P, P, C), [4] base + gradient maps) level by level: the loops of detection_ref or the restatement in `f`"""
    from oracle import detection_ref
    out = np.zeros(dout.shape, f)
    maps = []
    for k in range(4):
        idx, sc = np.flatnonzero(lv == k), ML_SCALE0 / (1 << k)
        if loops:
            if len(idx):
                out[idx] = detection_ref.roi_align(feats[k], rois[idx], sc, (case.P, case.P), case.sr, False)
            g = detection_ref.roi_align_backward(dout[idx], feats[k].shape, rois[idx], sc, (case.P, case.P), case.sr, False)
            maps.append(np.asarray(base[k], F64) + g)
        else:
            out[idx] = roi_align_np(feats[k], rois[idx], sc, (case.P, case.P), case.sr, False, f)
            maps.append(roi_align_bwd_np(dout[idx], feats[k].shape, rois[idx], sc, case.sr, False, f, base=base[k]))
    return out, maps


# ------------------------------------------------------------------------------------------------------------ E: mask targets
MASK_SHAPE = (3, 12, 16)                             # G, H, W


def mask_inputs():
    """masks (G, H, W) of 0/1: random, stripes two pixels wide, a filled rectangle"""
    G, H, W = MASK_SHAPE
    m = np.zeros(MASK_SHAPE, np.uint8)
    m[0] = np.random.default_rng(31).random((H, W)) < 0.5
    m[1] = ((np.arange(W) // 2) % 2 == 0)[None, :]
    m[2, 3:9, 4:11] = 1
    return m


def mask_exact_rois(P=4):
    """integer-aligned RoIs of P x P bins with bins of 1 and 2 pixels, some past the border: (R, 5) with the instance first"""
    G, H, W = MASK_SHAPE
    rois = [[g, x, y, x + P * b, y + P * b] for g in range(G) for b in (1, 2) for x in range(-2, W - 1, 3) for y in range(-1, H - 1, 3)]
    return np.asarray(rois, F32)


def mask_random_rois(n=40, P=14):
    """n random RoIs none of whose P x P float64 averages lies within 2^-19 of the threshold 0.5"""
    rng = np.random.default_rng(32)
    G, H, W = MASK_SHAPE
    m = mask_inputs().astype(F64)[..., None]
    out = []
    while len(out) < n:
        x1, y1 = rng.uniform(-2, W - 3), rng.uniform(-2, H - 3)
        roi = np.array([rng.integers(0, G), x1, y1, x1 + rng.uniform(0.5, W), y1 + rng.uniform(0.5, H)], F32)
        if np.abs(roi_align_np(m, roi, 1.0, (P, P), 2, False, F64) - 0.5).min() > 2.0 ** -19:
            out.append(roi)
    return np.asarray(out, F32)


def mask_averages(masks, rois, P):
    """float64 RoIAlign (scale 1, 2 x 2 samples, not aligned) of the instance masks: (R, P, P)"""
    from oracle import detection_ref
    return detection_ref.roi_align(masks.astype(F64)[..., None], rois, 1.0, (P, P), 2, False)[..., 0]


# ------------------------------------------------------------------------------------------------------------ tables
def _tables():
    def u(e, w):
        return e / (U24 * max(float(np.abs(w).max()), 1e-300))
    print("A rpn_loss")
    for key in sorted({(c.P, c.A) for c in RPN_CASES}):
        er, dl, cov = {r: 0.0 for r in RANGES}, 0.0, None
        cs = [c for c in RPN_CASES if (c.P, c.A) == key]
        for c in cs:
            head, lab, tg, ns, _, _ = rpn_inputs(c)
            w, e, d = loss_figures(rpn_ref, head, lab, tg, c.A, c.beta, ns)
            er[c.logits] = max(er[c.logits], u(e, w[2]))
            dl = max(dl, d[0] / (U24 * max(1, abs(w[0]))), d[1] / (U24 * max(1, abs(w[1]))))
            if c.logits == "saturated":
                cov = coverage(head[:, :c.A])
        print(f"  P {key[0]} A {key[1]}  {len(cs)}  {cov[0]:.3f}/{cov[1]:.3f}/{cov[2]}/{cov[3]:.1f}  {er['default']:.2f} {er['saturated']:.2f}  {dl:.2f}")
    print("A fastrcnn_loss")
    for key in sorted({(c.R, c.K1) for c in FRC_CASES}):
        er, dl, cov = {r: 0.0 for r in RANGES}, 0.0, None
        cs = [c for c in FRC_CASES if (c.R, c.K1) == key]
        for c in cs:
            head, lab, tg, _, _ = frc_inputs(c)
            w, e, d = loss_figures(frc_ref, head, lab, tg, c.beta)
            er[c.logits] = max(er[c.logits], u(e, w[2]))
            dl = max(dl, d[0] / (U24 * max(1, abs(w[0]))), d[1] / (U24 * max(1, abs(w[1]))))
            if c.logits == "saturated":
                cov = coverage(head[:, :c.K1])
        print(f"  R {key[0]} K1 {key[1]}  {len(cs)}  {cov[0]:.3f}/{cov[1]:.3f}/{cov[2]}/{cov[3]:.1f}  {er['default']:.2f} {er['saturated']:.2f}  {dl:.2f}")
    from oracle import detection_ref
    print("B")
    d = decode_deltas()
    for clip in (None, CLIP):
        e = np.abs(decode32(DECODE_ANCHORS, d, clip) - detection_ref.decode_boxes(DECODE_ANCHORS, d, clip)) / decode_steps(DECODE_ANCHORS, d)
        print("  table", clip, f"{e.max():.2f}")
    d = decode_large_deltas()
    print(f"  large {(np.abs(decode32(DECODE_ANCHORS, d) - detection_ref.decode_boxes(DECODE_ANCHORS, d)) / decode_steps(DECODE_ANCHORS, d)).max():.2f}")
    a, g = roundtrip_boxes()
    t = encode32(a, g)
    print(f"  roundtrip {(np.abs(decode32(a, t) - g.astype(F64)) / decode_steps(a, t)).max():.2f}")
    print("D")
    worst = {}
    for c in ROI_CASES + [ROI_FWD_TRIP, ROI_BWD_TRIP]:
        x, rois, dout = roi_inputs(c)
        a = (c.scale, (c.PH, c.PW), c.sr, c.aligned)
        w, r = roi_align_np(x, rois, *a, f=F64), roi_align_np(x, rois, *a, f=F32)
        wb = roi_align_bwd_np(dout, x.shape, rois, c.scale, c.sr, c.aligned, F64)
        rb = roi_align_bwd_np(dout, x.shape, rois, c.scale, c.sr, c.aligned, F32)
        ef, eb = u(np.abs(r - w).max(), w), u(np.abs(rb - wb).max(), wb)
        worst[c.kind] = tuple(map(max, worst.get(c.kind, (0, 0)), (ef, eb)))
        print(f"  {c.id}  R {len(rois)}  {ef:.2f} {eb:.2f}", flush=True)
    for c in ML_CASES:
        feats, rois, lv, start, dout = ml_inputs(c)
        base = [np.random.default_rng(5 + k).standard_normal(f_.shape).astype(F32) for k, f_ in enumerate(feats)]
        w, wm = ml_reference(c, feats, rois, lv, dout, base, F64)
        r, rm = ml_reference(c, feats, rois, lv, dout, base, F32)
        ef, eb = u(np.abs(r - w).max(), w), max(u(np.abs(rm[k] - wm[k]).max(), wm[k]) for k in range(4))
        worst["ml"] = tuple(map(max, worst.get("ml", (0, 0)), (ef, eb)))
        print(f"  {c.id}  R {len(rois)}  {ef:.2f} {eb:.2f}", flush=True)
    print({k: (round(v[0], 2), round(v[1], 2)) for k, v in worst.items()})


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _tables()
