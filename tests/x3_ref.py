"""Single-product probes of the float32-by-3xbf16 arithmetic (plain torch, no GPU needed).

The split kernels claim ONE float32 rounding per product.  With dense operands that error hides under the float32
accumulation of K products; with operands built so that every output element is a single product a*b (or an exact zero)
it becomes a per-element bound:  e = max |got - a*b| / |a*b|  in units of 2^-24.  A correct kernel adds six exact piece
products in a float32 accumulator (at most five roundings of partial sums <= |ab|(1 + 2^-8)) and drops products of at most
2^-26 |ab|, so e <= 6; a kernel that loses one piece product lands at 90 or more (test_x3_probes_host.py pins both).

An operation is a bilinear map f(a, b) of two float tensors in the NCHW / OIHW layouts of torch:

    conv-like ops      a = activations (or the output gradient, for the *_dgrad ops), b = filters
    weight gradients   a = the layer input x, b = the output gradient dy

Every probe has two roles: 'b' makes b sparse and a dense, 'a' the reverse.  The dense operand is randn (full 24-bit
significands: its high, middle and low bf16 pieces are all non-zero); so are the non-zero elements of the sparse one
(sharp_randn).
Shapes follow the C ABI: (n, h, w, cin, cout) with h, w the INPUT grid of the layer (the *_dgrad ops of a strided layer
included)."""
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_weight

U = 2.0 ** -24          # the unit of every error figure here

ALL9 = [(r, s) for r in range(3) for s in range(3)]
ALL4 = [(r, s) for r in range(2) for s in range(2)]
PARITIES = [(0, 0), (0, 1), (1, 0), (1, 1)]


class Op:
    """f: the operation on float64 (or float32) torch tensors.  kind 'conv': b is a filter tensor whose axis `out_axis`
    indexes the op's output channels; tap_classes: groups of taps that can meet in ONE output element (the sparse filter
    holds one tap of each group per output channel); lattice: which activation pixels may be non-zero so that the
    receptive field of every output holds at most one of them.  kind 'wgrad': a_classes / b_classes: the pixel parity
    classes of which the sparse operand holds one pixel per channel (one class: any pixel); cover: the largest fraction
    of the reachable outputs a single-product probe of that role can make non-zero (derived per op below)."""

    def __init__(self, name, kind, f, a_shape, b_shape, **kw):
        self.name, self.kind, self.f, self.a_shape, self.b_shape = name, kind, f, a_shape, b_shape
        self.out_axis = kw.get("out_axis", 0)
        self.tap_classes = kw.get("tap_classes")
        self.lattice = kw.get("lattice")
        self.a_classes = kw.get("a_classes", [None])
        self.b_classes = kw.get("b_classes", [None])
        self.cover = kw.get("cover", {"a": 1.0, "b": 1.0})


def _s2_dgrad(k):
    return lambda a, b: F.conv_transpose2d(a, b, stride=2, padding=k // 2, output_padding=1)


# the input gradient of the 3x3 / stride-2 conv: an input pixel of parity (py, px) is reached through the taps r with
# r = 1 (py even) or r in {0, 2} (py odd), the same along x: four groups of taps that never meet in one output
_S2_DGRAD_CLASSES = [[(r, s) for r in rs for s in ss] for rs in ([1], [0, 2]) for ss in ([1], [0, 2])]

OPS = {op.name: op for op in [
    Op("conv3x3", "conv", lambda a, b: F.conv2d(a, b, padding=1),
       lambda n, h, w, ci, co: (n, ci, h, w), lambda ci, co: (co, ci, 3, 3), tap_classes=[ALL9], lattice="mod3"),
    # dx = the 3x3 correlation of dy with the flipped, transposed filters
    Op("conv3x3_dgrad", "conv", lambda a, b: F.conv_transpose2d(a, b, padding=1),
       lambda n, h, w, ci, co: (n, co, h, w), lambda ci, co: (co, ci, 3, 3), out_axis=1, tap_classes=[ALL9], lattice="mod3"),
    Op("conv1x1", "conv", lambda a, b: F.conv2d(a, b),
       lambda n, h, w, ci, co: (n, ci, h, w), lambda ci, co: (co, ci, 1, 1), tap_classes=[[(0, 0)]], lattice="all"),
    # every output pixel (2y + r, 2x + s) reads ONE input pixel through ONE tap: the four taps never meet, the sparse
    # filter holds all four (with a channel of their own each); every input pixel may be non-zero
    Op("convt2x2", "conv", lambda a, b: F.conv_transpose2d(a, b, stride=2),
       lambda n, h, w, ci, co: (n, ci, h, w), lambda ci, co: (ci, co, 2, 2), out_axis=1,
       tap_classes=[[t] for t in ALL4], lattice="all"),
    # dx(y, x) reads the 2 x 2 block of dy under it: one non-zero pixel per block
    Op("convt2x2_dgrad", "conv", lambda a, b: F.conv2d(a, b, stride=2),
       lambda n, h, w, ci, co: (n, co, 2 * h, 2 * w), lambda ci, co: (ci, co, 2, 2), tap_classes=[ALL4], lattice="block2"),
    # rows 2 oy - 1 .. 2 oy + 1: three consecutive rows hold exactly one row of a period-3 lattice
    Op("conv_s2_k3", "conv", lambda a, b: F.conv2d(a, b, stride=2, padding=1),
       lambda n, h, w, ci, co: (n, ci, h, w), lambda ci, co: (co, ci, 3, 3), tap_classes=[ALL9], lattice="mod3"),
    Op("conv_s2_k1", "conv", lambda a, b: F.conv2d(a, b, stride=2),
       lambda n, h, w, ci, co: (n, ci, h, w), lambda ci, co: (co, ci, 1, 1), tap_classes=[[(0, 0)]], lattice="all"),
    # dx(y, x) of the strided 3x3 reads dy rows {y/2} (y even) or {(y-1)/2, (y+1)/2} (y odd): windows of up to 2 x 2
    # ADJACENT pixels, so at most one pixel in four may be non-zero -- (even, even) outputs then see one with probability
    # 1/4, (even, odd) and (odd, even) 1/2, (odd, odd) 1: no lattice covers more than 9/16 of the outputs
    Op("conv_s2_k3_dgrad", "conv", _s2_dgrad(3),
       lambda n, h, w, ci, co: (n, co, h // 2, w // 2), lambda ci, co: (co, ci, 3, 3), out_axis=1,
       tap_classes=_S2_DGRAD_CLASSES, lattice="even", cover={"a": 9 / 16, "b": 1.0}),
    Op("conv_s2_k1_dgrad", "conv", _s2_dgrad(1),
       lambda n, h, w, ci, co: (n, co, h // 2, w // 2), lambda ci, co: (co, ci, 1, 1), out_axis=1,
       tap_classes=[[(0, 0)]], lattice="all"),
    # ---- weight gradients: f(x, dy)
    Op("conv3x3_wgrad", "wgrad", lambda a, b: conv2d_weight(a, (b.shape[1], a.shape[1], 3, 3), b, padding=1),
       lambda n, h, w, ci, co: (n, ci, h, w), lambda n, h, w, ci, co: (n, co, h, w)),
    # dW[ci, co, r, s] = sum x[y, x] dy[2y + r, 2x + s]: a dy pixel feeds the ONE tap of its parity, so the sparse dy
    # holds a pixel of each parity per channel
    Op("convt2x2_wgrad", "wgrad", lambda a, b: conv2d_weight(b, (a.shape[1], b.shape[1], 2, 2), a, stride=2),
       lambda n, h, w, ci, co: (n, ci, h, w), lambda n, h, w, ci, co: (n, co, 2 * h, 2 * w), b_classes=PARITIES),
    # dW[co, ci, r, s] = sum dy[oy, ox] x[2 oy + r - 1, 2 ox + s - 1]: an x pixel feeds the taps of its parity class
    # (r = 1 for even y, r in {0, 2} for odd y -- the latter two at different oy), so the sparse x holds one of each
    Op("conv_s2_k3_wgrad", "wgrad", lambda a, b: conv2d_weight(a, (b.shape[1], a.shape[1], 3, 3), b, stride=2, padding=1),
       lambda n, h, w, ci, co: (n, ci, h, w), lambda n, h, w, ci, co: (n, co, h // 2, w // 2), a_classes=PARITIES),
    Op("conv_s2_k1_wgrad", "wgrad", lambda a, b: conv2d_weight(a, (b.shape[1], a.shape[1], 1, 1), b, stride=2),
       lambda n, h, w, ci, co: (n, ci, h, w), lambda n, h, w, ci, co: (n, co, h // 2, w // 2), a_classes=[(0, 0)]),
]}


def shapes(op, n, h, w, cin, cout):
    a = op.a_shape(n, h, w, cin, cout)
    b = op.b_shape(cin, cout) if op.kind == "conv" else op.b_shape(n, h, w, cin, cout)
    return tuple(a), tuple(b)


# ------------------------------------------------------------------ builders
def sharp_randn(shape, g, k=8):
    """randn values for the few non-zeros of a sparse operand: of k draws per element, the one whose middle AND low
    bf16 pieces are largest against the value, so that a probe with a handful of non-zeros (the four channels of a stem)
    still shows a lost piece product at full size.  A correct kernel is indifferent to the choice."""
    v = torch.randn((k,) + tuple(shape), generator=g)
    h = v.to(torch.bfloat16).float()
    m = (v - h).to(torch.bfloat16).float()
    lo = (v - h - m).to(torch.bfloat16).float()
    score = torch.minimum((m / v).abs() * 2.0 ** 8, (lo / v).abs() * 2.0 ** 16)
    return torch.gather(v, 0, score.argmax(0, keepdim=True))[0]


def sparse_filter(op, bshape, g):
    """one non-zero (reduction channel, tap) per output channel and tap class; the channel walks over every residue
    mod 16 (every k-slot of the K = 16 MFMA), the tap over every tap of its class"""
    oa = op.out_axis
    nout, nred = bshape[oa], bshape[1 - oa]
    dense = sharp_randn(bshape, g)
    wt = torch.zeros(bshape)
    for o in range(nout):
        for ci, cls in enumerate(op.tap_classes):
            r, s = cls[(o + o // len(cls)) % len(cls)]
            c = (o + 5 * ci + o // nred) % nred
            idx = (o, c, r, s) if oa == 0 else (c, o, r, s)
            wt[idx] = dense[idx]
    return wt


def _lattice_mask(kind, n, h, w):
    ys, xs = torch.arange(h)[:, None], torch.arange(w)[None, :]
    if kind == "all":
        m = torch.ones(h, w, dtype=torch.bool)
    elif kind == "mod3":           # every third row / column, phased so that the last window of a 3x3 conv holds one too
        m = (ys % 3 == (0 if h % 3 == 1 else 1)) & (xs % 3 == (0 if w % 3 == 1 else 1))
    elif kind == "even":
        m = (ys % 2 == 0) & (xs % 2 == 0)
    else:
        assert kind == "block2"
        m = None
    if m is not None:
        return m[None].expand(n, h, w).clone()
    sel = (3 * (ys // 2) + (xs // 2) + torch.arange(n)[:, None, None]) % 4      # which pixel of the block, varying
    return ((ys % 2)[None] == sel // 2) & ((xs % 2)[None] == sel % 2)


def sparse_activation(op, ashape, g):
    """non-zero at ONE channel per lattice pixel, the channel varying with the pixel"""
    n, c, h, w = ashape
    mask = _lattice_mask(op.lattice, n, h, w)
    k = torch.cumsum(mask.flatten(), 0).reshape(n, h, w) - 1
    ch = (k + k // c) % c
    a = torch.zeros(n, h, w, c)
    vals = sharp_randn((n, h, w), g)
    a[mask, ch[mask]] = vals[mask]
    return a.permute(0, 3, 1, 2).contiguous()


def sparse_pixels(shape, classes, g):
    """one non-zero pixel per channel and parity class, spread evenly over the images (hence over the tiles and the
    split-K slabs of a launch).  Every fourth channel takes the pixel the stride gives it, on the image border where
    that falls (taps that leave the image: exact zeros): channel 0 sits in the first corner of the first image, and
    with 32 channels or more the last channel in the last corner of the last one (the ragged last tile).  The others are
    interior pixels, so that the probe keeps its coverage on small images, which are mostly border."""
    n, c, h, w = shape
    t = torch.zeros(n, h, w, c)
    vals = sharp_randn((len(classes), c), g)
    ys, xs = torch.arange(h)[:, None].expand(h, w), torch.arange(w)[None, :].expand(h, w)
    inner = (ys > 0) & (ys < h - 1) & (xs > 0) & (xs < w - 1)
    for k, cls in enumerate(classes):
        ok = torch.ones(h, w, dtype=torch.bool) if cls is None else (ys % 2 == cls[0]) & (xs % 2 == cls[1])
        flat = lambda m: torch.nonzero(m[None].expand(n, h, w).flatten()).flatten()      # flat pixel indices
        every, interior = flat(ok), flat(ok & inner)
        for ch in range(c):
            cand = every if ch % 4 == 0 and c >= 8 else interior
            m = len(cand)
            i = (ch * m // c + (ch * 37) % 11 + 5 * k) % m
            if c >= 32 and ch == c - 1:
                cand, i = every, len(every) - 1
            p = int(cand[i])
            t[p // (h * w), (p // w) % h, p % w, ch] = vals[k, ch]
    return t.permute(0, 3, 1, 2).contiguous()


def pow2_transform(c, g, sparse, relu):
    """a BatchNorm-like load transform whose scales are signed powers of two: x * scale is exact, so
    relu(x * scale + shift) in float32 is the same with or without fma.  Dense operand: shifts around +2 |scale|, so that
    the ReLU removes part of the elements (about one in thirty) and the probe keeps its coverage.  Sparse operand: shifts
    <= 0 (zero without the ReLU), so that its zeros stay zero; non-zero in one channel of eight, where the ReLU then removes
    the elements below a quarter."""
    e = torch.randint(-3, 4, (c,), generator=g).float()
    sign = torch.where(torch.rand(c, generator=g) < 0.3, -1.0, 1.0)
    scale = sign * torch.pow(torch.tensor(2.0), e)
    if not sparse:
        shift = scale.abs() * (2.0 + 0.5 * torch.randn(c, generator=g))
    elif relu:
        shift = torch.zeros(c)
        shift[3::8] = -0.25 * scale.abs()[3::8]
    else:
        shift = torch.zeros(c)
    return scale, shift


def apply_transform(a, scale, shift, relu):
    t = a * scale[None, :, None, None] + shift[None, :, None, None]       # float32, as the kernels evaluate it
    return torch.relu(t) if relu else t


def build_probe(op, role, n, h, w, cin, cout, g, relu=None):
    """(a, b, a_eff, scale, shift): the operands as the device gets them and the a operand behind the load transform
    (a itself, and no scale / shift, without one).  relu: None (no transform), False (scale and shift), True (+ ReLU)."""
    ash, bsh = shapes(op, n, h, w, cin, cout)
    if op.kind == "conv":
        a = torch.randn(ash, generator=g) if role == "b" else sparse_activation(op, ash, g)
        b = sparse_filter(op, bsh, g) if role == "b" else torch.randn(bsh, generator=g)
    else:
        a = torch.randn(ash, generator=g) if role == "b" else sparse_pixels(ash, op.a_classes, g)
        b = sparse_pixels(bsh, op.b_classes, g) if role == "b" else torch.randn(bsh, generator=g)
    if relu is None:
        return a, b, a, None, None
    scale, shift = pow2_transform(ash[1], g, role == "a", relu)
    if role == "a" and relu:       # most non-zeros on the side of the ReLU that passes (negative scales: negative values)
        order = torch.cumsum((a != 0).flatten(), 0).reshape(ash)
        keep = torch.where(order % 32 == 7, -1.0, 1.0)                  # ... and one non-zero in 32 on the other side
        a = a.abs() * keep * torch.sign(scale)[None, :, None, None]
    return a, b, apply_transform(a, scale, shift, relu), scale, shift


# ------------------------------------------------------------------ the statistic
def exact(op, a, b):
    """(want, bound) = (f(a, b), f(|a|, |b|)) in float64"""
    a, b = a.double(), b.double()
    return op.f(a, b), op.f(a.abs(), b.abs())


def products_per_output(op, a, b):
    """how many non-zero products meet in each output: the operation on the non-zero masks"""
    return op.f((a != 0).double(), (b != 0).double())


def probe_error(got, want, bound):
    """(e in units of 2^-24 over outputs with bound > 0, all outputs with bound == 0 are exactly 0.0, index of the worst)"""
    got = torch.as_tensor(got).double()
    nz = bound > 0
    zeros_ok = bool((got[~nz] == 0).all())
    rel = torch.where(nz, (got - want).abs() / torch.where(nz, bound, torch.ones_like(bound)), torch.zeros_like(bound))
    worst = tuple(int(i) for i in torch.nonzero(rel == rel.max())[0]) if rel.numel() else ()
    return float(rel.max()) / U, zeros_ok, worst


def coverage(op, a, b, bound):
    """non-zero outputs as a fraction of the outputs ANY operands can reach (a strided input gradient of a 1x1 filter
    never writes the odd pixels)"""
    reach = op.f(torch.ones_like(a, dtype=torch.float64), torch.ones_like(b, dtype=torch.float64)) > 0
    return float((bound > 0).sum()) / float(reach.sum())


def dense_error(got, want, bound):
    """max |got - want| / sum |a||b| in units of 2^-24 (outputs no product reaches must be exact zeros)"""
    got = torch.as_tensor(got).double()
    nz = bound > 0
    assert bool((got[~nz] == 0).all())
    return float(((got - want).abs()[nz] / bound[nz]).max()) / U


# ------------------------------------------------------------------ the emulation of the scheme
def split3(t):
    """float32 -> its three bf16 pieces (round to nearest even; the residuals are exact in float32), as float64"""
    t = t.float()
    h = t.to(torch.bfloat16).float()
    m = (t - h).to(torch.bfloat16).float()
    lo = (t - h - m).to(torch.bfloat16).float()
    return h.double(), m.double(), lo.double()


SIX = [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)]           # (piece of a, piece of b): every product down to 2^-16
VARIANTS = {
    "six": SIX,
    "no_al_bh": [p for p in SIX if p != (2, 0)],
    "no_ah_bl": [p for p in SIX if p != (0, 2)],
    "no_am_bm": [p for p in SIX if p != (1, 1)],
    "two_pieces": [(0, 0), (0, 1), (1, 0), (1, 1)],              # 4 MFMAs instead of 6
}


def emulate(op, a, b, variant="six"):
    """the scheme on the CPU: float64 sum of the chosen exact piece products, rounded once to float32"""
    pa, pb = split3(a), split3(b)
    acc = None
    for i, j in VARIANTS[variant]:
        t = op.f(pa[i], pb[j])
        acc = t if acc is None else acc + t
    return acc.float()


# ------------------------------------------------------------------ dense operands for the accumulation
def wide(shape, g, lo=-20, hi=20):
    """randn scaled by 2^k, k uniform in [lo, hi]"""
    k = torch.randint(lo, hi + 1, shape, generator=g).double()
    return (torch.randn(shape, generator=g).double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), k)).float()


def build_dense(op, style, n, h, w, cin, cout, g):
    """dense operands: 'randn' (the filter scaled like an initialised layer), or 'wide': exponents spread over
    2^-20 .. 2^20 and, for the first quarter of the output channels, pairs of terms that cancel exactly (conv-like ops:
    channel pairs with equal activations and opposite filters; weight gradients: image pairs with equal x, opposite dy)"""
    ash, bsh = shapes(op, n, h, w, cin, cout)
    if style == "randn":
        a, b = torch.randn(ash, generator=g), torch.randn(bsh, generator=g)
        if op.kind == "conv":
            b = b / (bsh[2] * bsh[1 - op.out_axis] ** 0.5)
        return a, b
    a, b = wide(ash, g), wide(bsh, g)
    if op.kind == "conv":
        nred = ash[1] // 2 * 2
        q = max(1, bsh[op.out_axis] // 4)
        a[:, 1:nred:2] = a[:, 0:nred:2]
        if op.out_axis == 0:
            b[:q, 1:nred:2] = -b[:q, 0:nred:2]
        else:
            b[1:nred:2, :q] = -b[0:nred:2, :q]
    else:
        npair = ash[0] // 2 * 2
        q = max(1, bsh[1] // 4)
        a[1:npair:2] = a[0:npair:2]
        b[1:npair:2, :q] = -b[0:npair:2, :q]
    return a, b
