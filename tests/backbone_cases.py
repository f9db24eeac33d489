"""The oracle harness of the ResNet-50-FPN backbone tests (CPU only; tests/test_backbone_cases_host.py proves it, tests/
test_gpu_backbone.py uses it).

A recording run of oracle/backbone_ref.py (float32 or float64) collects every tensor the device exposes through
``debug_tensor`` -- each Conv2d output ("conv.<i>", state-dict order of the conv weights), the pooled stem ("pool"), each
Bottleneck output ("block.<b>"), the merged FPN maps ("merged.<i>") -- the five pyramid levels ("feat.<i>"), the 49 ReLU
inputs in call order (1 stem + 16 blocks x 3) and every parameter gradient, plus the gradient of the merged maps
("dmerged.<i>").

The MASKED oracle is the same module with every ReLU replaced by ``z * mask_k``, the masks given in call order.  With
the masks fixed the backward pass is one linear map, so two implementations that use the same masks differ by rounding
only: a ReLU input within rounding of 0 can no longer take the other branch in one of them and move every gradient
computed after it by one element's share.  ``masks_from_device`` reads the masks off the device's own forward tensors.
"""
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from oracle import backbone_ref as bref

EPS = 2.0 ** -24                      # half a unit in the last place of float32, relative
N_RELU = 49                           # 1 stem + 16 Bottlenecks x (bn1, bn2, block output)
BLOCKS = (3, 4, 6, 3)

Case = namedtuple("Case", "id mode cin w f n h wd seed")


# (C_in, base width, FPN channels, N, H, W).  The seeds are those at which the device's forward pass leaves no undecided
# ReLU input and no undecided pooling window (a condition on the inputs: masks_from_tensors)
CASES = [
    Case("c3_w8_2x64x64", "float32", 3, 8, 16, 2, 64, 64, 11),              # the smallest
    Case("c3_w8_1x64x128", "float32", 3, 8, 16, 1, 64, 128, 11),            # H != W ...
    Case("c3_w8_1x128x64", "float32", 3, 8, 16, 1, 128, 64, 11),            # ... both ways round
    Case("c1_w8_3x64x64", "float32", 1, 8, 16, 3, 64, 64, 11),              # stem K 49 -> 64; 48 pixels on the 4x4 level: not flattened there
    Case("c8_w4_2x64x64", "float32", 8, 4, 8, 2, 64, 64, 11),               # stem K 392 -> 400, the minimum width
    Case("c3_w16_2x128x128", "float32", 3, 16, 32, 2, 128, 128, 11),        # 32-wide maps, not flattened
    Case("c3_w64_1x128x128", "float32", 3, 64, 256, 1, 128, 128, 11),       # the real widths
    Case("mfma_c3_w8_2x64x64", "float32_mfma", 3, 8, 16, 2, 64, 64, 11),
]
BY_ID = {c.id: c for c in CASES}
HOST_CASE = Case("host_c3_w4_1x64x128", "float32", 3, 4, 8, 1, 64, 128, 11)   # (non-square: a transposed tensor is a different tensor)


def case_inputs(c):
    return inputs(c.cin, c.w, c.f, c.n, c.h, c.wd, c.seed)


def _state(cin, w, f, seed):
    """Default conv init with non-trivial frozen BatchNorm buffers (every term of the affine matters)."""
    st = bref.init_state(cin, w, f, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k in st:
        if k.endswith("running_mean"):
            st[k] = 0.1 * torch.randn(st[k].shape, generator=g)
        elif k.endswith("running_var"):
            st[k] = 0.5 + torch.rand(st[k].shape, generator=g)
        elif ".bn" in k or "downsample.1" in k:
            st[k] = (1 + 0.2 * torch.randn(st[k].shape, generator=g)) if k.endswith("weight") else 0.1 * torch.randn(st[k].shape, generator=g)
    return st


def inputs(cin, w, f, n, h, wd, seed):
    """(state, x NHWC, [d(loss)/d(P_i)] NHWC) of a case, all float32 torch tensors."""
    st = _state(cin, w, f, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(n, h, wd, cin, generator=g)
    dfe = []
    for i in range(5):
        hh, ww = h >> (2 + i), wd >> (2 + i)
        dfe.append(torch.randn(n, hh, ww, f, generator=g) / (hh * ww * f) ** 0.5)
    return st, x, dfe


def conv_names(st):
    """Conv layers in state-dict order of their weights: the device's ``conv.<i>`` / ``chan.<i>`` index."""
    return [k[:-len(".weight")] for k, v in st.items() if k.endswith(".weight") and v.ndim == 4]


def relu_sources(names):
    """For each of the 49 ReLUs in call order: ("conv", i) -- the affine of conv i's output -- or ("block", b)."""
    idx = {k: i for i, k in enumerate(names)}
    src = [("conv", idx["body.conv1"])]
    b = 0
    for s, nb in enumerate(BLOCKS):
        for j in range(nb):
            p = f"body.layer{s + 1}.{j}"
            src += [("conv", idx[p + ".conv1"]), ("conv", idx[p + ".conv2"]), ("block", b)]
            b += 1
    assert len(src) == N_RELU
    return src


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()


class _Functional:
    """Stands in for ``backbone_ref.F`` during one run: ``relu`` records its input and applies the given mask."""

    def __init__(self, masks, relu_in):
        self.masks, self.relu_in = masks, relu_in

    def relu(self, z):
        k = len(self.relu_in)
        self.relu_in.append(z.detach())
        if self.masks is None:
            return torch.nn.functional.relu(z)
        m = self.masks[k]
        assert m.shape == z.shape, (k, tuple(m.shape), tuple(z.shape))
        return z * m.to(z.dtype)

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)


Run = namedtuple("Run", "tensors grads relu_in hooked")


def run_oracle(st, x, dfe, dtype=torch.float64, masks=None):
    """One forward + backward pass of the oracle module in `dtype` (x, dfe: NHWC float32).  `masks`: 49 NCHW tensors (any
    dtype, non-zero = pass) for the masked oracle, None for the plain one.  ``backbone_ref.F`` is replaced for the duration of
    the call by a stand-in whose ``relu`` records its input and applies the mask.  -> Run: NHWC NumPy `tensors` by device
    name, `grads` by parameter name (+ "dmerged.<i>"), the ReLU inputs (NCHW torch), and the hooked conv names."""
    mod = bref.ResNet50FPN(x.shape[-1], st["body.conv1.weight"].shape[0], st["fpn.inner_blocks.0.0.weight"].shape[0]).to(dtype)
    mod.load_state_dict(OrderedDict((k, v.to(dtype)) for k, v in st.items()))
    t, hooked, merged, relu_in = {}, [], [None] * 4, []
    handles = []
    for name, sub in mod.named_modules():
        if isinstance(sub, torch.nn.Conv2d):
            i = len(hooked)
            hooked.append(name)
            handles.append(sub.register_forward_hook(lambda m, a, out, i=i: t.__setitem__(f"conv.{i}", out)))
    nblk = 0
    for s in range(4):
        for blk in getattr(mod.body, f"layer{s + 1}"):
            handles.append(blk.register_forward_hook(lambda m, a, out, b=nblk: t.__setitem__(f"block.{b}", out)))
            nblk += 1
    handles.append(mod.body.layer1.register_forward_pre_hook(lambda m, a: t.__setitem__("pool", a[0])))
    for i in range(4):
        handles.append(mod.fpn.layer_blocks[i].register_forward_pre_hook(lambda m, a, i=i: merged.__setitem__(i, a[0])))
    names = [k for k, _ in mod.named_parameters()]
    params = [p for _, p in mod.named_parameters()]
    keep = bref.F
    bref.F = _Functional(None if masks is None else list(masks), relu_in)
    try:
        feats = mod(_nchw(x.numpy()).to(dtype))
    finally:
        bref.F = keep
        for hd in handles:
            hd.remove()
    assert len(relu_in) == N_RELU, len(relu_in)
    loss = sum((p * _nchw(d.numpy()).to(dtype)).sum() for p, d in zip(feats, dfe))
    g = torch.autograd.grad(loss, params + merged)
    tensors = {k: _nhwc(v) for k, v in t.items()}
    for i in range(4):
        tensors[f"merged.{i}"] = _nhwc(merged[i])
    for i in range(5):
        tensors[f"feat.{i}"] = _nhwc(feats[i])
    grads = OrderedDict((k, v.numpy()) for k, v in zip(names, g[:len(names)]))
    for i in range(4):
        grads[f"dmerged.{i}"] = _nhwc(g[len(names) + i])
    return Run(tensors, grads, relu_in, hooked)


def own_masks(run):
    return [z > 0 for z in run.relu_in]


DeviceMasks = namedtuple("DeviceMasks", "masks undecided undecided_windows")


def masks_from_tensors(get, names, n, h, w):
    """The 49 masks from forward tensors only.  `get(name)` returns the flat float32 tensor ``conv.<i>`` / ``chan.<i>`` /
    ``block.<b>``.  Block outputs: ``block.<b> > 0``.  Stem, conv1, conv2: ``Y * scale + shift > 0`` in float32 (two roundings,
    as the kernels compute it).  undecided: elements with |Y scale + shift| <= 4 * 2^-24 (|Y scale| + |shift|), which a fused
    multiply-add could decide the other way.  undecided_windows: 3x3/2 max-pool windows of the activated stem whose two
    largest values at different positions are positive and closer than 4 * 2^-24 relative (all-zero windows: both sides
    take the first position)."""
    masks, undecided, windows = [], 0, 0
    for kind, i in relu_sources(names):
        if kind == "block":
            a = np.asarray(get(f"block.{i}"), np.float32)
            lvl = _block_level(i)
            z = a.reshape(n, h >> lvl, w >> lvl, -1)
            masks.append(_nchw(z > 0))
            continue
        ch = np.asarray(get(f"chan.{i}"), np.float32)
        cout = ch.size // 8
        scale, shift = ch[4 * cout:5 * cout], ch[5 * cout:6 * cout]
        y = np.asarray(get(f"conv.{i}"), np.float32).reshape(-1, cout)
        ys = y * scale
        z = ys + shift
        undecided += int((np.abs(z) <= np.float32(4 * EPS) * (np.abs(ys) + np.abs(shift))).sum())
        px = y.shape[0] // n
        lvl = _level_of_pixels(px, h, w)
        z = z.reshape(n, h >> lvl, w >> lvl, cout)
        masks.append(_nchw(z > 0))
        if i == 0:
            windows = undecided_pool_windows(np.maximum(z, 0))
    return DeviceMasks(masks, undecided, windows)


def masks_from_device(model, names, n, h, w):
    return masks_from_tensors(model.debug_tensor, names, n, h, w)


def _block_level(b):
    edges = np.cumsum(BLOCKS)
    return 2 + int(np.searchsorted(edges, b, side="right"))


def _level_of_pixels(px, h, w):
    for lvl in range(1, 7):
        if (h >> lvl) * (w >> lvl) == px:
            return lvl
    raise ValueError(px)


def undecided_pool_windows(a):
    """a: the activated stem, NHWC, >= 0."""
    t = torch.nn.functional.pad(_nchw(np.asarray(a, np.float32)).double(), (1, 1, 1, 1), value=-1.0)
    n, c = t.shape[:2]
    win = torch.nn.functional.unfold(t, 3, stride=2).reshape(n, c, 9, -1)
    top = win.topk(2, dim=2).values
    v1, v2 = top[:, :, 0], top[:, :, 1]
    return int(((v2 > 0) & (v1 - v2 <= 4 * EPS * v1)).sum())


# ---------------------------------------------------------------------------------------------------------- the checkers
def check_forward(hip, f32, f64, bound=None):
    """Per tensor t: e_hip = max|hip - f64| against e_ref = max(max|f32 - f64|, 2^-24 max|f64|).  -> (worst e_hip / e_ref, its
    name); with `bound`, asserts every ratio <= bound.  `hip` may hold flat arrays; every tensor of `f64` must be there."""
    worst = (0.0, None)
    for k, w64 in f64.items():
        w64 = np.asarray(w64, np.float64).ravel()
        got = np.asarray(hip[k], np.float64).ravel()
        assert got.size == w64.size, (k, got.size, w64.size)
        assert np.isfinite(got).all(), k
        e_hip = np.abs(got - w64).max()
        e_ref = max(np.abs(np.asarray(f32[k], np.float64).ravel() - w64).max(), EPS * np.abs(w64).max())
        r = e_hip / e_ref
        if bound is not None:
            assert r <= bound, (k, r, e_hip, e_ref)
        worst = max(worst, (r, k))
    return worst


def check_gradients(hip, g32, g64, bound=None):
    """Per gradient k: rel_hip = |hip - g64| / |g64| against rel_ref = |g32 - g64| / |g64| (2-norms; g32 and g64 from the
    masked oracles with the same masks).  -> (worst rel_hip / rel_ref, its name); with `bound`, asserts every ratio."""
    worst = (0.0, None)
    for k, w64 in g64.items():
        w64 = np.asarray(w64, np.float64).ravel()
        got = np.asarray(hip[k], np.float64).ravel()
        assert got.size == w64.size, (k, got.size, w64.size)
        assert np.isfinite(got).all(), k
        nrm = np.linalg.norm(w64) + 1e-30
        rel_ref = np.linalg.norm(np.asarray(g32[k], np.float64).ravel() - w64) / nrm
        rel_hip = np.linalg.norm(got - w64) / nrm
        r = rel_hip / rel_ref if rel_ref > 0 else (0.0 if rel_hip == 0 else np.inf)
        if bound is not None:
            assert r <= bound, (k, r, rel_hip, rel_ref)
        worst = max(worst, (r, k))
    return worst
