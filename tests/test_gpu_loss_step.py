"""-m gpu: the kernels every training step ends in, on their own (the tables and float64 references of
tests/loss_step_cases.py; test_loss_step_cases_host.py pins those on the CPU).

test_loss_and_dlogits          loss_reduce / loss_finish / loss_bwd, the focal triple, sigmoid_fwd / sigmoid_bwd: the returned loss
                               and debug_tensor("dlogits") against float64 closed forms evaluated on the logits the device itself
                               produced -- saturated and default logits, all-background / all-RFI / one-pixel label planes, below
                               one wave up to past both grid caps
test_clip_adam                 sumsq / sumsq_finish / adam_kernel on crafted sign-coherent gradients written into the flat buffer
                               through the layout map: the norm, m, v and the update against unet_ref.adam_update in float64,
                               bounded by twice the float32 oracle's own error
test_inactive_clip_is_no_clip  max_grad_norm = 2 x norm gives the bits of max_grad_norm = 0
test_clip_adam_mixed_signs     m0 and p signed independently of g, scale-aware bounds
test_clip_adam_nan             one NaN gradient: everything NaN with the clip active, one element with the clip off
test_padding_stays_zero        after a real backward pass nothing lies outside the named entries of the flat gradient buffer, and
                               after a train_step nothing outside those of the parameter buffer

Lines printed:  LOSSSTEP <case> dloss=... dgrad=... e_ref=...   ADAMSTEP <case> ...   PADDING <model> <mode> ..."""
import ctypes as C
import functools
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

import loss_step_cases as L
from rfi_toolbox_amd import models
from rfi_toolbox_amd._lib import check, lib
from rfi_toolbox_amd.models import SimpleCNN, UNet, UNetOverfit

pytestmark = pytest.mark.gpu


class _OverfitOneLevel(UNetOverfit):
    """UNetOverfit's sigmoid head (and its loss on sigmoid(z)) on a one-level U-Net: 2 x 16 x 16 is then a valid shape"""
    _DEPTH = 1


# ------------------------------------------------------------------------------------------------------------ A
_MODELS, _LOADED = {}, {}


def _loss_model(case):
    if case.model not in _MODELS:
        args = L.MODELS[case.model][0]
        _MODELS[case.model] = {"cnn": lambda: SimpleCNN(*args), "unet_d1": lambda: UNet(*args[:3], depth=args[3]),
                               "overfit": lambda: _OverfitOneLevel(*args[:3])}[case.model]().train()
    m = _MODELS[case.model]
    setup = (case.model, case.shape, case.logits)
    if _LOADED.get(case.model) != setup:
        m.load_state_dict(L.head_state(*setup))
        _LOADED[case.model] = setup
    return m


@functools.lru_cache(maxsize=4)
def _input(model, shape, logits):
    return L.loss_input(model, shape, logits)


@pytest.mark.parametrize("case", L.LOSS_CASES, ids=lambda c: c.id)
def test_loss_and_dlogits(case):
    m = _loss_model(case)
    if case.loss[0] == "focal":
        m.set_loss("focal", alpha=case.loss[1], gamma=case.loss[2])
    else:
        m.set_loss("bce_dice")
    x, y = _input(case.model, case.shape, case.logits), L.labels_of(case)
    loss = m.forward_backward(x, y)
    logits, dlogits = m.debug_tensor("logits"), m.debug_tensor("dlogits")
    assert logits.shape == dlogits.shape == (y.numel(),)
    loss_fwd = m.loss(x, y)
    l64, g64, e_ref, _ = L.loss_figures(case, logits, y.reshape(-1).numpy())
    dloss = abs(loss - l64)
    dgrad = float(np.abs(dlogits.astype(np.float64) - g64).max()) if np.isfinite(dlogits).all() else float("inf")
    lo, hi, near, mx, finite = L.coverage(logits)
    print(f"LOSSSTEP {case.id} dloss={dloss:.2e} ({dloss / (L.U24 * max(1.0, abs(l64))):.2f}u24) dgrad={dgrad:.2e} "
          f"e_ref={e_ref:.2e} bound={L.grad_bound(e_ref, g64):.2e} gmax={np.abs(g64).max():.2e} cover={lo:.2f}/{hi:.2f}/{near}/{mx:.0f}")
    assert finite
    if case.logits == "saturated":                        # the device's own logits reach what the case is for
        assert lo >= 0.10 and hi >= 0.10 and near > 0 and 60 <= mx <= 100, (lo, hi, near, mx)
    assert np.isfinite(dlogits).all()
    assert math.isfinite(loss) and dloss <= L.loss_bound(l64), (loss, l64)
    assert dgrad <= L.grad_bound(e_ref, g64), (dgrad, e_ref)
    assert np.float32(loss_fwd).tobytes() == np.float32(loss).tobytes(), (loss_fwd, loss)


# ------------------------------------------------------------------------------------------------------------ B
LR, BETAS, EPS = L.LR, L.BETAS, L.EPS


def _buffer(m, which):
    p, n = C.c_void_p(), C.c_int64()
    check({"grad": lib.rfi_model_grad_buffer, "param": lib.rfi_model_param_buffer}[which](m._h, C.byref(p), C.byref(n)))
    return p.value, n.value


def _read(m, which):
    p, n = _buffer(m, which)
    h = np.empty(n, np.float32)
    check(lib.rfi_memcpy(m.ctx.handle, h.ctypes.data_as(C.c_void_p), 0, C.c_void_p(p), 1, h.nbytes))
    return h


def _write(m, which, flat):
    p, n = _buffer(m, which)
    flat = np.ascontiguousarray(flat, dtype=np.float32)
    assert flat.shape == (n,)
    check(lib.rfi_memcpy(m.ctx.handle, C.c_void_p(p), 1, flat.ctypes.data_as(C.c_void_p), 0, flat.nbytes))


def _param_names(m):
    return [n for n, _, kind in m._entries if kind in ("conv_w", "conv_b", "bn_g", "bn_b")]


def _layout(m):
    """(name -> flat offsets, padding mask): arange written into the flat gradient buffer, read back entry by entry; the
    buffer is restored afterwards"""
    keep = _read(m, "grad")
    assert keep.size < 2 ** 24                               # every offset is a float32 integer
    _write(m, "grad", np.arange(keep.size, dtype=np.float32))
    gathered = OrderedDict((n, m.grad(n)) for n in _param_names(m))
    _write(m, "grad", keep)
    return L.layout_from_gather(gathered, keep.size)


_ADAM_MODELS = {}


def _adam_model(kind, fresh=False):
    """(model, layout, padding mask), one per kind for the whole file; `fresh`: a model of its own (the NaN rows leave NaN
    in the align4 gaps of the flat buffers, as they do in every parameter)"""
    if fresh or kind not in _ADAM_MODELS:
        a = L.ADAM_MODELS[kind]
        m = UNet(*a[:3], depth=a[3]).train()
        g = torch.Generator().manual_seed(0)
        m.forward_backward(torch.randn(1, 16, 16, a[0], generator=g), torch.zeros(1, 16, 16, dtype=torch.uint8))   # the workspaces
        layout, pad = _layout(m)
        assert list(layout) == list(L.adam_shapes(kind)) and all(layout[n].shape == tuple(s) for n, s in L.adam_shapes(kind).items())
        assert pad.any()                                     # (the stem's fourth input channel, the align4 gaps)
        if fresh:
            return m, layout, pad
        _ADAM_MODELS[kind] = (m, layout, pad)
    return _ADAM_MODELS[kind]


def _run_adam(case, inp, max_norm, fresh=False):
    """load the case into the model, apply once; returns (norm, {"p", "m", "v"} as name -> float32 array, padding of the
    parameter buffer before and after)"""
    m, layout, pad = _adam_model(case.model, fresh)
    m.load_state_dict(inp["p"], strict=False)
    flat = np.zeros(pad.size, np.float32)
    for n in layout:
        m.load_adam_state(n, inp["m"][n].numpy(), inp["v"][n].numpy())
        flat[layout[n]] = inp["g"][n].numpy()
    m.set_adam_step(case.t - 1)
    _write(m, "grad", flat)
    pad_before = _read(m, "param")[pad]
    norm = m.apply_gradients(lr=LR, betas=BETAS, eps=EPS, weight_decay=case.wd, max_grad_norm=max_norm, grad_scale=case.gs)
    pad_after = _read(m, "param")[pad]
    sd = m.state_dict()
    got = {"p": OrderedDict(), "m": OrderedDict(), "v": OrderedDict()}
    for n in layout:
        got["p"][n] = sd[n].numpy()
        got["m"][n], got["v"][n], step = m.adam_state(n)
        assert step == case.t
    return norm, got, pad_before, pad_after


@functools.lru_cache(maxsize=2)
def _adam_refs(cid):
    case = L.ADAM_BY_ID[cid]
    inp = L.adam_inputs(case)
    return inp, L.adam_reference(case, inp, torch.float64), L.adam_reference(case, inp, torch.float32)


def _np32(r):
    return {k: OrderedDict((n, v.numpy()) for n, v in r[k].items()) for k in ("p", "m", "v")}


@pytest.mark.parametrize("case", L.ADAM_CASES, ids=lambda c: c.id)
def test_clip_adam(case):
    inp, r64, r32 = _adam_refs(case.id)
    norm, got, pad0, pad1 = _run_adam(case, inp, L.max_grad_norm(case, inp))
    e32 = L.ulp_errors(_np32(r32), r64, inp["p"])
    bm, bv, bu = L.adam_bounds(e32)
    em, ev, eu, stray = L.ulp_errors(got, r64, inp["p"])
    norm64 = L.grad_norm64(inp, case.gs)
    dnorm = abs(norm - norm64) / norm64
    print(f"ADAMSTEP {case.id} dnorm={dnorm / L.U24:.2f}u24 m={em:.2f} v={ev:.2f} update={eu:.2f} ulp  "
          f"e32={e32[0]:.2f},{e32[1]:.2f},{e32[2]:.2f}  bounds={bm:.2f},{bv:.2f},{bu:.2f} coef={float(r64['coef']):.6g}")
    assert dnorm <= 4 * L.U24, (norm, norm64)
    assert em <= bm and ev <= bv and eu <= bu, (em, ev, eu)
    assert stray == 0                                        # where float64 leaves m, v or p untouched, so does the device
    zero = np.concatenate([z.ravel() for z in inp["zero"].values()])
    for k in ("p", "m", "v"):
        assert not L._cat(got[k])[zero].any(), k             # g = p = m0 = v0 = 0 stays 0, with weight decay too
    assert not pad0.any() and not pad1.any()                 # the padding of the parameter buffer, before and after


@pytest.mark.parametrize("case", [c for c in L.ADAM_CASES if c.clip == "inactive" and c.model == "small"], ids=lambda c: c.id)
def test_inactive_clip_is_no_clip(case):
    inp = L.adam_inputs(case)
    mx = L.max_grad_norm(case, inp)
    norm_a, a, _, _ = _run_adam(case, inp, mx)
    norm_b, b, _, _ = _run_adam(case, inp, 0.0)
    assert mx > norm_a > 0 and np.float32(norm_a).tobytes() == np.float32(norm_b).tobytes()
    for k in ("p", "m", "v"):
        for n in a[k]:
            assert a[k][n].tobytes() == b[k][n].tobytes(), (k, n)


def test_clip_adam_mixed_signs():
    case = L.MIXED_CASE
    inp, r64, _ = _adam_refs(case.id)
    norm, got, pad0, pad1 = _run_adam(case, inp, L.max_grad_norm(case, inp))
    norm64 = L.grad_norm64(inp, case.gs)
    assert abs(norm - norm64) / norm64 <= 4 * L.U24
    for key, bound in zip(("m", "v", "p"), L.mixed_bounds(case, inp, r64)):
        err = np.abs(L._cat(got[key]) - L._cat(r64[key]))
        worst = float((err / np.where(bound > 0, bound, 1.0)).max())
        print(f"ADAMSTEP {case.id} {key} worst error / bound = {worst:.3f}")
        assert (err <= bound).all(), key
    assert not pad0.any() and not pad1.any()


@pytest.mark.parametrize("case", L.NAN_CASES, ids=lambda c: c.id)
def test_clip_adam_nan(case):
    """a value check: the call returns without a HIP error, and the NaN goes where clip_grad_norm_'s default sends it"""
    inp = L.adam_inputs(case)
    name, at = L.NAN_AT
    assert sum(int(torch.isnan(g).sum()) for g in inp["g"].values()) == 1 and bool(torch.isnan(inp["g"][name].reshape(-1)[at]))
    norm, got, _, _ = _run_adam(case, inp, L.max_grad_norm(case, inp), fresh=True)
    assert math.isnan(norm)
    if case.clip == "active":
        assert all(np.isnan(a).all() for a in got["p"].values())
    else:
        for k in ("p", "m", "v"):
            bad = {n: np.flatnonzero(np.isnan(a.ravel())).tolist() for n, a in got[k].items() if np.isnan(a).any()}
            assert bad == {name: [at]}, (k, bad)


# ------------------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("mode", L.PADDING_MODES)
@pytest.mark.parametrize("run", L.PADDING_RUNS, ids=lambda r: f"{r[0]}{'_'.join(map(str, r[1]))}" + ("_d%d" % r[2]["depth"] if r[2] else ""))
def test_padding_stays_zero(run, mode):
    cls, args, kw, (n, h, w) = run
    torch.manual_seed(0)
    m = getattr(models, cls)(*args, **kw).train().set_compute_dtype(mode)
    layout, pad = _layout(m)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, h, w, args[0], generator=g)
    y = (torch.rand(n, h, w, generator=g) > 0.7).to(torch.uint8)
    loss = m.forward_backward(x, y)
    grads = _read(m, "grad")
    named = sum(a.size for a in layout.values())
    assert named + int(pad.sum()) == grads.size and named == m.num_parameters()
    live = sum(1 for a in layout.values() if np.abs(grads[a]).max() > 0)
    bad_g = np.flatnonzero(grads[pad] != 0)
    m.train_step(x, y, lr=1e-3)
    params = _read(m, "param")
    bad_p = np.flatnonzero(params[pad] != 0)
    print(f"PADDING {cls}{args} {mode} n_flat={grads.size} padding={int(pad.sum())} entries_with_gradient={live}/{len(layout)} "
          f"nonzero_padding_grads={bad_g.size} nonzero_padding_params={bad_p.size} loss={loss:.5f}")
    assert math.isfinite(loss) and np.isfinite(grads).all() and live > 0
    assert bad_g.size == 0, (np.flatnonzero(pad)[bad_g][:8], grads[pad][bad_g][:8])
    assert bad_p.size == 0, (np.flatnonzero(pad)[bad_p][:8], params[pad][bad_p][:8])
