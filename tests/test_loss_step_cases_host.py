"""No GPU: pins the tables of tests/loss_step_cases.py and records the float32 CPU oracle's own error.

test_loss_table                   the shapes, labels, losses and ranges the sweep must contain
test_logit_coverage               each saturated setup reaches what it claims on the float32 oracle's logits; default ones stay small
test_closed_forms_against_autograd  the float64 closed forms are finite on every case and equal float64 autograd to 1e-12
                                  wherever autograd is finite; autograd is NOT finite on the saturated gamma < 1 cases
test_autograd_is_not_finite_at_saturation   ... which is why the references are closed forms
test_oracle_loss_error            the float32 oracle's loss and dlogits against float64 on its own logits (prints e_ref)
test_adam_table                   the pairwise cover, the extra rows, the two models
test_adam_case_inputs             sign coherence, no subnormal second moment, the float32 oracle inside the bounds (prints e32)
test_adam_inactive_clip_is_no_clip  max_grad_norm = 2 x norm and 0 give the same bits in the float32 oracle
test_adam_mixed_row               the float32 oracle inside the scale-aware bounds of the mixed-sign row
test_adam_nan_rows_reference      where one NaN gradient goes with the clip active and with the clip off
test_adam_update_is_train_step    adam_update reproduces what train_step computed before it was factored out
test_layout_from_gather           the layout-map helper on a hand-made gather

Lines printed: LOSSSETUP <model> <shape> <range> cover=..., LOSSSTEP <case> dloss=... e_ref=... (host), ADAMSTEP <case> e32=...
"""
import functools
import itertools
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

import loss_step_cases as L
from oracle import unet_ref


# ------------------------------------------------------------------------------------------------------------ A
def test_loss_table():
    ids = [c.id for c in L.LOSS_CASES]
    assert len(set(ids)) == len(ids) == 4 * 2 * 4 * 5 + 4
    small = {(c.model, c.shape) for c in L.LOSS_CASES if c.shape[1] < 100}
    assert small == {("cnn", (1, 5, 7)), ("cnn", (3, 33, 47)), ("unet_d1", (2, 6, 10)), ("overfit", (2, 16, 16))}
    for key in small:                                   # the full cross over the small shapes
        got = {(c.logits, c.labels, c.loss) for c in L.LOSS_CASES if (c.model, c.shape) == key}
        assert got == set(itertools.product(L.RANGES, L.LABELS, L.LOSSES)), key
    assert set(L.LOSSES) == {("bce_dice",), ("focal", 0.25, 2.0), ("focal", -1.0, 1.5), ("focal", 0.6, 0.0), ("focal", -1.0, 0.5)}
    large = [c for c in L.LOSS_CASES if c.shape[1] >= 100]
    assert {(c.shape, c.loss) for c in large} == set(itertools.product(((1, 512, 520), (1, 1024, 1040)), (("bce_dice",), ("focal", 0.25, 2.0))))
    assert all(c.logits == "saturated" and c.labels == "random" and c.model == "cnn" for c in large)
    count = lambda s: s[0] * s[1] * s[2]
    assert count((1, 5, 7)) < 64                                                   # less than one wave
    assert all(count((3, 33, 47)) % d for d in (4, 64, 256))
    assert count((1, 512, 520)) > 1024 * 256 and count((1, 1024, 1040)) > 4096 * 256     # both block caps stride
    for c in L.LOSS_CASES:
        y = L.labels_of(c)
        assert y.shape == c.shape and y.dtype == torch.uint8
        pos = int(y.sum())
        want = {"zeros": 0, "ones": y.numel(), "single": 1}.get(c.labels)
        assert pos == want if want is not None else 0 < pos < y.numel(), c.id
    assert all(s in L.SETUPS for s in {(c.model, c.shape, c.logits) for c in L.LOSS_CASES})


@functools.lru_cache(maxsize=None)
def _logits(model, shape, rng):
    return L.oracle_logits(model, shape, rng)


@pytest.mark.parametrize("setup", sorted(L.SETUPS), ids=lambda s: f"{s[0]}_{'x'.join(map(str, s[1]))}_{s[2]}")
def test_logit_coverage(setup):
    x = _logits(*setup).numpy()
    lo, hi, near, mx, finite = L.coverage(x)
    print(f"LOSSSETUP {setup[0]} {'x'.join(map(str, setup[1]))} {setup[2]} cover={lo:.3f}/{hi:.3f}/{near}/{mx:.1f} seed,k,b={L.SETUPS[setup]}")
    assert finite
    if setup[2] == "saturated":
        assert lo >= 0.10 and hi >= 0.10, (lo, hi)
        assert near > 0
        assert 60 <= mx <= 100, mx
    else:
        assert mx < 10, mx                              # the default init: a few units at most


def _case_data(c):
    return _logits(c.model, c.shape, c.logits), L.labels_of(c).reshape(-1)


@pytest.mark.parametrize("case", L.LOSS_CASES, ids=lambda c: c.id)
def test_closed_forms_against_autograd(case):
    x, t = _case_data(case)
    l64, g64 = L.reference(case, x, t)
    assert math.isfinite(float(l64)) and bool(torch.isfinite(g64).all())
    la, ga = L.autograd(case, x, t, torch.float64)
    ok = torch.isfinite(ga)
    if case.logits == "default" or case.loss[0] == "bce_dice" or case.loss[2] >= 1:
        assert bool(ok.all())
    assert float((ga[ok] - g64[ok]).abs().max()) <= 1e-12
    assert math.isfinite(float(la)) and abs(float(la) - float(l64)) <= 1e-12 * max(1.0, abs(float(l64)))
    # the float32 closed form (what stands in for the oracle where float32 autograd is not finite) is finite too
    assert bool(torch.isfinite(L.reference(case, x, t, torch.float32)[1]).all())


def test_autograd_is_not_finite_at_saturation():
    """the reason for the closed forms: (1 - p_t) ** gamma through autograd at saturated logits, gamma < 1"""
    bad = [c for c in L.LOSS_CASES if c.logits == "saturated" and c.loss[0] == "focal" and 0 < c.loss[2] < 1
           and not bool(torch.isfinite(L.autograd(c, *_case_data(c), torch.float64)[1]).all())]
    assert bad


@pytest.mark.parametrize("case", L.LOSS_CASES, ids=lambda c: c.id)
def test_oracle_loss_error(case):
    x, t = _case_data(case)
    l64, g64, e_ref, dloss = L.loss_figures(case, x, t)
    gmax = float(np.abs(g64).max())
    print(f"LOSSSTEP {case.id} host dloss={dloss / (L.U24 * max(1.0, abs(l64))):.2f}u24 e_ref={e_ref / (L.U24 * gmax):.2f}u24 "
          f"loss64={l64:.6g} gmax={gmax:.3e}")
    assert dloss <= L.loss_bound(l64), (dloss, l64)
    assert gmax > 0


# ------------------------------------------------------------------------------------------------------------ B
def test_adam_table():
    small = [c for c in L.ADAM_CASES if c.model == "small" and c.clip in L.CLIPS]
    assert 12 <= len(small) <= 16
    factors = {"t": L.STEPS, "wd": L.WDS, "gs": L.SCALES, "clip": L.CLIPS}
    assert L.STEPS == (1, 2, 10, 1000, 10 ** 6) and L.WDS == (0.0, 1e-5, 1e-2) and L.SCALES == (1.0, 0.5, 1.0 / 3.0)
    for (fa, va), (fb, vb) in itertools.combinations(factors.items(), 2):
        got = {(getattr(c, fa), getattr(c, fb)) for c in small}
        assert got == set(itertools.product(va, vb)), (fa, fb)
    assert {c.clip for c in L.ADAM_CASES if c.model == "small"} == {"off", "active", "inactive", "below", "above"}
    assert len([c for c in L.ADAM_CASES if c.model == "large"]) == 3
    assert sum(int(np.prod(s)) for s in L.adam_shapes("small").values()) < 10000
    assert sum(int(np.prod(s)) for s in L.adam_shapes("large").values()) > 4 * 262144 + 262144     # past both caps
    assert L.MIXED_CASE.kind == "mixed" and [c.clip for c in L.NAN_CASES] == ["active", "off"]
    assert L.NAN_AT[0] in L.adam_shapes("small")


@functools.lru_cache(maxsize=None)
def _adam(cid):
    case = L.ADAM_BY_ID[cid]
    inp = L.adam_inputs(case)
    return case, inp, L.adam_reference(case, inp, torch.float64), L.adam_reference(case, inp, torch.float32)


# what a float32 evaluation of the documented sequence can lose on sign-coherent inputs, to first order, counted in roundings
# (each at most 2^-24 relative, so at most one ulp of whatever it is measured against):  g' = fma(wd, p, (g gs) coef) with gs
# and wd rounded: 5.  m = fma(w, g' - m0, m0): the terms have one sign, so the error of g' enters with weight w |g'| / |m|
# <= 1: 5, + the difference, w and the fma: 8.  v = fma(c g', g', b2 v0): twice g' (10) + c, c g', b2, b2 v0 and the fma: 15.
# update = (ns m) / (sqrt(v) / bs + eps): m (8) + half of v (7.5) + sqrt, bs, the division, eps, the sum (5) + ns, the
# product, the division (3): 23.5.
E32_CAPS = (8.0, 15.0, 23.5)


@pytest.mark.parametrize("case", L.ADAM_CASES, ids=lambda c: c.id)
def test_adam_case_inputs(case):
    case, inp, r64, r32 = _adam(case.id)
    g, p, m0, v0 = (L._cat(inp[k]) for k in ("g", "p", "m", "v"))
    zero = np.concatenate([z.ravel() for z in inp["zero"].values()])
    # the recipe
    assert np.count_nonzero(g == 0) >= g.size // 17 and (g[zero] == 0).all() and (p[zero] == 0).all()
    assert (m0[zero] == 0).all() and (v0[zero] == 0).all() and zero.sum() >= g.size // 34
    lo, hi = (1e-6, 1e3) if L.clip_is_active(case) else (1e-12, 1e6)
    nzg = np.abs(g[g != 0])
    assert nzg.min() >= lo * 0.999 and nzg.max() <= hi * 1.001 and nzg.min() < lo * 100 and nzg.max() > hi / 100
    if case.t == 1:
        assert not m0.any() and not v0.any()
    else:
        assert (np.abs(m0[g != 0]) >= 0.2499 * nzg).all() and (np.abs(m0[g != 0]) <= 1.7501 * nzg).all()
    # sign coherence: g, p, m0 of one element never have opposite signs; v0 >= 0
    for a, b in ((g, p), (g, m0), (p, m0)):
        assert (a * b >= 0).all()
    assert (v0 >= 0).all()
    # the clip is on the side of max_grad_norm the case names
    norm64, mx = L.grad_norm64(inp, float(np.float32(case.gs))), L.max_grad_norm(case, inp)
    coef = float(r64["coef"])
    if L.clip_is_active(case):
        assert norm64 > mx > 0 and coef < 1
        if case.clip == "below":
            assert 0.98 < coef < 0.995
    else:
        assert coef == 1.0 and (mx == 0 or mx > norm64)
    # no subnormal second moment in the float64 result, every value finite
    v64 = L._cat(r64["v"])
    assert (v64[v64 != 0] >= 2.0 ** -126).all() and np.isfinite(v64).all()
    assert all(np.isfinite(L._cat(r64[k])).all() for k in ("p", "m"))
    # the float32 oracle inside the bounds the device test uses
    f32 = {k: OrderedDict((n, v.numpy()) for n, v in r32[k].items()) for k in ("p", "m", "v")}
    em, ev, eu, stray = L.ulp_errors(f32, r64, inp["p"])
    total32, _ = unet_ref.clip_coefficient(OrderedDict((k, v * torch.tensor(np.float32(case.gs))) for k, v in inp["g"].items()), 1.0)
    dnorm = abs(float(total32) - norm64) / norm64
    print(f"ADAMSTEP {case.id} host e32(m,v,update)={em:.2f},{ev:.2f},{eu:.2f} ulp  dnorm={dnorm / L.U24:.2f}u24 coef={coef:.6g}")
    assert stray == 0
    assert dnorm <= 4 * L.U24
    assert abs(float(r64["norm"]) - norm64) / norm64 <= 4 * L.U24             # the norm formed as the kernel documents it
    assert em <= E32_CAPS[0] and ev <= E32_CAPS[1] and eu <= E32_CAPS[2], (em, ev, eu)
    # elements with nothing in them stay exactly 0
    for k in ("p", "m", "v"):
        assert not L._cat(r64[k])[zero].any() and not L._cat(f32[k])[zero].any()


def test_adam_inactive_clip_is_no_clip():
    """max_grad_norm = 2 x norm and max_grad_norm = 0 give the same float32 oracle result, bit for bit"""
    for case in (c for c in L.ADAM_CASES if c.clip == "inactive" and c.model == "small"):
        _, inp, _, r32 = _adam(case.id)
        off = L.adam_reference(case, inp, torch.float32, max_norm=0.0)
        for k in ("p", "m", "v"):
            for n in off[k]:
                assert torch.equal(off[k][n], r32[k][n]), (case.id, k, n)


def test_adam_mixed_row():
    case, inp, r64, r32 = _adam(L.MIXED_CASE.id)
    g, p, m0 = (L._cat(inp[k]) for k in ("g", "p", "m"))
    assert (g * p < 0).mean() > 0.3 and (g * m0 < 0).mean() > 0.3            # the signs really are mixed
    dm, dv, dp = L.mixed_bounds(case, inp, r64)
    for key, bound in (("m", dm), ("v", dv), ("p", dp)):
        err = np.abs(L._cat(OrderedDict((n, v.numpy()) for n, v in r32[key].items())) - L._cat(r64[key]))
        worst = float((err / np.where(bound > 0, bound, 1.0)).max())
        print(f"ADAMSTEP {case.id} host {key} worst error / bound = {worst:.3f}")
        assert (err <= bound).all(), key


def test_adam_nan_rows_reference():
    """what the device must reproduce: with the clip active one NaN gradient makes the norm and every parameter NaN
    (clip_grad_norm_'s default, error_if_nonfinite=False); with the clip off only that element is"""
    for case in L.NAN_CASES:
        _, inp, _, r32 = _adam(case.id)
        assert math.isnan(float(r32["norm"]))
        bad = sum(int(torch.isnan(v).sum()) for v in r32["p"].values())
        total = sum(v.numel() for v in r32["p"].values())
        if case.clip == "active":
            assert math.isnan(float(r32["coef"])) and bad == total
        else:
            assert bad == 1 and bool(torch.isnan(r32["p"][L.NAN_AT[0]].reshape(-1)[L.NAN_AT[1]]))
            assert all(sum(int(torch.isnan(v).sum()) for v in r32[k].values()) == 1 for k in ("m", "v"))


def test_adam_update_is_train_step():
    """train_step = loss_and_grads + clip_coefficient + adam_update: two steps through train_step equal the same two steps
    assembled by hand, bit for bit"""
    st = unet_ref.init_state(3, 1, 4, 1, seed=0)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 8, 8, generator=g)
    y = (torch.rand(2, 1, 8, 8, generator=g) > 0.7).float()
    a = OrderedDict((k, v.clone()) for k, v in st.items())
    b = OrderedDict((k, v.clone()) for k, v in st.items())
    adam_a, adam_b = unet_ref.new_adam_state(a), unet_ref.new_adam_state(b)
    for _ in range(2):
        unet_ref.train_step(a, adam_a, x, y, lr=1e-3, weight_decay=1e-2)
        _, _, grads, bufs = unet_ref.loss_and_grads(b, x, y)
        _, coef = unet_ref.clip_coefficient(grads, 1.0)
        unet_ref.adam_update(b, adam_b, grads, coef, lr=1e-3, weight_decay=1e-2)
        b.update(bufs)
    assert adam_a["step"] == adam_b["step"] == 2
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for k in adam_a["m"]:
        assert torch.equal(adam_a["m"][k], adam_b["m"][k]) and torch.equal(adam_a["v"][k], adam_b["v"][k]), k


# ------------------------------------------------------------------------------------------------------------ C
def test_layout_from_gather():
    flat = np.arange(12, dtype=np.float32)
    gathered = OrderedDict([("w", flat[[0, 4, 1, 5]].reshape(2, 2)), ("b", flat[8:10])])
    layout, pad = L.layout_from_gather(gathered, 12)
    assert layout["w"].tolist() == [[0, 4], [1, 5]] and layout["b"].tolist() == [8, 9]
    assert np.flatnonzero(pad).tolist() == [2, 3, 6, 7, 10, 11]
    with pytest.raises(AssertionError):
        L.layout_from_gather(OrderedDict([("w", flat[:4]), ("b", flat[3:5])]), 12)
    assert {r[0] for r in L.PADDING_RUNS} == {"UNet", "UNetResNet18", "SimpleCNN"} and len(L.PADDING_RUNS) == 4
    assert L.PADDING_MODES == ("float32", "float32_mfma", "bfloat16")
