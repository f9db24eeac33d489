"""-m gpu: the plain U-Net away from the benched configuration -- the channel counts, depths, shapes and compute modes of
tests/unet_cases.py, each against the CPU oracle (oracle/unet_ref.py) with the criteria the project already uses at its
flagship width (test_flagship_width_vs_oracle, test_bench_configuration_step_vs_oracle, test_three_steps_golden_f4).

test_training_case_float32      every training case x {float32, float32_mfma, float32_planes}: eval forward, loss, logits,
                                every gradient against float64 next to the float32 oracle's own error, BatchNorm buffers,
                                gradient norm and post-step eval logits
test_training_case_bf16_regs    ... x bfloat16_regs, against the oracle in the same arithmetic
test_out_channels_forward       out_channels 2, 3, 8, 12: train- and eval-mode forward through both entry points
test_intended_kernels_ran       the context profile of one forward + backward pass shows the kernels the gates predict
test_one_model_several_shapes   one model through five shapes: bit-equal to a fresh model per step, and inside the criteria

Each case and mode prints one line:  UNETCFG <id> <mode> dlogit=... ratio_max=... ratio_med=... worst=<tensor>"""
import functools
import os
import tempfile
from collections import OrderedDict

import numpy as np
import pytest
import torch

import unet_cases as U
from oracle import unet_ref
from rfi_toolbox_amd.models import UNet
from rfi_toolbox_amd.runtime import Context

pytestmark = pytest.mark.gpu

LR, WD = 1e-4, 1e-5
FLOAT32_MODES = ("float32", "float32_mfma", "float32_planes")


def _clone(st):
    return OrderedDict((k, v.clone()) for k, v in st.items())


def _flat(logits_nchw):
    return logits_nchw.permute(0, 2, 3, 1).reshape(-1).numpy()


@functools.lru_cache(maxsize=None)
def _oracle(cid):
    """everything the oracle says about a training case, computed once"""
    c = U.BY_ID[cid]
    st = unet_ref.init_state(c.in_ch, c.out_ch, c.feat, c.depth, seed=c.seed)
    x, y = U.inputs(c)
    xo, yo = unet_ref.nhwc_to_nchw(x), y.float().unsqueeze(1)
    o = {"state": st, "x": x, "y": y}
    _, _, o["g64"], _ = unet_ref.loss_and_grads(U.to64(st), xo.double(), yo.double())
    with torch.no_grad():
        o["eval0"] = unet_ref.forward(st, xo, training=False)
    ost = _clone(st)
    o["step"] = unet_ref.train_step(ost, unet_ref.new_adam_state(ost), xo, yo, lr=LR, weight_decay=WD)
    o["state1"] = ost
    with torch.no_grad():
        o["eval1"] = unet_ref.forward(ost, xo, training=False)
    return o


@functools.lru_cache(maxsize=None)
def _oracle_bf16(cid):
    """(loss, logits, gradients) of the oracle with the operands of every contraction rounded to bfloat16"""
    o = _oracle(cid)
    with unet_ref.bf16_operands(round_outputs=False):
        lb, lgb, gb, _ = unet_ref.loss_and_grads(o["state"], unet_ref.nhwc_to_nchw(o["x"]), o["y"].float().unsqueeze(1))
    return float(lb), lgb, gb


def _model(c, mode):
    if c.id.startswith("default_"):
        m = UNet()                                        # the bare default: in_channels 1, out_channels 1, 32 features
        assert (m.in_channels, m.out_channels, m.init_features, m.depth) == (c.in_ch, c.out_ch, c.feat, c.depth)
    else:
        m = UNet(c.in_ch, c.out_ch, c.feat, depth=c.depth)
    return m.set_compute_dtype(mode)


def _gradients(m, g64, g32, floor, tag):
    """test_flagship_width_vs_oracle's criterion.  Returns (ratios rel_hip / rel_ref, the worst ratio, its tensor, the
    tensors outside max(4 x the float32 oracle's own distance from float64, floor)); the pre-BatchNorm biases (exact
    gradient 0) hold rounding noise on both sides and are bounded as there."""
    ratios, fails, worst, worst_k = [], [], 0.0, ""
    for k, want64 in g64.items():
        want64 = want64.numpy().ravel()
        if U.is_prebn_bias(k):
            assert np.abs(m.grad(k)).max() <= 1e-6 + 1e-5 * max(np.abs(g32[k].numpy()).max(), 1e-3), (tag, k)
            continue
        nrm = np.linalg.norm(want64) + 1e-30
        rel_ref = np.linalg.norm(g32[k].numpy().ravel() - want64) / nrm
        rel_hip = np.linalg.norm(m.grad(k).ravel() - want64) / nrm
        ratio = rel_hip / max(rel_ref, 1e-9)
        ratios.append(ratio)
        if ratio > worst:
            worst, worst_k = ratio, k
        if not rel_hip <= max(4 * rel_ref, floor):
            fails.append((k, float(rel_hip), float(rel_ref)))
    return ratios, worst, worst_k, fails


@pytest.mark.parametrize("mode", FLOAT32_MODES)
@pytest.mark.parametrize("case", U.TRAIN_CASES, ids=lambda c: c.id)
def test_training_case_float32(case, mode):
    o = _oracle(case.id)
    x, y, r = o["x"], o["y"], o["step"]
    m = _model(case, mode).load_state_dict(o["state"])
    m.eval()
    ev0 = m.forward_nhwc(x.numpy())
    assert ev0.shape == (case.n, case.h, case.w, 1)
    d_eval0 = float(np.abs(ev0[..., 0] - o["eval0"][:, 0].numpy()).max())
    m.train()
    loss = m.forward_backward(x, y)
    dlogit = float(np.abs(m.debug_tensor("logits") - _flat(r["logits"])).max())
    floor = 5e-5 if case.id in U.MARGIN_IDS else 2e-2
    ratios, worst, worst_k, fails = _gradients(m, o["g64"], r["grads"], floor, (case.id, mode))
    print(f"UNETCFG {case.id} {mode} dlogit={dlogit:.2e} ratio_max={worst:.2f} ratio_med={np.median(ratios):.2f} worst={worst_k} "
          f"dloss={abs(loss - r['loss']):.1e} deval0={d_eval0:.1e}")
    assert d_eval0 <= 2e-5
    assert loss == pytest.approx(r["loss"], abs=2e-5)
    assert dlogit <= 2e-5
    assert not fails, fails
    assert np.median(ratios) <= 3.0, np.median(ratios)
    norm = m.apply_gradients(lr=LR, weight_decay=WD)
    assert norm == pytest.approx(r["grad_norm"], rel=5e-3)
    sd = m.state_dict()
    for k, want in o["state1"].items():
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(want), k
        elif k.endswith(("running_mean", "running_var")):
            np.testing.assert_allclose(sd[k].numpy(), want.numpy(), rtol=0, atol=5e-6, err_msg=k)
    m.eval()
    np.testing.assert_allclose(m.forward_nhwc(x.numpy())[..., 0], o["eval1"][:, 0].numpy(), rtol=0, atol=1e-3)


@pytest.mark.parametrize("case", U.TRAIN_CASES, ids=lambda c: c.id)
def test_training_case_bf16_regs(case):
    """test_bf16_data_flow_other_shapes' criterion against `unet_ref.bf16_operands(round_outputs=False)` (this mode keeps
    float32 tensors and rounds the operands of every contraction in registers): closer to the oracle in the SAME arithmetic
    than that oracle is to float32 -- the typical logit by 0.6, the worst by 0.75, every gradient tensor within 1.5 x
    (floor 3e-2), the median ratio <= 1."""
    o = _oracle(case.id)
    x, y = o["x"], o["y"]
    lb, lgb, gb = _oracle_bf16(case.id)
    g32, lg32 = o["step"]["grads"], o["step"]["logits"]
    m = _model(case, "bfloat16_regs").load_state_dict(o["state"]).train()
    loss = m.forward_backward(x, y)
    want, w32 = _flat(lgb), _flat(lg32)
    span = float(np.abs(want).max())
    e_same, e_arith = np.abs(m.debug_tensor("logits") - want), np.abs(w32 - want)
    d_same, d_arith = float(e_same.max()), float(e_arith.max())
    rels, fails, worst, worst_k = [], [], 0.0, ""
    for k, gk in gb.items():
        if U.is_prebn_bias(k):
            continue
        gk = gk.numpy().ravel()
        nrm = np.linalg.norm(gk) + 1e-30
        rel_same = np.linalg.norm(m.grad(k).ravel() - gk) / nrm
        rel_arith = np.linalg.norm(g32[k].numpy().ravel() - gk) / nrm
        ratio = rel_same / max(rel_arith, 1e-9)
        rels.append(ratio)
        if ratio > worst:
            worst, worst_k = ratio, k
        if not rel_same <= max(1.5 * rel_arith, 3e-2):
            fails.append((k, float(rel_same), float(rel_arith)))
    print(f"UNETCFG {case.id} bfloat16_regs dlogit={d_same:.2e} ratio_max={worst:.2f} ratio_med={np.median(rels):.2f} worst={worst_k} "
          f"d_arith={d_arith:.2e} span={span:.2e}")
    assert loss == pytest.approx(lb, rel=5e-3)
    assert d_same <= max(0.75 * d_arith, 5e-3 * span), (d_same, d_arith, span)
    assert np.median(e_same) <= max(0.6 * np.median(e_arith), 1e-3 * span), (np.median(e_same), np.median(e_arith))
    assert not fails, fails
    assert np.median(rels) <= 1.0, np.median(rels)


@pytest.mark.parametrize("mode", FLOAT32_MODES)
@pytest.mark.parametrize("case", U.FORWARD_CASES, ids=lambda c: c.id)
def test_out_channels_forward(case, mode):
    """head_fwd's loop over the output channels: shape, channel order and values, eval and train mode, NCHW and NHWC"""
    st = unet_ref.init_state(case.in_ch, case.out_ch, case.feat, case.depth, seed=case.seed)
    x, y = U.inputs(case)
    xo = unet_ref.nhwc_to_nchw(x)
    with torch.no_grad():
        want_eval = unet_ref.forward(st, xo, training=False).numpy()
        want_train = unet_ref.forward(st, xo, training=True, buffer_updates={}).numpy()
    # the channels differ from one another by far more than the tolerance: a swapped or repeated channel cannot pass
    assert min(np.abs(want_eval[:, a] - want_eval[:, b]).max() for a in range(case.out_ch) for b in range(a)) > 1e-2
    errs = []
    for training, want in ((False, want_eval), (True, want_train)):
        for nchw in (True, False):
            m = _model(case, mode).load_state_dict(st).train(training)      # (a train-mode forward moves the BatchNorm buffers)
            got = m(xo).numpy() if nchw else m.forward_nhwc(x.numpy())
            assert got.shape == ((case.n, case.out_ch, case.h, case.w) if nchw else (case.n, case.h, case.w, case.out_ch))
            got = got if nchw else got.transpose(0, 3, 1, 2)
            errs.append(float(np.abs(got - want).max()))
    print(f"UNETCFG {case.id} {mode} dlogit={max(errs):.2e} ratio_max=- ratio_med=- worst=forward-only")
    assert max(errs) <= 2e-5, errs
    with pytest.raises(RuntimeError, match="defined for out_channels == 1"):
        m.train().train_step(x, y)


KERNEL_OF_LABEL = (("conv_stem", "conv_stem"), ("conv_ws", "conv_ws"), ("gemm_ws", "gemm_ws"), ("conv R", "conv_mfma"),
                   ("wgrad_stem", "wgrad_stem"), ("wgrad_ws", "wgrad_ws"), ("wgrad R", "wgrad_mfma"), ("pconv", "pconv"),
                   ("pwgrad", "pwgrad"))


def _profiled_launches(fn):
    """{kernel: launches} of the contractions `fn` enqueues, from the family and label columns of the context profile"""
    c = Context.get(0)
    c.profile_reset()
    c.profile(True)
    try:
        fn()
    finally:
        c.profile(False)
    fd, path = tempfile.mkstemp(suffix=".csv")
    os.close(fd)
    try:
        c.profile_dump(path)
        rows = [line.rstrip("\n").split(",") for line in open(path)][1:]
    finally:
        os.remove(path)
        c.profile_reset()
    n, labels = {}, []
    for r in rows:
        fam, label = r[1], r[2]
        if fam == "conv_direct_valu":
            k = "direct"
        elif fam in ("conv_igemm_mfma", "wgrad_igemm_mfma"):
            k = next((name for head, name in KERNEL_OF_LABEL if label.startswith(head)), "unknown:" + label)
        else:
            continue
        n[k] = n.get(k, 0) + 1
        labels.append(label)
    return n, labels


@pytest.mark.parametrize("case", U.TRAIN_CASES, ids=lambda c: c.id)
def test_intended_kernels_ran(case):
    """Default arithmetic: the launches of one forward + backward pass, by kernel, are what tests/unet_cases.py derives from
    the gates -- a silent fallback would make the sweep test the wrong kernel.  Pinned examples: the direct VALU kernels run
    at feat = 6 and not at feat = 12; the stem kernels run for the true 4-channel input at feat = 32."""
    o = _oracle(case.id)
    m = _model(case, "float32").load_state_dict(o["state"]).train()
    got, labels = _profiled_launches(lambda: m.forward_backward(o["x"], o["y"]))
    want = U.predicted_launches(case)
    print(f"UNETKERNELS {case.id} {sorted(got.items())}")
    assert got == want, (got, want, labels)
    if case.id == "in4_f32_d1":
        assert any(l.startswith("conv_stem") and " 4->32" in l for l in labels) and any(l.startswith("wgrad_stem") for l in labels)
    if case.id == "in2_f6_d3_48x80":
        assert got["direct"] > 0
    if case.id == "in5_f12_d2_40x24":
        assert "direct" not in got
    # the pass under the profile is the pass the other tests check
    assert m.forward_backward(o["x"], o["y"]) == pytest.approx(o["step"]["loss"], abs=2e-5)


def _adam_of(m, names):
    return {k: m.adam_state(k) for k in names}


@pytest.mark.parametrize("f", [16, 6])
def test_one_model_several_shapes(f):
    """`prepare_shape` keeps buffers and workspace sizes per (n, h, w): one model through U.SHAPES, 2x64x64 -> 1x16x16 ->
    3x32x80 -> 2x64x64 -> 5x16x48 (smaller, larger, repeated, ragged).  After every train_step the model is compared with a FRESH model
    given the same state (parameters, buffers, Adam moments and step count) and the same single step: loss, every gradient,
    every state_dict entry and the eval logits are bit-equal -- no launch geometry of these widths depends on a workspace
    kept from a larger shape (wgrad_stem, which caps its grid by the slab size, needs 32 or 64 features).  Against the
    oracle started from that same state: the float32 criteria of test_training_case_float32.  The batches are seeded so that
    no ReLU input of the oracle's trajectory sits on the threshold (U.SHAPE_SEEDS, pinned by test_unet_cases_host.py): with
    unsearched seeds an f = 6 model met, at step 2, a BatchNorm output 1.5e-7 from the threshold in decoder3's first conv
    (float64 oracle); it landed on the other side on the device, every gradient tensor below it moved by ~1e-3 relative
    (inside the 2e-2 bound) and the median ratio was 909 -- a coin flip, not arithmetic.
    The 1x16x16 step leaves one value per channel at the bottleneck: the reference's BatchNorm raises on it in training, so
    that step is no parity claim; it is the small shape between two large ones, checked against the oracle like the rest."""
    m = UNet(3, 1, f).load_state_dict(U.shape_state(f))
    names = [k for k, _ in m.named_parameters()]
    for i, ((n, h, w), seed) in enumerate(zip(U.SHAPES, U.SHAPE_SEEDS[f])):
        x, y = U.shape_inputs(seed, n, h, w)
        st0, adam0 = m.state_dict(), _adam_of(m, names)
        loss = m.train_step(x, y, lr=LR, weight_decay=WD)
        fresh = UNet(3, 1, f).load_state_dict(st0)
        for k, (mm, vv, step) in adam0.items():
            fresh.load_adam_state(k, mm, vv)
        fresh.set_adam_step(i)
        assert all(step == i for _, _, step in adam0.values())
        loss_f = fresh.train_step(x, y, lr=LR, weight_decay=WD)
        # --- against the fresh model: bit-equal
        assert loss == loss_f, (i, loss, loss_f)
        for k in names:
            assert m.grad(k).tobytes() == fresh.grad(k).tobytes(), (i, k)
        sd, sdf = m.state_dict(), fresh.state_dict()
        for k in sd:
            assert torch.equal(sd[k], sdf[k]), (i, k)
        m.eval(); fresh.eval()
        ev, evf = m.forward_nhwc(x.numpy()), fresh.forward_nhwc(x.numpy())
        m.train(); fresh.train()
        assert ev.tobytes() == evf.tobytes(), i
        # --- against the oracle from the same state
        xo, yo = unet_ref.nhwc_to_nchw(x), y.float().unsqueeze(1)
        _, _, g64, _ = unet_ref.loss_and_grads(U.to64(st0), xo.double(), yo.double())
        ost = _clone(st0)
        adam = {"step": i, "m": {k: torch.from_numpy(adam0[k][0].copy()) for k in names},
                "v": {k: torch.from_numpy(adam0[k][1].copy()) for k in names}}
        r = unet_ref.train_step(ost, adam, xo, yo, lr=LR, weight_decay=WD)
        ratios, worst, worst_k, fails = _gradients(m, g64, r["grads"], 2e-2, (f, i))
        with torch.no_grad():
            want_ev = unet_ref.forward(ost, xo, training=False)[:, 0].numpy()
        d_ev = float(np.abs(ev[..., 0] - want_ev).max())
        print(f"UNETCFG shapes_f{f}_step{i}_{n}x{h}x{w} float32 dlogit={d_ev:.2e} ratio_max={worst:.2f} "
              f"ratio_med={np.median(ratios):.2f} worst={worst_k} dloss={abs(loss - r['loss']):.1e}")
        assert loss == pytest.approx(r["loss"], abs=2e-5), i
        assert not fails, (i, fails)
        assert np.median(ratios) <= 3.0, (i, np.median(ratios))
        assert d_ev <= 1e-3, (i, d_ev)
