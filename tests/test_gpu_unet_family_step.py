"""-m gpu: the whole training step of a K-channel U-Net on class-bit labels against the unchanged CPU oracle
(oracle/unet_ref.py, whose loss text flattens whatever shape it is given), head backward for several outputs included.

Models: UNet(8, 5, 4, depth=2) at 2 x 8 x 12, UNet(3, 2, 8) at 2 x 16 x 16 and UNet(8, 3, 16, depth=2) at 2 x 16 x 24 (a width
at which the plane flows keep bfloat16 gradient tensors), losses bce_dice (the oracle's own
segmentation_loss on (N, K, H, W) targets) and bce_class_dice (its definition in tests/family_step_cases.py), every
compute mode:

test_family_step_float32     float32, float32_mfma, float32_planes: the criteria of test_training_case_float32
test_family_step_bf16_regs   the criteria of test_training_case_bf16_regs
test_family_step_bfloat16    the criterion of test_bf16_data_flow_other_shapes
test_two_runs_bit_equal      two fresh models give bit-equal losses and gradients in every mode

Each case and mode prints one line:  FAMILYSTEP <id> <loss> <mode> dlogit=... ratio_max=... ratio_med=... worst=<tensor>"""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import unet_cases as U
from family_step_cases import CASES, LOSS_FN, LOSSES, inputs, targets
from oracle import unet_ref
from rfi_toolbox_amd.models import UNet

pytestmark = pytest.mark.gpu

LR, WD = 1e-4, 1e-5
FLOAT32_MODES = ("float32", "float32_mfma", "float32_planes")
ALL_MODES = FLOAT32_MODES + ("bfloat16_regs", "bfloat16")


def _clone(st):
    return OrderedDict((k, v.clone()) for k, v in st.items())


def _flat(logits_nchw):
    return logits_nchw.permute(0, 2, 3, 1).reshape(-1).numpy()


@functools.lru_cache(maxsize=None)
def _oracle(cid, loss):
    c = next(c for c in CASES if c.id == cid)
    st = unet_ref.init_state(c.in_ch, c.K, c.feat, c.depth, seed=c.seed)
    x, y = inputs(c)
    xo = unet_ref.nhwc_to_nchw(x)
    yo = targets(y, c.K)                                  # (N, K, H, W)
    assert tuple(yo.shape) == (c.n, c.K, c.h, c.w) and 0 < float(yo.mean()) < 1
    fn = LOSS_FN[loss]
    o = {"state": st, "x": x, "y": y, "xo": xo, "yo": yo}
    _, _, o["g64"], _ = unet_ref.loss_and_grads(U.to64(st), xo.double(), yo.double(), loss_fn=fn)
    with torch.no_grad():
        o["eval0"] = unet_ref.forward(st, xo, training=False)
    ost = _clone(st)
    o["step"] = unet_ref.train_step(ost, unet_ref.new_adam_state(ost), xo, yo, lr=LR, weight_decay=WD, loss_fn=fn)
    o["state1"] = ost
    with torch.no_grad():
        o["eval1"] = unet_ref.forward(ost, xo, training=False)
    return o


def _model(c, mode, loss, state):
    m = UNet(c.in_ch, c.K, c.feat, depth=c.depth).set_compute_dtype(mode).set_targets("class_bits").set_loss(loss)
    return m.load_state_dict(state)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("mode", FLOAT32_MODES)
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_family_step_float32(case, loss, mode):
    o = _oracle(case.id, loss)
    x, y, r = o["x"], o["y"], o["step"]
    m = _model(case, mode, loss, o["state"])
    m.eval()
    ev0 = m.forward_nhwc(x.numpy())
    assert ev0.shape == (case.n, case.h, case.w, case.K)
    d_eval0 = float(np.abs(ev0 - _nhwc(o["eval0"])).max())
    m.train()
    got_loss = m.forward_backward(x, y)
    dlogit = float(np.abs(m.debug_tensor("logits") - _flat(r["logits"])).max())
    ratios, fails, worst, worst_k = [], [], 0.0, ""
    for k, want64 in o["g64"].items():
        want64 = want64.numpy().ravel()
        if U.is_prebn_bias(k):
            assert np.abs(m.grad(k)).max() <= 1e-6 + 1e-5 * max(np.abs(r["grads"][k].numpy()).max(), 1e-3), k
            continue
        nrm = np.linalg.norm(want64) + 1e-30
        rel_ref = np.linalg.norm(r["grads"][k].numpy().ravel() - want64) / nrm
        rel_hip = np.linalg.norm(m.grad(k).ravel() - want64) / nrm
        ratio = rel_hip / max(rel_ref, 1e-9)
        ratios.append(ratio)
        if ratio > worst:
            worst, worst_k = ratio, k
        if not rel_hip <= max(4 * rel_ref, 2e-2):                 # (the floor of the cases outside U.MARGIN_IDS)
            fails.append((k, float(rel_hip), float(rel_ref)))
    print(f"FAMILYSTEP {case.id} {loss} {mode} dlogit={dlogit:.2e} ratio_max={worst:.2f} ratio_med={np.median(ratios):.2f} "
          f"worst={worst_k} dloss={abs(got_loss - r['loss']):.1e} deval0={d_eval0:.1e}")
    assert d_eval0 <= 2e-5
    assert got_loss == pytest.approx(r["loss"], abs=2e-5)
    assert dlogit <= 2e-5
    assert not fails, fails
    assert np.median(ratios) <= 3.0, np.median(ratios)
    norm = m.apply_gradients(lr=LR, weight_decay=WD)
    assert norm == pytest.approx(r["grad_norm"], rel=5e-3)
    m.eval()
    np.testing.assert_allclose(m.forward_nhwc(x.numpy()), _nhwc(o["eval1"]), rtol=0, atol=1e-3)


def _same_arithmetic(case, loss, mode, round_outputs):
    """how a reduced-precision mode is judged (test_training_case_bf16_regs, test_bf16_data_flow_other_shapes): closer to
    the oracle in the SAME arithmetic than that oracle is to float32"""
    o = _oracle(case.id, loss)
    x, y = o["x"], o["y"]
    with unet_ref.bf16_operands(round_outputs=round_outputs):
        lb, lgb, gb, _ = unet_ref.loss_and_grads(o["state"], o["xo"], o["yo"], loss_fn=LOSS_FN[loss])
    g32, lg32 = o["step"]["grads"], o["step"]["logits"]
    m = _model(case, mode, loss, o["state"]).train()
    got_loss = m.forward_backward(x, y)
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
    print(f"FAMILYSTEP {case.id} {loss} {mode} dlogit={d_same:.2e} ratio_max={worst:.2f} ratio_med={np.median(rels):.2f} "
          f"worst={worst_k} d_arith={d_arith:.2e} span={span:.2e}")
    assert got_loss == pytest.approx(float(lb), rel=5e-3)
    assert d_same <= max(0.75 * d_arith, 5e-3 * span), (d_same, d_arith, span)
    assert np.median(e_same) <= max(0.6 * np.median(e_arith), 1e-3 * span), (np.median(e_same), np.median(e_arith))
    assert not fails, fails
    assert np.median(rels) <= 1.0, np.median(rels)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_family_step_bf16_regs(case, loss):
    _same_arithmetic(case, loss, "bfloat16_regs", round_outputs=False)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_family_step_bfloat16(case, loss):
    _same_arithmetic(case, loss, "bfloat16", round_outputs=case.feat % 4 == 0)


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_two_runs_bit_equal(case, mode):
    o = _oracle(case.id, "bce_class_dice")
    runs = []
    for _ in range(2):
        m = _model(case, mode, "bce_class_dice", o["state"]).train()
        loss = m.forward_backward(o["x"], o["y"])
        runs.append((np.float32(loss).tobytes(), [m.grad(k).tobytes() for k, _ in m.named_parameters()]))
    assert runs[0] == runs[1]
