"""-m gpu: parity AT THE BENCHED CONFIGURATION (BASELINE configs[1]/[4] shape): UNet(3,1,32), batch 64 x 128x128x3
patches produced by the device input pipeline bench.py uses (`make_training_patches_device`), one training
step (train_model.py:139-151) in each of the three arithmetic modes of the contraction kernels, against the
CPU oracle in float32 and -- to calibrate the gradient tolerance instead of guessing it -- in float64.

At this size every layer launches the tile instantiations the bench runs (the double tiles of the native-float32
and bf16 modes included), so the numbers bench.py reports come from kernels this file has checked.
"""
from collections import OrderedDict
from functools import lru_cache

import numpy as np
import pytest
import torch

from oracle import metrics_ref, unet_ref
from rfi_toolbox_amd.data_generation import make_training_patches_device
from rfi_toolbox_amd.models import UNet

pytestmark = pytest.mark.gpu
B, S, FEAT = 64, 128, 32


def _is_prebn_bias(k):          # conv bias in front of a BatchNorm: exactly 0 gradient in exact arithmetic
    return k.endswith(".0.bias") or k.endswith(".3.bias")


@lru_cache(maxsize=1)
def _case():
    """Inputs, initial state and the oracle's float32 / float64 answers, computed once for all modes."""
    d_x, d_y = make_training_patches_device(B, S, seed=1234, device=0)       # bench.py's inputs (rank 0)
    x = torch.from_numpy(d_x.numpy().copy())
    y = torch.from_numpy(d_y.numpy().copy())
    torch.manual_seed(1234)                                                  # bench.py's weights
    st = UNet(3, 1, FEAT).state_dict()
    xo, yo = unet_ref.nhwc_to_nchw(x), y.float().unsqueeze(1)
    torch.set_num_threads(max(1, min(32, torch.get_num_threads())))
    l32, lg32, g32, bufs = unet_ref.loss_and_grads(st, xo, yo)
    st64 = OrderedDict((k, v.double() if v.dtype.is_floating_point else v.clone()) for k, v in st.items())
    l64, lg64, g64, _ = unet_ref.loss_and_grads(st64, xo.double(), yo.double())
    total, coef = unet_ref.clip_coefficient(g32, 1.0)
    return dict(x=x, y=y, st=st, l32=float(l32), lg32=lg32, g32=g32, g64=g64, lg64=lg64, l64=float(l64),
                bufs=bufs, norm=float(total))


@lru_cache(maxsize=1)
def _case_bf16():
    """The oracle in the bf16-operand arithmetic (`unet_ref.bf16_operands`) on the same inputs and state."""
    c = _case()
    xo, yo = unet_ref.nhwc_to_nchw(c["x"]), c["y"].float().unsqueeze(1)
    with unet_ref.bf16_operands(round_outputs=True):
        l, lg, g, bufs = unet_ref.loss_and_grads(c["st"], xo, yo)
    total, _ = unet_ref.clip_coefficient(g, 1.0)
    return dict(l=float(l), lg=lg, g=g, bufs=bufs, norm=float(total))


def test_bench_configuration_step_bf16_vs_bf16_operand_oracle():
    """bf16 compute mode at the bench shape (the double-tile bf16 instantiations run here) against the oracle
    in the SAME arithmetic.  bf16 operands move a deep-layer weight gradient by tens of percent against float32
    (rounding noise through ~20 layers each way plus ReLU-mask flips), so the float32 oracle only calibrates:
    the HIP result must sit closer to the same-arithmetic oracle than that oracle sits to float32."""
    c, b = _case(), _case_bf16()
    m = UNet(3, 1, FEAT).load_state_dict(c["st"]).train().set_compute_dtype("bfloat16")
    loss = m.forward_backward(c["x"], c["y"])
    assert loss == pytest.approx(b["l"], rel=2e-3)
    logits = m.debug_tensor("logits")
    want = b["lg"].permute(0, 2, 3, 1).reshape(-1).numpy()
    w32 = c["lg32"].permute(0, 2, 3, 1).reshape(-1).numpy()
    span = float(np.abs(want).max())
    d_same, d_arith = np.abs(logits - want).max(), np.abs(w32 - want).max()
    assert d_same <= max(0.5 * d_arith, 2e-3 * span), (d_same, d_arith, span)
    worst = []
    for k, gb in b["g"].items():
        if _is_prebn_bias(k):
            continue
        gb = gb.numpy().ravel()
        nrm = np.linalg.norm(gb) + 1e-30
        rel_same = np.linalg.norm(m.grad(k).ravel() - gb) / nrm
        rel_arith = np.linalg.norm(c["g32"][k].numpy().ravel() - gb) / nrm
        worst.append((rel_same / max(rel_arith, 1e-9), k, rel_same, rel_arith))
        # forward roundings repeat exactly (same inputs, same RNE), backward ones only partly: gradient tensors are
        # cancellation-heavy sums, so their float32 values differ in the low bits between two summation orders
        # and a few percent of them round to the neighbouring bf16 -- hence "no further from the same-arithmetic
        # oracle than float32 is", per tensor, and clearly closer for the typical tensor
        # -- and still EVERY tensor must sit clearly closer to the same-arithmetic oracle than float32 does (measured,
        # round 3: worst tensor 0.53 of the float32 distance, median 0.43, none of the 64 above 0.55)
        assert rel_same <= max(0.7 * rel_arith, 5e-3), (k, rel_same, rel_arith)
    assert np.median([w[0] for w in worst]) <= 0.55, sorted(worst)[-3:]
    norm = m.apply_gradients(lr=1e-4, weight_decay=1e-5)
    assert norm == pytest.approx(b["norm"], rel=2e-2)


@pytest.mark.parametrize("mode", ["float32", "float32_mfma"])
def test_bench_configuration_step_vs_oracle(mode):
    c = _case()
    m = UNet(3, 1, FEAT).load_state_dict(c["st"]).train().set_compute_dtype(mode)
    loss = m.forward_backward(c["x"], c["y"])
    logits = m.debug_tensor("logits")
    want_logits = c["lg32"].permute(0, 2, 3, 1).reshape(-1).numpy()
    span = float(np.abs(want_logits).max())
    f32 = mode != "bfloat16"
    # loss and logits: float32 modes agree with the float32 oracle to rounding; bf16 operands to ~2^-8 relative
    assert loss == pytest.approx(c["l32"], abs=2e-5 if f32 else 2e-2 * abs(c["l32"]))
    assert np.abs(logits - want_logits).max() <= (2e-4 if f32 else 0.05 * span)
    ratios, rels = [], []
    for k, want64 in c["g64"].items():
        want64 = want64.numpy().ravel()
        got = m.grad(k).ravel()
        assert np.isfinite(got).all(), k
        if _is_prebn_bias(k):
            assert np.abs(got).max() <= 1e-6 + (1e-5 if f32 else 1e-2) * max(np.abs(c["g32"][k].numpy()).max(), 1e-3), k
            continue
        nrm = np.linalg.norm(want64) + 1e-30
        rel_ref = np.linalg.norm(c["g32"][k].numpy().ravel() - want64) / nrm
        rel_hip = np.linalg.norm(got - want64) / nrm
        rels.append(rel_hip)
        if f32:
            # the criterion of test_flagship_width_vs_oracle: each tensor within 4x the float32 CPU path's own
            # distance from the float64 result (or 2e-2 where a ReLU-threshold element dominates) ...
            assert rel_hip <= max(4 * rel_ref, 2e-2), (k, rel_hip, rel_ref)
            ratios.append(rel_hip / max(rel_ref, 1e-9))
        else:
            assert rel_hip <= 0.25, (k, rel_hip)          # bf16 operands through up to 23 layers, both directions
    if f32:
        assert np.median(ratios) <= 3.0, np.median(ratios)  # ... and the typical tensor at that noise level
    else:
        assert np.median(rels) <= 0.08, np.median(rels)
    norm = m.apply_gradients(lr=1e-4, weight_decay=1e-5)
    assert norm == pytest.approx(c["norm"], rel=5e-3 if f32 else 5e-2)
    sd = m.state_dict()
    for k in ("encoder1.conv.conv.1.running_mean", "encoder4.conv.conv.4.running_var", "bottleneck.conv.4.running_var",
              "decoder1.conv.conv.4.running_var"):
        np.testing.assert_allclose(sd[k].numpy(), c["bufs"][k].numpy(), rtol=0 if f32 else 2e-2,
                                   atol=5e-6 if f32 else 2e-3, err_msg=k)
    assert int(sd["encoder1.conv.conv.1.num_batches_tracked"]) == 2


def test_bench_configuration_masks_agree_across_modes():
    """Eval-mode masks of the two float32 arithmetic modes at the bench shape on the same (random-init) weights
    differ at most in threshold pixels: fewer than 1e-4 of the pixels, and |dIoU| <= 1e-3 against each other."""
    c = _case()
    masks = {}
    for mode in ("float32", "float32_mfma"):
        m = UNet(3, 1, FEAT).load_state_dict(c["st"]).eval().set_compute_dtype(mode)
        masks[mode] = m.forward_nhwc(c["x"].numpy())[..., 0] > 0
    a, b = masks["float32"], masks["float32_mfma"]
    assert (a != b).mean() <= 1e-4
    if (a | b).mean() > 0.01:
        assert metrics_ref.evaluate_segmentation(a, b)["iou"] >= 1 - 1e-3


def test_bench_dump_outputs_is_the_state_after_its_timed_steps(tmp_path):
    """bench.py --dump-outputs writes what its timed path computed in the last timed step: the loss and the model state after
    W + K steps, for the float32 line and its bfloat16 companion -- bit for bit what the same steps on the same seeded
    inputs give through the model API (the sustained sample and the profile steps that follow do not leak into it)."""
    import os
    import subprocess
    import sys

    from rfi_toolbox_amd._lib import Hyper
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    b, s, f, warmup, steps = 4, 128, 32, 2, 3            # the benched patch and width, fewer patches
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--batch", str(b), "--size", str(s),
                        "--features", str(f), "--warmup", str(warmup), "--steps", str(steps), "--sustain-steps", "20",
                        "--profile-steps", "1", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d_x, d_y = make_training_patches_device(b, s, seed=1234, device=0)
    hp = Hyper(1e-4, 0.9, 0.999, 1e-8, 1e-5, 1.0)
    for mode, prefix in (("float32", ""), ("bfloat16", "bfloat16.")):
        torch.manual_seed(1234)
        m = UNet(3, 1, f, device=0).train().set_compute_dtype(mode)
        for _ in range(warmup + steps):
            m.train_step_async(d_x.ptr, d_y.ptr, b, s, s, hp)
        loss, _ = m.last_loss()
        assert float(np.load(tmp_path / f"{prefix}loss.npy")) == loss
        for k, v in m.state_dict().items():
            got = np.load(tmp_path / f"{prefix}{k}.npy")
            assert got.dtype in (np.float32, np.float64), (k, got.dtype)
            np.testing.assert_array_equal(got, v.numpy(), err_msg=prefix + k)


def test_bench_plain_line_is_the_headline_and_full_adds_the_rest():
    """A plain bench.py run times its steps and prints the headline alone; --full adds the sustained sample, the profile
    (roofline, kernel families) and the bfloat16 companion line to the same headline fields."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--batch", "4", "--warmup", "2", "--steps", "3"]
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline", "--sustain-steps", "20", "--profile-steps", "1"])):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, r.stdout
        lines[name] = json.loads(out[0])
    for d in lines.values():
        assert d["metric"] == "training patches/sec (128x128x3)" and d["unit"] == "patches/s" and d["higher_is_better"] is True
        assert d["dtype"] == "f32" and d["steps"] == 3 and d["warmup"] == 2
        assert d["value"] > 0 and abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
        assert np.isfinite(d["step"]["final_loss"])
    plain, full = lines["plain"], lines["full"]
    assert not {"sustained", "roofline", "families", "families_overlapped", "bfloat16", "cpu_baseline"} & set(plain)
    assert full["sustained"]["steps"] == 20 and "roofline" in full and full["families"] and full["families_overlapped"]
    assert full["bfloat16"]["dtype"] == "bf16" and "roofline" in full["bfloat16"] and full["bfloat16"]["families"]
    assert plain["step"]["final_loss"] == full["step"]["final_loss"]      # the same K timed steps from the same seeds
