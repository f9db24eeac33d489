"""No GPU: proves the oracle harness of the backbone tests (tests/backbone_cases.py) on the oracle's own numbers.

test_masked_oracle_is_the_oracle    the masked float64 oracle with its own masks equals the plain one bit for bit
test_masked_float32_at_rounding     the masked float32 oracle with float64's masks stays at float32 rounding level
test_recording_layout               hook order = state-dict conv order, 49 ReLU inputs, shapes as the product reports them
test_masks_from_tensors             the mask derivation, fed the float32 oracle's tensors, returns that oracle's masks
test_checkers_*                     the clean float32 oracle passes; four planted errors, fed in its place, fail
"""
import types

import numpy as np
import pytest
import torch

import backbone_cases as B
from rfi_toolbox_amd.models.backbone import ResNet50FPN

BOUND = 64          # the largest constant the device test may use (tests/test_gpu_backbone.py): a planted error must miss it


@pytest.fixture(scope="module")
def runs():
    c = B.HOST_CASE
    st, x, dfe = B.case_inputs(c)
    plain64 = B.run_oracle(st, x, dfe, torch.float64)
    masks = B.own_masks(plain64)
    m64 = B.run_oracle(st, x, dfe, torch.float64, masks=masks)
    m32 = B.run_oracle(st, x, dfe, torch.float32, masks=masks)
    return types.SimpleNamespace(c=c, st=st, x=x, dfe=dfe, plain64=plain64, masks=masks, m64=m64, m32=m32)


def test_masked_oracle_is_the_oracle(runs):
    assert len(runs.masks) == B.N_RELU
    for k, v in runs.plain64.grads.items():
        assert np.array_equal(runs.m64.grads[k], v), k
    for k, v in runs.plain64.tensors.items():
        assert np.array_equal(runs.m64.tensors[k], v), k


def test_masked_float32_at_rounding(runs):
    # 2^-16 = 256 half-units of float32: ~50 layers of float32 rounding each way, none of it amplified by a flipped ReLU
    for k, g64 in runs.m64.grads.items():
        rel = np.linalg.norm(runs.m32.grads[k].astype(np.float64).ravel() - g64.ravel()) / np.linalg.norm(g64)
        assert rel <= 2.0 ** -16, (k, rel)
    for k, t64 in runs.m64.tensors.items():
        assert np.abs(runs.m32.tensors[k] - t64).max() <= 2.0 ** -16 * max(1.0, np.abs(t64).max()), k


def test_recording_layout(runs):
    c = runs.c
    names = B.conv_names(runs.st)
    assert runs.m64.hooked == names and len(names) == 1 + 16 * 3 + 4 + 8
    t = runs.m64.tensors
    for i, k in enumerate(names):
        assert t[f"conv.{i}"].shape[-1] == runs.st[k + ".weight"].shape[0], k
    assert t["conv.0"].shape == (c.n, c.h // 2, c.wd // 2, c.w)
    assert t["pool"].shape == (c.n, c.h // 4, c.wd // 4, c.w)
    assert [f"block.{b}" in t for b in range(16)] == [True] * 16 and "block.16" not in t
    assert t["block.15"].shape == (c.n, c.h // 32, c.wd // 32, 32 * c.w)
    shapes = ResNet50FPN._shapes(types.SimpleNamespace(out_channels=c.f), c.n, c.h, c.wd)
    assert [t[f"feat.{i}"].shape for i in range(5)] == shapes
    assert [t[f"merged.{i}"].shape for i in range(4)] == shapes[:4]
    assert [runs.m64.grads[f"dmerged.{i}"].shape for i in range(4)] == shapes[:4]
    # the ReLU inputs in call order are the tensors relu_sources() names
    for z, (kind, i), in zip(runs.plain64.relu_in, B.relu_sources(names)):
        want = t[f"block.{i}"].shape if kind == "block" else t[f"conv.{i}"].shape
        assert (z.shape[0], z.shape[2], z.shape[3], z.shape[1]) == want, (kind, i)


def _chan(st, name):
    """The device's ``chan.<i>`` record of the stem / a conv1 / a conv2: frozen scale at [4 c, 5 c), shift at [5 c, 6 c)."""
    bn = name.replace("conv", "bn")
    g, b, rm, rv = (st[f"{bn}.{s}"].numpy() for s in ("weight", "bias", "running_mean", "running_var"))
    scale = g / np.sqrt(rv + np.float32(1e-5))
    out = np.zeros(8 * g.size, np.float32)
    out[4 * g.size:5 * g.size] = scale
    out[5 * g.size:6 * g.size] = b - rm * scale
    return out


def test_masks_from_tensors(runs):
    c = runs.c
    r32 = B.run_oracle(runs.st, runs.x, runs.dfe, torch.float32)
    names = B.conv_names(runs.st)

    def get(name):
        base, i = name.split(".")
        return _chan(runs.st, names[int(i)]) if base == "chan" else r32.tensors[name].ravel()
    dm = B.masks_from_tensors(get, names, c.n, c.h, c.wd)
    own = B.own_masks(r32)
    differ = sum(int((a != b).sum()) for a, b in zip(dm.masks, own))
    # (the oracle forms scale and shift with torch's rsqrt: an element may differ where z is within rounding of 0)
    assert len(dm.masks) == B.N_RELU and differ <= dm.undecided + 2, (differ, dm.undecided)
    assert all(a.shape == b.shape for a, b in zip(dm.masks, own))
    # a window with two equal positive maxima at different positions is undecided; an all-zero one is not
    a = np.zeros((1, 4, 4, 1), np.float32)
    assert B.undecided_pool_windows(a) == 0
    a[0, 1, 1, 0] = a[0, 1, 2, 0] = 1.0
    assert B.undecided_pool_windows(a) >= 1
    a[0, 1, 2, 0] = 0.999
    assert B.undecided_pool_windows(a) == 0


def test_checkers_pass_on_the_float32_oracle(runs):
    r, k = B.check_forward(runs.m32.tensors, runs.m32.tensors, runs.m64.tensors, bound=BOUND)
    assert r <= 1.0, (r, k)
    r, k = B.check_gradients(runs.m32.grads, runs.m32.grads, runs.m64.grads, bound=BOUND)
    assert r <= 1.0, (r, k)


def test_checkers_fail_on_a_scaled_gradient(runs):
    k = "body.layer2.0.conv2.weight"
    hip = dict(runs.m32.grads)
    hip[k] = hip[k] * np.float32(1 + 1e-4)
    with pytest.raises(AssertionError, match="layer2.0.conv2"):
        B.check_gradients(hip, runs.m32.grads, runs.m64.grads, bound=BOUND)


def test_checkers_fail_on_a_transposed_tensor(runs):
    i = B.conv_names(runs.st).index("body.layer2.0.conv2")
    hip = dict(runs.m32.tensors)
    t = hip[f"conv.{i}"]
    assert t.shape[1] != t.shape[2]
    hip[f"conv.{i}"] = np.ascontiguousarray(t.transpose(0, 2, 1, 3)).ravel()      # (flat, as the device returns it)
    with pytest.raises(AssertionError, match=f"conv.{i}'"):
        B.check_forward(hip, runs.m32.tensors, runs.m64.tensors, bound=BOUND)


def test_checkers_fail_on_a_flipped_mask_element(runs):
    masks = [m.clone() for m in runs.masks]
    k = 3 * 16                                     # the output ReLU of the last block
    z = runs.plain64.relu_in[k]
    at = np.unravel_index(int(z.abs().argmax()), z.shape)
    masks[k][at] = ~masks[k][at]
    flipped = B.run_oracle(runs.st, runs.x, runs.dfe, torch.float32, masks=masks)
    with pytest.raises(AssertionError):
        B.check_gradients(flipped.grads, runs.m32.grads, runs.m64.grads, bound=BOUND)
    with pytest.raises(AssertionError, match="block.15"):
        B.check_forward(flipped.tensors, runs.m32.tensors, runs.m64.tensors, bound=BOUND)


def test_checkers_fail_on_wrong_merge_parity(runs):
    names = B.conv_names(runs.st)
    t = runs.m32.tensors
    lat = t[f"conv.{names.index('fpn.inner_blocks.1.0')}"]
    up = t["merged.2"].repeat(2, axis=1).repeat(2, axis=2)
    assert np.array_equal(lat + up, t["merged.1"])                  # the right parity: pixel (y, x) reads (y // 2, x // 2)
    hip = dict(t)
    hip["merged.1"] = lat + np.roll(up, 1, axis=2)                  # reads ((x + 1) // 2 - 1) instead
    with pytest.raises(AssertionError, match="merged.1"):
        B.check_forward(hip, t, runs.m64.tensors, bound=BOUND)
