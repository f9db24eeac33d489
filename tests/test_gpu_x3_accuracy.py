"""-m gpu: every kernel variant that implements the float32-by-3xbf16 arithmetic, held to what DESIGN.md claims of it:
ONE float32 rounding per product.

test_single_product_probe   operands built so that every output is a single product or an exact zero (tests/x3_ref.py),
                            both operand roles: e = max |got - a b| / |a b| <= 16 (units of 2^-24; a correct kernel: <= 6,
                            a kernel that loses one piece product: >= 90, pinned on the CPU by test_x3_probes_host.py),
                            and exact zeros where no product lands.  Also the sharpest addressing test the tiles, halos,
                            taps, k-slots and split-K slabs get: a misplaced element is a wrong product.
test_bias_is_added_exactly  zero filters: the output equals the bias bit for bit.
test_dense_accumulation     randn operands, and operands spread over 2^-20 .. 2^20 with exactly cancelling pairs, on the
                            per-element statistic max |got - float64| / sum |a||b|: within 4x of what torch-CPU float32
                            shows on the same inputs (another summation order, not another arithmetic).

The cases (tests/x3_cases.py) are read off the dispatch code, one per tile variant, whole and ragged.  Every test checks
the profile label of the contraction it launched: a shape that falls to another kernel fails, it does not pass on the
wrong kernel.  The figures each test prints are the table in DESIGN.md ("measured per-product error").

Not expressible through the kernel-level ABI, hence left to the model-level tests (test_gpu_unet.py,
test_gpu_resnet_unet.py, test_gpu_bench_config.py): concat views (a pixel stride larger than the channel count), the
BatchNorm-statistics epilogue of the forward kernels, and the LeakyReLU load transform (in_relu carries no slope)."""
import os
import tempfile
import zlib

import numpy as np
import pytest
import torch

import x3_ref as X
from gpu_util import P, check, ctx, lib, nchw, nhwc
from x3_cases import CASES

pytestmark = pytest.mark.gpu

E_MAX = 16.0            # units of 2^-24; derived bound of a correct kernel: 6 (x3_ref.py)
DENSE_MARGIN = 4.0      # device vs torch-CPU float32 on the same inputs, both against float64

CONTRACTIONS = ("conv_igemm_mfma", "wgrad_igemm_mfma", "conv_direct_valu")      # profile families of the conv kernels


def _seed(case, salt):
    return zlib.crc32(f"{case.id}/{salt}".encode())


def _run(case, a, b, bias=None, scale=None, shift=None):
    """the operation through the C ABI; returns the result in the layout of torch (NCHW / the reference's filter layout)"""
    n, h, w, cin, cout = case.shape
    op, impl, c = case.op, case.impl, ctx()
    relu = 1 if case.relu else 0
    dsc = c.to_device(scale.numpy()) if scale is not None else None
    dsh = c.to_device(shift.numpy()) if shift is not None else None
    dbias = c.to_device(bias.numpy()) if bias is not None else None
    wgrad = X.OPS[op].kind == "wgrad"
    da = c.to_device(nhwc(a))
    db = c.to_device(nhwc(b)) if wgrad else c.to_device(np.ascontiguousarray(b.numpy()))
    if op == "conv3x3" or op == "conv1x1":
        out = c.empty((n, h, w, cout))
        fn = lib.rfi_op_conv3x3 if op == "conv3x3" else lib.rfi_op_conv1x1
        call = lambda: fn(c.handle, impl, P(da), n, h, w, cin, P(db), P(dbias), cout, P(dsc), P(dsh), relu, P(out))
    elif op == "conv3x3_dgrad":
        out = c.empty((n, h, w, cin))
        call = lambda: lib.rfi_op_conv3x3_dgrad(c.handle, impl, P(da), n, h, w, cout, P(db), cin, P(out))
    elif op == "convt2x2":
        out = c.empty((n, 2 * h, 2 * w, cout))
        call = lambda: lib.rfi_op_convt2x2(c.handle, impl, P(da), n, h, w, cin, P(db), P(dbias), cout, P(out))
    elif op == "convt2x2_dgrad":
        out = c.empty((n, h, w, cin))
        call = lambda: lib.rfi_op_convt2x2_dgrad(c.handle, impl, P(da), n, h, w, cout, P(db), cin, P(out))
    elif op in ("conv_s2_k3", "conv_s2_k1"):
        out = c.empty((n, h // 2, w // 2, cout))
        call = lambda: lib.rfi_op_conv_s2(c.handle, impl, int(op[-1]), P(da), n, h, w, cin, P(db), cout, P(out))
    elif op in ("conv_s2_k3_dgrad", "conv_s2_k1_dgrad"):
        out = c.empty((n, h, w, cin))
        call = lambda: lib.rfi_op_conv_s2_dgrad(c.handle, impl, int(op[9]), P(da), n, h, w, cout, P(db), cin, P(out))
    elif op == "conv3x3_wgrad":
        out = c.empty((cout, cin, 3, 3))
        call = lambda: lib.rfi_op_conv3x3_wgrad(c.handle, impl, P(da), P(db), n, h, w, cin, cout, P(dsc), P(dsh), relu, P(out))
    elif op in ("conv_s2_k3_wgrad", "conv_s2_k1_wgrad"):
        k = int(op[9])
        out = c.empty((cout, cin, k, k))
        call = lambda: lib.rfi_op_conv_s2_wgrad(c.handle, impl, k, P(da), P(db), n, h, w, cin, cout, P(out))
    else:
        assert op == "convt2x2_wgrad", op
        out = c.empty((cin, cout, 2, 2))
        call = lambda: lib.rfi_op_convt2x2_wgrad(c.handle, impl, P(da), P(db), n, h, w, cin, cout, P(out))
    assert scale is None or op in ("conv3x3", "conv1x1", "conv3x3_wgrad"), "only these entry points take a load transform"
    c.profile_reset()
    c.profile(True)
    try:
        check(call())
    finally:
        c.profile(False)
    _assert_label(case, c)
    got = torch.from_numpy(out.numpy().copy())
    return got if wgrad else nchw(got.numpy())


def _assert_label(case, c):
    """exactly one contraction was launched, and its label names the kernel, the shape and the tile variant of the case"""
    fd, path = tempfile.mkstemp(suffix=".csv")
    os.close(fd)
    try:
        c.profile_dump(path)
        rows = [line.rstrip("\n").split(",") for line in open(path)][1:]
    finally:
        os.remove(path)
        c.profile_reset()
    labels = [r[2] for r in rows if r[1] in CONTRACTIONS]
    assert len(labels) == 1, labels
    head, tail = case.label[0], case.label[1] if len(case.label) > 1 else ""
    assert labels[0].startswith(head) and labels[0].endswith(tail), (labels[0], case.label)


def _transform(case, a, g, sparse):
    if case.relu is None:
        return a, None, None
    scale, shift = X.pow2_transform(a.shape[1], g, sparse, case.relu)
    return X.apply_transform(a, scale, shift, case.relu), scale, shift


@pytest.mark.parametrize("role", ["a", "b"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_single_product_probe(case, role):
    """role b: the filter (weight gradients: dy) is sparse, the other operand dense randn; role a: the reverse"""
    op = X.OPS[case.op]
    g = torch.Generator().manual_seed(_seed(case, role))
    a, b, a_eff, scale, shift = X.build_probe(op, role, *case.shape, g, relu=case.relu)
    want, bound = X.exact(op, a_eff, b)
    got = _run(case, a, b, scale=scale, shift=shift)
    e, zeros_ok, worst = X.probe_error(got, want, bound)
    print(f"X3PROBE {case.id} role={role} e={e:.3f} worst={worst} nonzero={float((bound > 0).double().mean()):.2f}")
    assert zeros_ok, "an output no product reaches is not an exact zero"
    assert e <= E_MAX, (e, worst)


@pytest.mark.parametrize("case", [c for c in CASES if c.op in ("conv3x3", "conv1x1", "convt2x2")], ids=lambda c: c.id)
def test_bias_is_added_exactly(case):
    op = X.OPS[case.op]
    g = torch.Generator().manual_seed(_seed(case, "bias"))
    ash, bsh = X.shapes(op, *case.shape)
    a = torch.randn(ash, generator=g)
    _, scale, shift = _transform(case, a, g, False)
    bias = torch.randn(case.shape[4], generator=g)
    got = _run(case, a, torch.zeros(bsh), bias=bias, scale=scale, shift=shift)
    assert torch.equal(got, bias[None, :, None, None].expand_as(got))


@pytest.mark.parametrize("style", ["randn", "wide"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_dense_accumulation(case, style):
    op = X.OPS[case.op]
    g = torch.Generator().manual_seed(_seed(case, style))
    a, b = X.build_dense(op, style, *case.shape, g)
    if case.row in ("conv_stem", "wgrad_stem") and style == "wide":
        a[:, 3] = 0.0                  # the stem as the models run it: three channels padded with a zero fourth
    a_eff, scale, shift = _transform(case, a, g, False)
    want, bound = X.exact(op, a_eff, b)
    ref = X.dense_error(op.f(a_eff, b), want, bound)                     # torch-CPU float32 on the same inputs
    got = _run(case, a, b, scale=scale, shift=shift)
    assert torch.isfinite(got).all()
    dev = X.dense_error(got, want, bound)
    print(f"X3DENSE {case.id} style={style} device={dev:.3f} torch_f32={ref:.3f}")
    assert dev <= DENSE_MARGIN * ref, (dev, ref)
