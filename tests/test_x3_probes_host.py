"""The single-product probes of tests/x3_ref.py, pinned on the CPU (no GPU): what test_gpu_x3_accuracy.py asserts of a
kernel is only worth something if a subtly wrong kernel would miss it.  For every builder, on the CPU emulation of the
float32-by-3xbf16 scheme:

* at most ONE non-zero product meets in any output (counted with the operation on the non-zero masks);
* at least 80 % of the outputs any operands can reach are non-zero -- of the attainable maximum, where the geometry of
  an operation caps it (Op.cover: the sparse-dy probe of the strided 3x3 input gradient cannot pass 9/16);
* the six-product scheme gives e <= 2 (2^-24 units), torch float32 itself e <= 1 (one rounding of one product);
* every defect variant (one piece product missing, or the third piece dropped altogether) gives e >= 64.

The 16 the device tests assert lies between the two with a factor 4 on either side."""
import zlib

import pytest
import torch

import x3_ref as X
from x3_cases import CASES as DEVICE_CASES, ROWS

# (op, n, h, w, cin, cout): small shapes, ragged sizes, both a partial and whole 16-chunks of channels
CASES = [
    ("conv3x3", 2, 13, 18, 32, 48), ("conv3x3", 1, 16, 16, 4, 32), ("conv3x3_dgrad", 2, 12, 17, 32, 48),
    ("conv1x1", 2, 7, 9, 48, 40), ("convt2x2", 2, 6, 7, 32, 32), ("convt2x2_dgrad", 2, 6, 7, 32, 48),
    ("conv_s2_k3", 2, 12, 16, 16, 32), ("conv_s2_k1", 2, 12, 16, 16, 32), ("conv_s2_k3_dgrad", 2, 12, 16, 16, 32),
    ("conv_s2_k1_dgrad", 2, 12, 16, 16, 32),
    ("conv3x3_wgrad", 3, 12, 19, 32, 48), ("conv3x3_wgrad", 2, 16, 16, 4, 32), ("convt2x2_wgrad", 3, 6, 9, 32, 48),
    ("conv_s2_k3_wgrad", 3, 12, 16, 16, 32), ("conv_s2_k1_wgrad", 3, 12, 16, 16, 32),
]
XFORM_CASES = [("conv3x3", 2, 13, 18, 32, 48), ("conv1x1", 2, 7, 9, 48, 40), ("conv3x3_wgrad", 3, 12, 19, 32, 48)]


def _check(op, role, a_eff, b):
    assert float(X.products_per_output(op, a_eff, b).max()) <= 1.0, "two products meet in one output"
    want, bound = X.exact(op, a_eff, b)
    cov = X.coverage(op, a_eff, b, bound)
    assert cov >= 0.8 * op.cover[role], f"only {cov:.2f} of the reachable outputs are non-zero"
    e32, zeros_ok, _ = X.probe_error(op.f(a_eff, b), want, bound)
    assert zeros_ok and e32 <= 1.0, e32
    e6, zeros_ok, _ = X.probe_error(X.emulate(op, a_eff, b, "six"), want, bound)
    assert zeros_ok and e6 <= 2.0, e6
    worst = {}
    for v in X.VARIANTS:
        if v != "six":
            worst[v], zeros_ok, _ = X.probe_error(X.emulate(op, a_eff, b, v), want, bound)
            assert zeros_ok
    assert min(worst.values()) >= 64.0, worst
    return cov, e6, worst


@pytest.mark.parametrize("role", ["a", "b"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_probe_separates_the_scheme_from_its_defects(case, role):
    op = X.OPS[case[0]]
    g = torch.Generator().manual_seed(len(case[0]) + sum(case[1:]))
    a, b, a_eff, _, _ = X.build_probe(op, role, *case[1:], g)
    assert a_eff is a
    _check(op, role, a, b)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("role", ["a", "b"])
@pytest.mark.parametrize("case", XFORM_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_probe_behind_the_load_transform(case, role, relu):
    """the expected product is formed from relu(x * scale + shift) in float32: scales are signed powers of two, some
    negative, and with the ReLU part of the non-zero elements end up as zeros"""
    op = X.OPS[case[0]]
    g = torch.Generator().manual_seed(3 + sum(case[1:]) + relu)
    a, b, a_eff, scale, shift = X.build_probe(op, role, *case[1:], g, relu=relu)
    assert (scale < 0).any() and (torch.log2(scale.abs()) % 1 == 0).all()
    assert torch.equal(a.double() * scale.double()[None, :, None, None], (a * scale[None, :, None, None]).double())
    if relu:
        assert ((a != 0) & (a_eff == 0)).any(), "no non-zero element went through the ReLU"
    if role == "a":
        assert not ((a == 0) & (a_eff != 0)).any(), "the transform filled the zeros of the sparse operand"
    _check(op, role, a_eff, b)


@pytest.mark.parametrize("role", ["a", "b"])
@pytest.mark.parametrize("case", DEVICE_CASES, ids=lambda c: c.id)
def test_every_device_case_tests_something(case, role):
    """the very operands test_gpu_x3_accuracy.py sends to the device (same seeds): one product per output at most, and
    80 % of the reachable outputs non-zero (of the attainable maximum)"""
    op = X.OPS[case.op]
    g = torch.Generator().manual_seed(zlib.crc32(f"{case.id}/{role}".encode()))
    a, b, a_eff, _, _ = X.build_probe(op, role, *case.shape, g, relu=case.relu)
    assert float(X.products_per_output(op, a_eff, b).max()) <= 1.0
    cov = X.coverage(op, a_eff, b, X.exact(op, a_eff, b)[1])
    assert cov >= 0.8 * op.cover[role], cov


def test_device_cases_cover_every_row():
    assert {c.row for c in DEVICE_CASES} == set(ROWS) and len({c.id for c in DEVICE_CASES}) == len(DEVICE_CASES)
    for c in DEVICE_CASES:                  # the load transform exists on three entry points only
        assert c.relu is None or c.op in ("conv3x3", "conv1x1", "conv3x3_wgrad"), c.id


@pytest.mark.parametrize("name", [n for n, o in X.OPS.items() if o.kind == "conv"])
def test_sparse_filter_walks_every_k_slot_and_tap(name):
    op = X.OPS[name]
    bsh = X.shapes(op, 1, 8, 8, 32, 48)[1]
    wt = X.sparse_filter(op, bsh, torch.Generator().manual_seed(1))
    nz = torch.nonzero(wt)
    assert set((nz[:, 1 - op.out_axis] % 16).tolist()) == set(range(16))
    assert {(int(r), int(s)) for r, s in nz[:, 2:]} == {t for cls in op.tap_classes for t in cls}
    per_out = torch.bincount(nz[:, op.out_axis], minlength=bsh[op.out_axis])
    assert (per_out == len(op.tap_classes)).all()


def test_sparse_pixels_reach_corners_images_and_every_class():
    t = X.sparse_pixels((3, 32, 10, 13), X.PARITIES, torch.Generator().manual_seed(2))
    assert t[0, 0, 0, 0] != 0 and t[2, 31, 9, 11] != 0             # (last channel, class (1, 1): the last corner)
    nz = torch.nonzero(t)
    assert set(nz[:, 0].tolist()) == {0, 1, 2}
    border = (nz[:, 2] == 0) | (nz[:, 2] == 9) | (nz[:, 3] == 0) | (nz[:, 3] == 12)
    assert 2 <= int(border.sum()) <= len(nz) // 4
    for c in range(32):
        assert {(int(y) % 2, int(x) % 2) for _, _, y, x in nz[nz[:, 1] == c]} == set(X.PARITIES)


def test_dense_builders_hold_exactly_cancelling_pairs():
    """'wide': for the first quarter of the output channels every term has a partner that cancels it exactly"""
    for name in ("conv3x3", "conv3x3_dgrad", "convt2x2", "convt2x2_dgrad", "conv3x3_wgrad", "convt2x2_wgrad"):
        op = X.OPS[name]
        a, b = X.build_dense(op, "wide", 2, 8, 8, 16, 32, torch.Generator().manual_seed(5))
        want, bound = X.exact(op, a, b)
        axis = 1 if op.kind == "conv" or name == "convt2x2_wgrad" else 0      # the output-channel axis of the result
        nq = want.shape[axis] // 4
        w0, b0 = want.narrow(axis, 0, nq), bound.narrow(axis, 0, nq)
        assert float(b0.min()) > 0 and bool((w0.abs() <= 2.0 ** -40 * b0).all()), name      # (float64 residues only)
        assert float((want.abs() / bound).narrow(axis, nq, nq).max()) > 1e-3, name           # ... and only there
