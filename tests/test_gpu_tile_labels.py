"""-m gpu: inference.tile_labels (rfi_label_gather) bit for bit against the NumPy restatement of tests/tile_labels_ref.py,
and preprocessing.invalid_map against the definition.

test_tile_labels_matches_reference   B = 2, planes 37 x 50 and 10 x 12, ps = 16 at stride 16 and 12, views 1 / 2 / 4, edge pad /
                                     shift, invalid map none / per polarisation / per baseline, rule any / all, pad ignore / zero
test_input_kinds                     NumPy, torch and DeviceArray inputs, a bool map, a single (C, T) plane
test_rows_follow_tile_observation    the row count is tiling_count's and tile_observation's first axis
test_empty_observation               no baselines: an empty array
test_invalid_map                     prior flags or a non-finite part, (B, 4, C, T); feeds tile_labels
"""
import itertools

import numpy as np
import pytest
import torch

import tile_labels_ref as T
from rfi_toolbox_amd.inference import tile_labels, tile_observation, tiling_count
from rfi_toolbox_amd.preprocessing import invalid_map
from rfi_toolbox_amd.runtime import Context

pytestmark = pytest.mark.gpu

PS = 16
PLANES = ((37, 50), (10, 12))


def _planes(shape, seed=0):
    """label bytes below 0x80 over many values, a per-polarisation invalid map where any and all differ"""
    rng = np.random.default_rng(seed + shape[0] * shape[1])
    lab = rng.integers(0, 128, (2,) + shape, dtype=np.uint8)
    pol = (rng.random((2, 4) + shape) < 0.35).astype(np.uint8) * rng.integers(1, 256, (2, 4) + shape, dtype=np.uint8)
    assert pol.astype(bool).any(1).sum() > pol.astype(bool).all(1).sum() > 0
    return lab, pol


@pytest.mark.parametrize("shape", PLANES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_labels_matches_reference(shape):
    lab, pol = _planes(shape)
    base = pol[:, 0]
    for stride, views, edge in itertools.product((16, 12), (1, 2, 4), ("pad", "shift")):
        for invalid, rule in ((None, "any"), (pol, "any"), (pol, "all"), (base, "any"), (base, "all")):
            for pad in ("ignore", "zero"):
                got = tile_labels(lab, PS, stride=stride, views=views, edge=edge, invalid=invalid, invalid_rule=rule, pad=pad)
                want = T.tile(lab, PS, stride, views, edge, invalid, rule, 0x80 if pad == "ignore" else 0)
                assert got.shape == want.shape and got.dtype == np.uint8
                assert np.array_equal(got.numpy(), want), (stride, views, edge, rule, pad, invalid is not None)


def test_input_kinds():
    lab, pol = _planes(PLANES[0], seed=1)
    want = T.tile(lab, PS, 12, 4, "pad", pol, "any")
    ctx = Context.get(None)
    assert np.array_equal(tile_labels(torch.from_numpy(lab), PS, 12, 4, invalid=torch.from_numpy(pol)).numpy(), want)
    assert np.array_equal(tile_labels(torch.from_numpy(lab).cuda(), PS, 12, 4, invalid=torch.from_numpy(pol).cuda()).numpy(), want)
    dl, dp = ctx.to_device(lab), ctx.to_device(pol)
    assert np.array_equal(tile_labels(dl, PS, 12, 4, invalid=dp).numpy(), want)
    assert np.array_equal(dl.numpy(), lab) and np.array_equal(dp.numpy(), pol)          # the inputs are untouched
    m = lab[0] > 64
    assert np.array_equal(tile_labels(m, PS, invalid=pol[0].astype(bool)).numpy(), T.tile(m[None], PS, invalid=pol[:1]))


@pytest.mark.parametrize("shape", PLANES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rows_follow_tile_observation(shape):
    lab, _ = _planes(shape)
    rng = np.random.default_rng(3)
    vis = (rng.standard_normal((2, 4) + shape) + 1j * rng.standard_normal((2, 4) + shape)).astype(np.complex64)
    for stride, views, edge in ((16, 1, "pad"), (12, 4, "shift"), (12, 2, "pad")):
        y = tile_labels(lab, PS, stride=stride, views=views, edge=edge)
        x = tile_observation(vis, PS, stride=stride, views=views, edge=edge)
        assert y.shape[0] == x.shape[0] == 2 * tiling_count(shape[0], shape[1], PS, stride, views, edge)
        assert y.shape[1:] == x.shape[1:3]
    # the same tile order: a label plane equal to the data's sign pattern lands on the data's tiles
    sign = (vis[:, 0].real > 0).astype(np.uint8)
    y = tile_labels(sign, PS, stride=12, views=4, pad="zero").numpy()
    x = tile_observation(vis, PS, stride=12, views=4).numpy()
    assert np.array_equal(y, (x[..., 0] > 0).astype(np.uint8))


def test_empty_observation():
    out = tile_labels(np.zeros((0, 37, 50), np.uint8), PS, stride=12, views=4)
    assert out.shape == (0, PS, PS) and out.dtype == np.uint8 and out.numpy().size == 0


def test_invalid_map():
    shape = PLANES[1]
    rng = np.random.default_rng(4)
    vis = (rng.standard_normal((2, 4) + shape) + 1j * rng.standard_normal((2, 4) + shape)).astype(np.complex64)
    vis[0, 1, 2, 3] = np.nan
    vis[1, 3, 0, 5] = complex(0.0, np.inf)
    prior = rng.random((2, 4) + shape) < 0.2
    bad = ~(np.isfinite(vis.real) & np.isfinite(vis.imag))
    for flags, want in ((None, bad), (prior, bad | prior), (prior[:, 0], bad | prior[:, :1])):
        got = invalid_map(vis, flags)
        assert got.shape == (2, 4) + shape and got.dtype == np.uint8
        assert np.array_equal(got.numpy() != 0, want)
    inv = invalid_map(vis, prior)
    lab = rng.integers(0, 128, (2,) + shape, dtype=np.uint8)
    assert np.array_equal(tile_labels(lab, PS, invalid=inv).numpy(), T.tile(lab, PS, invalid=bad | prior))
