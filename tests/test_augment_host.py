"""CPU-only: the host half of the training augmentation -- rfi_augment_params (the function the kernel evaluates per
sample) against the NumPy oracle tests/augment_ref.py, the statistics of the draw, the exact special cases, the oracle's
own warp against an independent interpolator, and argument validation."""
import ctypes as C

import numpy as np
import pytest

import augment_ref as R

SHAPES = [(5, 16, 24), (3, 17, 9), (2, 1, 7), (64, 32, 32)]
OFF = dict(p_hflip=0.0, p_vflip=0.0, p_rotate=0.0, p_ssr=0.0)


def _aug(**kw):
    from rfi_toolbox_amd.training import Augmenter
    return Augmenter(**kw)


@pytest.mark.parametrize("call", [3, (5 << 32) | 9])
@pytest.mark.parametrize("shape", SHAPES)
def test_params_match_oracle(shape, call):
    n, h, w = shape
    gates, inv = _aug(seed=7).params(n, h, w, call=call)
    want = R.draw(n, h, w, seed=7, call=call)
    assert gates.dtype == np.int32 and gates.shape == (n, 4) and inv.shape == (n, 6)
    np.testing.assert_array_equal(gates, want["gates"])
    err = np.abs(inv - want["inv"]).max()
    print(f"shape {shape} call {call}: max |inv - oracle| = {err:.3e}")
    assert err <= 1e-12
    # the closed form of the oracle is the inverse of M = SSR R Fv Fh built the long way round
    assert np.abs(want["inv"] - R.forward_inverse(want, h, w)).max() <= 1e-9


def test_gate_counts_and_parameter_ranges():
    n = 4096
    gates, _ = _aug(seed=11).params(n, 32, 48, call=0)
    counts = gates.sum(axis=0)
    print("gate counts", counts.tolist())
    assert np.all(np.abs(counts - 2048) <= 160)              # 5 sigma of Binomial(4096, 1/2)
    assert set(np.unique(gates)) <= {0, 1}
    p = R.draw(n, 32, 48, seed=11, call=0)
    np.testing.assert_array_equal(gates, p["gates"])
    assert np.abs(p["theta1"]).max() <= 15 and np.abs(p["theta2"]).max() <= 10
    assert np.abs(p["s"] - 1).max() <= np.float64(np.float32(0.05))
    assert np.abs(p["dx"]).max() <= np.float64(np.float32(0.05)) * 48 and np.abs(p["dy"]).max() <= np.float64(np.float32(0.05)) * 32
    on = p["gates"][:, 3] == 1                               # the draws do spread over their ranges, and only when gated on
    assert np.abs(p["theta2"][on]).max() > 9 and np.abs(p["dx"][on]).max() > 0.045 * 48 and np.all(p["dx"][~on] == 0)
    assert np.abs(p["theta1"][p["gates"][:, 2] == 1]).max() > 14 and np.all(p["theta1"][p["gates"][:, 2] == 0] == 0)
    # the library's map, taken apart: the linear part is a rotation times 1 / s with |angle| <= 25 degrees
    _, inv = _aug(seed=11).params(n, 32, 48, call=0)
    det = inv[:, 0] * inv[:, 4] - inv[:, 1] * inv[:, 3]
    flips = np.where(gates[:, 0] == 1, -1.0, 1.0) * np.where(gates[:, 1] == 1, -1.0, 1.0)
    assert np.all(det * flips > 0)
    scale = 1.0 / np.sqrt(np.abs(det))
    assert np.all(np.abs(scale - 1) <= np.float64(np.float32(0.05)) + 1e-12)
    angle = np.degrees(np.arctan2(np.abs(inv[:, 1]), np.abs(inv[:, 0])))
    assert angle.max() <= 25 + 1e-9


def test_exact_special_cases():
    gates, inv = _aug(seed=3, **OFF).params(9, 13, 21, call=4)
    assert not gates.any()
    np.testing.assert_array_equal(inv, np.tile([1.0, 0, 0, 0, 1.0, 0], (9, 1)))
    gates, inv = _aug(seed=3, **{**OFF, "p_hflip": 1.0}).params(9, 13, 21, call=4)
    np.testing.assert_array_equal(gates, np.tile([1, 0, 0, 0], (9, 1)))
    np.testing.assert_array_equal(inv, np.tile([-1.0, 0, 20.0, 0, 1.0, 0], (9, 1)))
    gates, inv = _aug(seed=3, **{**OFF, "p_vflip": 1.0}).params(2, 13, 22, call=4)
    np.testing.assert_array_equal(inv, np.tile([1.0, 0, 0, 0, -1.0, 12.0], (2, 1)))
    g0, i0 = _aug().params(0, 4, 4)
    assert g0.shape == (0, 4) and i0.shape == (0, 6)


def test_same_seed_and_call_reproduce_and_others_differ():
    a = _aug(seed=7).params(16, 32, 32, call=3)
    b = _aug(seed=7).params(16, 32, 32, call=3)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    for other in (_aug(seed=7).params(16, 32, 32, call=4), _aug(seed=8).params(16, 32, 32, call=3),
                  _aug(seed=7).params(16, 32, 32, call=3 + (1 << 32)), _aug(seed=7 + (1 << 32)).params(16, 32, 32, call=3)):
        assert not np.array_equal(a[1], other[1])
    assert np.array_equal(a[1][:8], _aug(seed=7).params(8, 32, 32, call=3)[1])       # sample i does not depend on n


def test_oracle_warp_against_an_independent_interpolator():
    """scipy's map_coordinates(order=1, mode="mirror") is the same bilinear / reflect-101 gather; without scipy the
    oracle's flip-only samples are checked against NumPy slicing."""
    x, y = R.inputs((64, 32, 32, 3))
    p = R.draw(64, 32, 32, seed=7, call=3)
    xo, yo, ties = R.warp(x, y, p)
    flip_only = (p["gates"][:, 2] == 0) & (p["gates"][:, 3] == 0)
    assert 8 <= flip_only.sum() <= 32 and not ties[flip_only].any()
    try:
        from scipy.ndimage import map_coordinates
    except ImportError:
        for i in np.flatnonzero(flip_only):
            gh, gv = p["gates"][i, :2]
            assert np.array_equal(xo[i], x[i][::-1 if gv else 1, ::-1 if gh else 1])
            assert np.array_equal(yo[i], y[i][::-1 if gv else 1, ::-1 if gh else 1])
        return
    worst = 0.0
    for i in range(64):
        sx, sy = R.source_positions(p["inv"][i], 32, 32)
        for c in range(3):
            want = map_coordinates(x[i, :, :, c].astype(np.float64), [sy, sx], order=1, mode="mirror")
            worst = max(worst, np.abs(xo[i, :, :, c] - want).max())
    print(f"oracle vs map_coordinates: max error {worst:.3e}")
    assert worst <= 2.0 ** -23 * np.abs(x).max()


def test_argument_validation_without_gpu():
    from rfi_toolbox_amd import _lib
    from rfi_toolbox_amd.training import Augmenter, train_rfi_model
    for bad in (dict(p_hflip=1.5), dict(p_ssr=-0.1), dict(rotate_limit=-1), dict(scale_limit=1.0), dict(shift_limit=float("nan")),
                dict(seed=-1), dict(seed=1.5), dict(p_rotate="0.5")):
        with pytest.raises(ValueError):
            Augmenter(**bad)
    a = Augmenter(seed=5, rotate_limit=20)
    with pytest.raises(ValueError):
        a.params(4, 0, 8)
    with pytest.raises(ValueError):
        a.params(4, 8, 8, call=-1)
    with pytest.raises(ValueError):                          # shapes are checked before any GPU call
        a(np.zeros((2, 8, 8), np.float32), np.zeros((2, 8, 8), np.uint8))
    with pytest.raises(ValueError):
        a(np.zeros((2, 8, 8, 17), np.float32), np.zeros((2, 8, 8), np.uint8))
    with pytest.raises(ValueError):
        a(np.zeros((2, 8, 8, 3), np.float32), np.zeros((2, 8, 9), np.uint8))
    with pytest.raises(ValueError):
        a(np.zeros((2, 8, 8, 3), np.float32), np.zeros((2, 8, 8), np.uint8), call=2 ** 64)
    with pytest.raises(ValueError):
        train_rfi_model(None, (np.zeros((2, 8, 8, 3), np.float32), np.zeros((2, 8, 8), np.uint8)), augment=True, augment_seed=-3)
    st = a.state_dict()
    assert st == {"seed": 5, "p_hflip": 0.5, "p_vflip": 0.5, "p_rotate": 0.5, "p_ssr": 0.5, "rotate_limit": 20.0,
                  "shift_limit": 0.05, "scale_limit": 0.05, "ssr_rotate_limit": 10.0}
    assert all(type(v) in (int, float) for v in st.values())
    b = Augmenter.from_state_dict(st)
    assert b.state_dict() == st and np.array_equal(a.params(6, 9, 9, call=2)[1], b.params(6, 9, 9, call=2)[1])
    # the C entry checks its own arguments (the usual error string)
    cfg = _lib.AugmentConfig(0, 0.5, 0.5, 2.0, 15, 0.5, 0.05, 0.05, 10)
    g, inv = np.zeros((1, 4), np.int32), np.zeros((1, 6))
    rc = _lib.lib.rfi_augment_params(C.byref(cfg), 0, 1, 4, 4, g.ctypes.data_as(C.POINTER(C.c_int32)),
                                     inv.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc != 0 and b"probabilities" in _lib.lib.rfi_last_error()
