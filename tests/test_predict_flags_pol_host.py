"""CPU-only: the argument checks of the 8-channel whole-observation path that touch no device, and the invariants
of its NumPy restatement (tests/pol_tiling_ref.py)."""
import numpy as np
import pytest

import normalize_ref as nref
import pol_tiling_ref as pref
import stitch_ref as sref


def _stub(in_channels, out_channels=1):
    """A model object with the attributes the argument checks read; it owns nothing on a device."""
    from rfi_toolbox_amd.models import UNet
    m = object.__new__(UNet)
    m.in_channels, m.out_channels, m.depth = in_channels, out_channels, 4
    return m


def _data(shape, dtype=np.complex64, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


def test_new_functions_are_exported():
    from rfi_toolbox_amd import inference
    assert {"predict_flags", "tile_observation", "stitch_patches"} <= set(inference.__all__)


def test_predict_flags_argument_errors_touch_no_device():
    from rfi_toolbox_amd.inference import predict_flags
    from rfi_toolbox_amd.preprocessing import Normalizer
    m8, m3 = _stub(8), _stub(3)
    for shape in ((2, 2, 64, 64), (3, 64, 64), (1, 8, 64, 64)):           # not 4 polarisations
        with pytest.raises(ValueError, match="channel"):
            predict_flags(m8, _data(shape), patch_size=32)
    with pytest.raises(ValueError, match="reconstruct_flags"):            # real data
        predict_flags(m8, np.zeros((1, 4, 64, 64), dtype=np.float32), patch_size=32)
    with pytest.raises(ValueError, match="8 input channels"):             # the new keywords with a 3-channel model
        predict_flags(m3, _data((1, 4, 64, 64)), patch_size=32, normalizer=Normalizer("standardize", "sample"))
    with pytest.raises(ValueError, match="8 input channels"):
        predict_flags(m3, _data((1, 4, 64, 64)), patch_size=32, broadcast_pols=False)
    with pytest.raises(RuntimeError, match="fit"):                        # unfitted dataset-scope normalizer
        predict_flags(m8, _data((1, 4, 64, 64)), patch_size=32, normalizer=Normalizer("standardize", "dataset"))
    with pytest.raises(TypeError):
        predict_flags(m8, _data((1, 4, 64, 64)), patch_size=32, normalizer="standardize")
    for m in (m8, m3):
        with pytest.raises(ValueError, match="out"):
            predict_flags(m, _data((1, 4, 64, 64)), patch_size=32, out="cuda")
    for args in ((1, 1), (3, 2), (8, 2)):                                 # other models: the wording the GPU test matches
        with pytest.raises(ValueError, match="channel"):
            predict_flags(_stub(*args), _data((1, 4, 64, 64)), patch_size=32)
    with pytest.raises(ValueError, match="multiple"):
        predict_flags(m8, _data((1, 4, 64, 64)), patch_size=40)


def test_tile_and_stitch_argument_errors_touch_no_device():
    from rfi_toolbox_amd.inference import stitch_patches, tile_observation
    from rfi_toolbox_amd.preprocessing import Normalizer
    with pytest.raises(ValueError, match="channel"):
        tile_observation(_data((2, 3, 40, 40)), 32)
    with pytest.raises(ValueError, match="complex"):
        tile_observation(np.zeros((2, 4, 40, 40)), 32)
    with pytest.raises(RuntimeError, match="fit"):
        tile_observation(_data((2, 4, 40, 40)), 32, normalizer=Normalizer("robust_scale", "dataset"))
    with pytest.raises(ValueError):
        tile_observation(_data((2, 4, 40, 40)), 32, stride=33)
    with pytest.raises(ValueError, match="values"):
        stitch_patches(np.zeros((4, 32, 16), dtype=np.float32), 40, 40, 32)
    with pytest.raises(ValueError, match="whole number"):
        stitch_patches(np.zeros((5, 32, 32), dtype=np.float32), 40, 40, 32)          # 4 patches per 40 x 40 plane
    with pytest.raises(ValueError):
        stitch_patches(np.zeros((4, 32, 32), dtype=np.float32), 40, 40, 32, combine="median")


def test_python_patch_table_is_the_restatement():
    from rfi_toolbox_amd.inference import tiling_table
    for C, T in ((50, 77), (77, 50), (20, 70), (64, 64), (65, 63), (20, 20)):
        for stride in (32, 24, 16):
            for views in (1, 2, 4):
                for edge in ("pad", "shift"):
                    assert np.array_equal(tiling_table(3, C, T, 32, stride, views, edge),
                                          sref.patch_table(3, C, T, 32, stride, views, edge)), (C, T, stride, views, edge)


def test_sample_groups_are_whole_baselines(monkeypatch):
    from rfi_toolbox_amd import inference
    assert inference._SAMPLE_GROUP_BYTES == 256 << 20
    assert inference._sample_groups(5, 1000) == [(0, 5)]
    assert inference._sample_groups(10000, 8)[:2] == [(0, 4096), (4096, 8192)]        # at most 4096 baselines
    monkeypatch.setattr(inference, "_SAMPLE_GROUP_BYTES", 2500)
    assert inference._sample_groups(5, 1000) == [(0, 2), (2, 4), (4, 5)]
    assert inference._sample_groups(3, 5000) == [(0, 1), (1, 2), (2, 3)]              # at least one


# ---------------------------------------------------------------- the restatement's own invariants
@pytest.mark.parametrize("edge", ["pad", "shift"])
@pytest.mark.parametrize("stride", [32, 24])
def test_identity_pair_and_one_view_is_the_raw_cut(stride, edge):
    data = _data((3, 4, 50, 77), np.complex64, seed=1)
    got = pref.tile(data, [(0.0, 1.0)] * 3, 32, stride, 1, edge)
    table = sref.patch_table(3, 50, 77, 32, stride, 1, edge)
    for pol in range(4):
        assert np.array_equal(got[..., 2 * pol], sref.cut(data[:, pol].real, table, 32))
        assert np.array_equal(got[..., 2 * pol + 1], sref.cut(data[:, pol].imag, table, 32))


def test_padding_is_a_normalised_zero_visibility():
    data = _data((2, 4, 20, 40), np.complex128, seed=2) + (3 - 2j)
    pairs = [(1.5, 4.0), (-2.0, 0.25)]
    got = pref.tile(data, pairs, 32, views=4)
    table = sref.patch_table(2, 20, 40, 32, None, 4, "pad")
    for e, (p, v, r0, c0) in enumerate(table):
        hv, wv = (40, 20) if v >= 2 else (20, 40)
        pad = np.ones((32, 32), dtype=bool)
        pad[:max(0, hv - r0), :max(0, wv - c0)] = False
        assert pad.any() and np.all(got[e][pad] == np.float32((0.0 - pairs[p][0]) / pairs[p][1]))
    assert pref.pad_value(None) == 0 and pref.pad_value((3.0, 0.0)) == 0
    assert np.all(pref.tile(data, [None, None], 32) == 0)


def test_views_are_views_of_the_first():
    """tile k of view v is view_of applied to the whole normalised plane: square planes, one tile per view."""
    data = _data((1, 4, 32, 32), seed=3)
    t = pref.tile(data, [(0.25, 2.0)], 32, views=4)
    assert t.shape == (4, 32, 32, 8)
    assert np.array_equal(t[1], t[0][::-1]) and np.array_equal(t[2], t[0].transpose(1, 0, 2))
    assert np.array_equal(t[3], t[0].transpose(1, 0, 2)[::-1])


def test_pairs_follow_the_normalisation_restatement():
    data = _data((3, 4, 24, 40), seed=4) * np.array([1.0, 7.5, 0.02]).reshape(3, 1, 1, 1)
    for method in nref.METHODS:
        sample = pref.pairs_of(data, method, "sample")
        assert len({p for p in sample}) == 3                                   # every baseline its own
        assert np.array_equal(pref.normalise(data, sample), nref.normalize_samples(data, method))
        ds = pref.pairs_of(data, method, "dataset")
        assert len(set(ds)) == 1
        assert np.array_equal(pref.normalise(data, ds), nref.normalize_dataset([data], method)[1][0])
    assert pref.pairs_of(data, None, "sample") == [(0.0, 1.0)] * 3
    assert pref.broadcast(np.zeros((3, 5, 6), dtype=bool)).shape == (3, 4, 5, 6)
    assert pref.broadcast(np.zeros((5, 6), dtype=bool)).shape == (4, 5, 6)
