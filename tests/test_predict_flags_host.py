"""CPU-only: the tiling rules of whole-observation prediction (tests/stitch_ref.py) against the reference's own
tiling (stitch_ref.reference_patch_table), rfi_tiling_count and rfi_tiling_table, and the argument checks that need no
model."""
import numpy as np
import pytest

import stitch_ref as ref

SHAPES = [(40, 40), (64, 64), (128, 64), (64, 128), (65, 64), (129, 257), (200, 333), (333, 200), (30, 100),
          (100, 30), (192, 128), (1, 64)]
BAD_TILINGS = [(64, 0, 0, 1), (64, 65, 0, 1), (64, 64, 2, 1), (64, 64, 0, 3), (0, 1, 0, 1)]


@pytest.mark.parametrize("views", [1, 2, 4])
@pytest.mark.parametrize("shape", SHAPES)          # (C, T <= ps: whole, unpadded waterfalls, one entry per view)
def test_stride_ps_pad_equals_reference_patch_table(shape, views):
    from rfi_toolbox_amd.inference import tiling_table
    from rfi_toolbox_amd.preprocessing.preprocessor import _patch_table
    C, T = shape
    ps = 64
    got = ref.patch_table(3, C, T, ps, ps, views, "pad")
    want = ref.reference_patch_table(3, C, T, views, ps)
    assert np.array_equal(got, want)
    assert np.array_equal(_patch_table(3, C, T, views, ps), want)          # the Preprocessor's table
    lib = tiling_table(3, C, T, ps, ps, views, "pad")
    assert lib.dtype == np.int32 and lib.flags.c_contiguous and np.array_equal(lib, want)


@pytest.mark.parametrize("edge", ["pad", "shift"])
@pytest.mark.parametrize("stride", [64, 48, 32, 1])
@pytest.mark.parametrize("views", [1, 2, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_tiling_table_is_the_restatement(shape, views, stride, edge):
    from rfi_toolbox_amd.inference import tiling_table
    C, T = shape
    for n_units in (1, 3):
        got = tiling_table(n_units, C, T, 64, stride, views, edge)
        assert got.dtype == np.int32 and got.flags.c_contiguous
        assert np.array_equal(got, ref.patch_table(n_units, C, T, 64, stride, views, edge))
    assert tiling_table(0, C, T, 64, stride, views, edge).shape == (0, 4)


def test_tiling_table_rejects_small_capacity_and_bad_tilings():
    from rfi_toolbox_amd import _lib
    import ctypes as C
    good = _lib.Tiling(64, 32, 0, 2)
    n = C.c_int64()
    assert _lib.lib.rfi_tiling_count(100, 130, C.byref(good), C.byref(n)) == 0
    buf = np.full((3 * n.value + 1, 4), -7, dtype=np.int32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert _lib.lib.rfi_tiling_table(100, 130, C.byref(good), 3, ptr, 3 * n.value - 1) != 0
    assert _lib.lib.rfi_last_error() and np.all(buf == -7)                  # too small: an error, nothing written
    assert _lib.lib.rfi_tiling_table(100, 130, C.byref(good), 3, ptr, 3 * n.value) == 0
    assert np.array_equal(buf[:-1], ref.patch_table(3, 100, 130, 64, 32, 2, "pad")) and np.all(buf[-1] == -7)
    assert _lib.lib.rfi_tiling_table(100, 130, C.byref(good), 0, None, 0) == 0
    for t in BAD_TILINGS:
        assert _lib.lib.rfi_tiling_table(100, 100, C.byref(_lib.Tiling(*t)), 1, ptr, len(buf)) != 0
        assert _lib.lib.rfi_last_error()


@pytest.mark.parametrize("edge", ["pad", "shift"])
@pytest.mark.parametrize("stride", [64, 48, 32, 1])
@pytest.mark.parametrize("views", [1, 2, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_tiling_count_agrees(shape, views, stride, edge):
    from rfi_toolbox_amd.inference import tiling_count
    C, T = shape
    assert tiling_count(C, T, 64, stride, views, edge) == ref.patches_per_plane(C, T, 64, stride, views, edge) \
        == len(ref.patch_table(1, C, T, 64, stride, views, edge))


@pytest.mark.parametrize("stride", [64, 48, 32, 7])
@pytest.mark.parametrize("shape", SHAPES)
def test_edge_shift_leaves_no_padded_tile_and_covers_everything(shape, stride):
    C, T = shape
    ps = 64
    for views in (1, 4):
        for p, v, r0, c0 in ref.patch_table(1, C, T, ps, stride, views, "shift"):
            hv, wv = (T, C) if v >= 2 else (C, T)
            assert r0 + ps <= max(hv, ps) and c0 + ps <= max(wv, ps)
    for edge in ("pad", "shift"):
        for L in shape:
            o = ref.origins(L, ps, stride, edge)
            cover = np.zeros(L, dtype=int)
            for a in o:
                cover[a:a + ps] += 1
            assert cover.min() >= 1 and o == sorted(o) and len(set(o)) == len(o)


def test_restated_stitch_inverts_the_cut():
    """cut -> stitch of probabilities gives the plane back where it was a probability map."""
    rng = np.random.default_rng(0)
    planes = rng.random((2, 70, 90)).astype(np.float32)
    for views in (1, 2, 4):
        for stride, edge in ((32, "pad"), (32, "shift"), (20, "pad")):
            pt = ref.cut(planes, ref.patch_table(2, 70, 90, 32, stride, views, edge), 32)
            _, out = ref.stitch(pt, 2, 70, 90, 32, stride, views, edge, "max", logits=False)
            assert np.array_equal(out, planes)
            _, out = ref.stitch(pt, 2, 70, 90, 32, stride, views, edge, "mean", logits=False)
            assert np.allclose(out, planes, atol=1e-6)


def test_tiling_count_rejects_bad_tilings():
    from rfi_toolbox_amd import _lib
    import ctypes as C
    n = C.c_int64()
    for t in BAD_TILINGS:
        assert _lib.lib.rfi_tiling_count(100, 100, C.byref(_lib.Tiling(*t)), C.byref(n)) != 0
        assert _lib.lib.rfi_last_error()


def test_argument_errors_without_a_model():
    from rfi_toolbox_amd.inference import predict_flags
    z = np.zeros((2, 64, 64), dtype=np.complex64)
    with pytest.raises(ValueError, match="reconstruct_flags"):
        predict_flags(None, np.zeros((2, 64, 64), dtype=np.float32))
    with pytest.raises(ValueError, match="shape"):
        predict_flags(None, np.zeros((64, 64), dtype=np.complex64))
    with pytest.raises(ValueError, match="shape"):
        predict_flags(None, np.zeros((1, 1, 1, 64, 64), dtype=np.complex64))
    for kw in ({"stride": 0}, {"stride": 65}, {"stride": 1.5}, {"views": 3}, {"combine": "median"}, {"edge": "wrap"},
               {"patch_size": 0}, {"batch_size": 0}):
        with pytest.raises(ValueError):
            predict_flags(None, z, patch_size=kw.pop("patch_size", 64), **kw)
    with pytest.raises(TypeError):
        predict_flags(object(), z, patch_size=64)


def test_reconstruct_flags_needs_an_inference_dataset():
    from rfi_toolbox_amd.preprocessing import Preprocessor
    with pytest.raises(ValueError, match="inference_mode"):
        Preprocessor(np.zeros((1, 8, 8), dtype=np.complex64)).reconstruct_flags(np.zeros((1, 8, 8)))
