"""-m gpu: on-device Preprocessor hot loop and confusion counts against the golden vectors."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import metrics_ref, preprocess_ref
from rfi_toolbox_amd.evaluation import confusion_counts, evaluate_segmentation
from rfi_toolbox_amd.preprocessing import Preprocessor, patchify

pytestmark = pytest.mark.gpu


def _g(golden_dir):
    return np.load(os.path.join(golden_dir, "preprocess.npz"))


def test_patchify_known_answer():
    p = patchify(np.arange(16).reshape(4, 4), (2, 2), 2)      # reference tests/test_preprocessing.py:22-33
    assert p.shape == (2, 2, 2, 2)
    np.testing.assert_array_equal(p[0, 0], [[0, 1], [4, 5]])
    np.testing.assert_array_equal(p[1, 1], [[10, 11], [14, 15]])
    assert patchify(np.zeros((1024, 1024), np.float32), (128, 128), 128).shape == (8, 8, 128, 128)
    assert patchify(np.zeros((256, 512)), (128, 128), 128).shape == (2, 4, 128, 128)
    assert patchify(np.zeros((4, 4), np.complex64), (2, 2), 2).dtype == np.complex64


def test_create_dataset_complex_golden(golden_dir):
    g = _g(golden_dir)
    np.random.seed(7)
    ds = Preprocessor(g["a_w"], flags=g["a_m"]).create_dataset(patch_size=64, num_workers=0)
    assert ds.images.dtype == torch.float32 and ds.labels.dtype == torch.uint8
    assert tuple(ds.images.shape) == (4, 64, 64, 3)
    np.testing.assert_allclose(ds.images.numpy(), g["a_img"], rtol=0, atol=2e-6)
    np.testing.assert_array_equal(ds.labels.numpy(), g["a_lab"])
    np.random.seed(8)
    ds = Preprocessor(g["b_w"], flags=g["b_m"]).create_dataset(patch_size=32, num_workers=0)
    np.testing.assert_allclose(ds.images.numpy(), g["b_img"], rtol=0, atol=2e-6)
    np.testing.assert_array_equal(ds.labels.numpy(), g["b_lab"])
    ds = Preprocessor(g["b_w"], flags=g["b_m"]).create_dataset(patch_size=32, enable_augmentation=False,
                                                               inference_mode=True)
    np.testing.assert_allclose(ds.images.numpy(), g["b2_img"], rtol=0, atol=2e-6)
    assert ds.labels.sum() == 0
    np.random.seed(9)
    ds = Preprocessor(g["b_w"], flags=g["b_m"]).create_dataset(patch_size=32, augmentation_rotations=2,
                                                               num_patches=10)
    np.testing.assert_allclose(ds.images.numpy(), g["b3_img"], rtol=0, atol=2e-6)
    np.testing.assert_array_equal(ds.labels.numpy(), g["b3_lab"])
    item = ds[0]
    assert set(item) == {"image", "label"} and tuple(item["image"].shape) == (32, 32, 3)


@pytest.mark.parametrize("tag,kw", [("c_sqrt", dict(stretch="SQRT")),
                                    ("c_log", dict(stretch="LOG10", normalize_after_stretch=True)),
                                    ("c_none", dict(stretch=None, normalize_before_stretch=False))])
def test_create_dataset_real_golden(golden_dir, tag, kw):
    g = _g(golden_dir)
    np.random.seed(10)
    ds = Preprocessor(g["c_w"], flags=None).create_dataset(patch_size=32, flag_sigma=5, **kw)
    np.testing.assert_allclose(ds.images.numpy(), g[f"{tag}_img"], rtol=0, atol=3e-6)
    np.testing.assert_array_equal(ds.labels.numpy(), g[f"{tag}_lab"])


def test_edge_patches_and_dtypes(golden_dir):
    g = _g(golden_dir)
    p = Preprocessor(np.zeros((1, 1, 8, 8), np.complex128))
    mean, std = preprocess_ref.IMAGENET_MEAN, preprocess_ref.IMAGENET_STD
    for src, want in (("d_z", "d_z_ch"), ("d_zc", "d_zc_ch"), ("d_zz", "d_zz_ch")):
        got = p._channels_on_device(g[src][None])[0]
        np.testing.assert_allclose(got, (g[want].astype(np.float32) - mean) / std, rtol=0, atol=2e-6)
    z64 = g["d_z"].astype(np.complex64)                      # complex64 / float32 inputs: fp32 math
    got = p._channels_on_device(z64[None])[0]
    want = preprocess_ref.images_of(preprocess_ref.channels(z64[None]))[0]
    err_ref = np.abs(preprocess_ref.images_of(preprocess_ref.channels_f32(z64[None]))[0].astype(np.float64) - want).max(axis=(0, 1))
    err = np.abs(got.astype(np.float64) - want).max(axis=(0, 1))
    # what float32 arithmetic costs NumPy itself on this patch, times 4 for log10f / atan2f / hypotf, per channel; over the
    # complex64 cases of test_gpu_preprocess_kernels.py an MI355X gave err_ref <= 9.5e-7 and a device error <= 1.2e-6
    assert (err <= np.maximum(4.0 * err_ref, 2e-6)).all(), (err, err_ref)
    with pytest.raises(ValueError):
        Preprocessor(np.zeros((4, 4)))
    with pytest.raises(ValueError):
        Preprocessor(np.ones((1, 1, 8, 8))).create_dataset(patch_size=8, stretch="CBRT")
    assert len(Preprocessor(np.zeros((1, 0, 8, 8), np.complex128)).data[0]) == 0


def test_metrics_golden(golden_dir):
    exp = json.load(open(os.path.join(golden_dir, "metrics_expected.json")))
    inp = np.load(os.path.join(golden_dir, "metrics_inputs.npz"))
    for name, want in exp.items():
        got = evaluate_segmentation(inp[f"{name}/pred"], inp[f"{name}/true"])
        for k in want:
            assert got[k] == pytest.approx(want[k], abs=1e-15), (name, k)
    got = evaluate_segmentation(torch.from_numpy(inp["torch_n1hw/pred"]), torch.from_numpy(inp["torch_n1hw/true"]))
    assert got["iou"] == pytest.approx(exp["torch_n1hw"]["iou"], abs=1e-15)


def test_metrics_large_and_empty():
    rng = np.random.default_rng(0)
    a = rng.random(64 * 128 * 128) > 0.7
    b = rng.random(64 * 128 * 128) > 0.6
    assert confusion_counts(a, b) == metrics_ref.confusion(a, b)
    assert confusion_counts(np.zeros(0, np.uint8), np.zeros(0, np.uint8)) == (0, 0, 0)
    assert evaluate_segmentation(np.zeros(0), np.zeros(0)) == {"iou": 1.0, "precision": 1.0, "recall": 1.0,
                                                              "f1": 1.0, "dice": 1.0}
    with pytest.raises(ValueError):
        confusion_counts(np.zeros(3), np.zeros(4))


# ------------------------------------------------------------------ views / tiling / blank-patch test on device
def _wf(shape, dtype, seed, frac=0.02):
    rng = np.random.default_rng(seed)
    z = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(dtype)
    fl = rng.random(shape) < frac
    fl[..., : shape[-2] // 3, :] = False           # leaves some tiles blank
    return z, fl


@pytest.mark.parametrize("shape,dtype,ps,kw", [
    ((1, 1, 128, 128), np.complex128, 128, {}),
    ((2, 2, 200, 300), np.complex64, 128, {}),
    ((1, 3, 256, 130), np.complex128, 64, {"augmentation_rotations": 2}),
    ((1, 1, 256, 256), np.complex128, 128, {"enable_augmentation": False}),
    ((1, 2, 300, 200), np.complex128, 128, {"num_patches": 5}),
    ((1, 1, 64, 64), np.complex128, 128, {}),
    ((1, 1, 256, 256), np.complex128, 128, {"inference_mode": True}),
])
def test_device_tiling_equals_host_bookkeeping(shape, dtype, ps, kw):
    """The gather form (views, zero-padded tiling, blank-patch removal and labels resolved on the GPU
    from the waterfall) must give the very dataset the host-bookkeeping form gives -- same patch
    order under the same global-RNG seed, bit-identical images and labels."""
    z, fl = _wf(shape, dtype, seed=sum(shape) + ps)
    np.random.seed(99)
    a = Preprocessor(z, flags=fl).create_dataset(patch_size=ps, num_workers=0, on_device_tiling=False, **kw)
    np.random.seed(99)
    pre = Preprocessor(z, flags=fl)
    b = pre.create_dataset(patch_size=ps, num_workers=0, **kw)
    assert pre._table is not None                                       # the device path really ran
    assert tuple(a.images.shape) == tuple(b.images.shape) and len(a) > 0
    assert torch.equal(a.labels, b.labels)
    assert torch.equal(a.images, b.images)
    assert a.metadata == b.metadata
    patches, pflags = pre.materialise_patches()
    if not kw.get("inference_mode"):
        np.testing.assert_array_equal(pflags.astype(np.uint8), b.labels.numpy())
    assert patches.shape == tuple(b.labels.shape)


# ------------------------------------------------------------------ order-statistic branches on the GPU
@pytest.mark.parametrize("kw", [dict(stretch="SQRT"), dict(stretch="LOG10", normalize_after_stretch=True),
                                dict(stretch=None), dict(stretch="LOG10", normalize_before_stretch=False)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_real_input_branch_on_device_equals_host(kw, dtype):
    """Median normalise / stretch / MAD flags / channels for REAL input on the GPU (exact order statistics
    by radix selection) against the NumPy form of the same steps -- with zeros (log10 -> -inf, replaced by
    the MAD of the finite values), NaNs (skipped by nanmedian) and negative values in the data."""
    rng = np.random.default_rng(5)
    x = rng.lognormal(0.0, 1.0, size=(1, 2, 96, 64)).astype(dtype)
    x[0, 0, 3:5, 10:40] = 0.0
    x[0, 1, 50, 7] = np.nan
    x[0, 1, 20:22, :] *= -1.0
    x[0, 0, 70:72, 30:34] *= 500.0
    np.random.seed(3)
    a = Preprocessor(x).create_dataset(patch_size=32, flag_sigma=4, on_device_tiling=False, **kw)
    np.random.seed(3)
    b = Preprocessor(x).create_dataset(patch_size=32, flag_sigma=4, **kw)      # float32: float32 arithmetic on the device too
    assert len(a) == len(b) > 0
    np.testing.assert_array_equal(a.labels.numpy(), b.labels.numpy())
    np.testing.assert_allclose(a.images.numpy(), b.images.numpy(), rtol=0, atol=2e-6, equal_nan=True)
    # with caller-supplied flags the MAD step is skipped and the labels are the tiled flags
    fl = np.zeros(x.shape, bool)
    fl[0, :, 10:20, 10:20] = True
    np.random.seed(4)
    c = Preprocessor(x, flags=fl).create_dataset(patch_size=32, on_device_tiling=False, **kw)
    np.random.seed(4)
    d = Preprocessor(x, flags=fl).create_dataset(patch_size=32, **kw)
    np.testing.assert_array_equal(c.labels.numpy(), d.labels.numpy())
    np.testing.assert_allclose(c.images.numpy(), d.images.numpy(), rtol=0, atol=2e-6, equal_nan=True)


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_mad_flags_of_complex_input_on_device(dtype):
    rng = np.random.default_rng(6)
    z = (rng.normal(size=(1, 1, 128, 64)) + 1j * rng.normal(size=(1, 1, 128, 64))).astype(dtype)
    z[0, 0, 40:44, :] *= 30.0
    np.random.seed(8)
    a = Preprocessor(z).create_dataset(patch_size=64, flag_sigma=5, on_device_tiling=False)
    np.random.seed(8)
    b = Preprocessor(z).create_dataset(patch_size=64, flag_sigma=5)
    assert b.labels.numpy().any()
    np.testing.assert_array_equal(a.labels.numpy(), b.labels.numpy())
    np.testing.assert_allclose(a.images.numpy(), b.images.numpy(), rtol=0, atol=2e-6)


def test_failed_preprocess_calls_release_their_device_temporaries():
    """A call that stages host data and then fails on an argument check leaves no device memory behind: the context's
    allocation count is what the valid calls (and the grow-only scratch they made) left, and the context stays usable."""
    import ctypes as C

    from rfi_toolbox_amd import runtime
    from rfi_toolbox_amd._lib import F64, HOST, lib

    ctx = runtime.Context(0)          # a context of its own: arrays of other tests freed meanwhile cannot move the count
    try:
        def ptr(a):
            return a.ctypes.data_as(C.c_void_p)

        def calls(pixels):
            """rfi_preprocess_patches and rfi_preprocess_real on one float64 host row -> (rc, last error) of each"""
            x = np.random.default_rng(pixels).random((1, 1, pixels))
            out = np.empty((1, 1, pixels, 3), np.float32)
            rc = lib.rfi_preprocess_patches(ctx.handle, ptr(x), HOST, F64, 1, 1, pixels, ptr(out), HOST)
            res = [(rc, lib.rfi_last_error().decode())]
            rc = lib.rfi_preprocess_real(ctx.handle, ptr(x), HOST, F64, 1, 1, pixels, 0, 0, 0, 3.0, ptr(out), HOST,
                                         None, HOST)
            res.append((rc, lib.rfi_last_error().decode()))
            return res

        def allocations():
            n, b = C.c_int64(), C.c_uint64()
            assert lib.rfi_ctx_allocations(ctx.handle, C.byref(n), C.byref(b)) == 0
            return n.value, b.value

        assert [rc for rc, _ in calls(4096)] == [0, 0]
        before = allocations()
        for rc, err in calls(4097):       # 64-bit rows longer than 4,096 pixels: refused after the host data is staged
            assert rc == 1 and "patch rows this long" in err, err
        assert allocations() == before
        assert [rc for rc, _ in calls(4096)] == [0, 0]
        assert allocations() == before
    finally:
        lib.rfi_ctx_destroy(ctx.handle)
