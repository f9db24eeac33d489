"""Whole-observation flag prediction on the GPU: rfi_stitch_patches against the NumPy restatement
(tests/stitch_ref.py), and predict_flags against the composition of the library's existing public pieces
(Preprocessor.create_dataset(inference_mode=True) -> model.forward_nhwc -> the restatement)."""
import ctypes as C

import numpy as np
import pytest
import torch

import stitch_ref as ref
from rfi_toolbox_amd._lib import EDGE_PAD, EDGE_SHIFT, HOST, VALUES_LOGITS, VALUES_PROBS, Tiling, check, lib
from rfi_toolbox_amd.runtime import Context

pytestmark = pytest.mark.gpu

BAND = 1e-5          # probabilities of two paths whose forwards ran in different batch sizes


def _stitch_dev(vals, n_planes, Cn, Tn, ps, stride, views, edge, combine, thr, kind):
    ctx = Context.get(0)
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    flags = np.empty((n_planes, Cn, Tn), dtype=np.uint8)
    prob = np.empty((n_planes, Cn, Tn), dtype=np.float32)
    check(lib.rfi_stitch_patches(ctx.handle, vals.ctypes.data_as(C.c_void_p), HOST, kind, n_planes, Cn, Tn,
                                 C.byref(Tiling(ps, stride, {"pad": EDGE_PAD, "shift": EDGE_SHIFT}[edge], views)),
                                 {"mean": 0, "max": 1}[combine], float(thr), flags.ctypes.data_as(C.c_void_p), HOST,
                                 prob.ctypes.data_as(C.c_void_p), HOST))
    return flags.astype(bool), prob


def _check_stitch(n_planes, Cn, Tn, ps, stride, views, edge, combine, seed):
    rng = np.random.default_rng(seed)
    n = n_planes * ref.patches_per_plane(Cn, Tn, ps, stride, views, edge)
    probs = rng.random((n, ps, ps), dtype=np.float32)
    probs[:, :2, :2] = 0.5                                  # exactly at the threshold: not flagged
    f, p = _stitch_dev(probs, n_planes, Cn, Tn, ps, stride, views, edge, combine, 0.5, VALUES_PROBS)
    wf, wp = ref.stitch(probs, n_planes, Cn, Tn, ps, stride, views, edge, combine, 0.5, logits=False)
    assert np.array_equal(p.view(np.uint32), wp.view(np.uint32)) and np.array_equal(f, wf)
    logits = (rng.standard_normal((n, ps, ps)) * 3).astype(np.float32)
    f, p = _stitch_dev(logits, n_planes, Cn, Tn, ps, stride, views, edge, combine, 0.5, VALUES_LOGITS)
    wf, wp = ref.stitch(logits, n_planes, Cn, Tn, ps, stride, views, edge, combine, 0.5, logits=True)
    assert np.abs(p - wp).max() <= 1e-6
    sure = np.abs(wp - 0.5) > 1e-6
    assert np.array_equal(f[sure], wf[sure])


@pytest.mark.parametrize("combine", ["mean", "max"])
@pytest.mark.parametrize("edge", ["pad", "shift"])
@pytest.mark.parametrize("views", [1, 2, 4])
@pytest.mark.parametrize("stride", [64, 32, 48])
def test_stitch_matches_restatement(stride, views, edge, combine):
    _check_stitch(3, 200, 333, 64, stride, views, edge, combine, seed=stride * 10 + views)


@pytest.mark.parametrize("shape", [(192, 192), (40, 333), (333, 40), (50, 60)])
def test_stitch_square_and_short_axes(shape):
    for stride, views, edge, combine in ((64, 4, "pad", "mean"), (48, 4, "shift", "max"), (32, 2, "pad", "max")):
        _check_stitch(2, *shape, 64, stride, views, edge, combine, seed=7)


# ---------------------------------------------------------------- predict_flags
def _observation(shape, dtype, seed=0):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    C_, T_ = shape[-2:]
    d[..., C_ // 3: C_ // 3 + 5, :] *= 40.0                # a few bright channels and a burst in time
    d[..., :, T_ // 2: T_ // 2 + 3] *= 25.0
    return d.astype(dtype)


def _unet(cls=None, *args, seed=0):
    from rfi_toolbox_amd.models import UNet
    torch.manual_seed(seed)
    m = (cls or UNet)(*(args or (3, 1, 8)), device="cuda:0")
    return m.eval()


def _composition(model, data, ps, views, combine="mean", logits=True):
    """create_dataset(inference_mode=True) -> forward_nhwc -> restatement: (preprocessor, patch outputs, combined
    probabilities, a threshold at their median -- so that both flag values occur -- and the flags at it)."""
    from rfi_toolbox_amd.preprocessing import Preprocessor
    d4 = data if data.ndim == 4 else data[None]
    kw = {"enable_augmentation": False} if views == 1 else {"augmentation_rotations": views}
    prep = Preprocessor(data, flags=np.zeros(data.shape, dtype=bool))
    ds = prep.create_dataset(ps, inference_mode=True, **kw)
    out = model.forward_nhwc(ds.images.numpy())[..., 0]
    B, P, Cn, Tn = d4.shape
    _, wp = ref.stitch(out, B * P, Cn, Tn, ps, ps, views, "pad", combine, 0.5, logits=logits)
    wp = wp.reshape(data.shape)
    thr = float(np.median(wp))
    return prep, out, wp, thr, wp > np.float32(thr)


def _agree(f, p, wp, thr, band=BAND):
    assert np.abs(p - wp).max() <= band, np.abs(p - wp).max()
    sure = np.abs(wp - thr) > band
    assert np.array_equal(np.asarray(f)[sure], (wp > np.float32(thr))[sure])
    assert 0 < np.asarray(f)[sure].sum() < sure.sum()


@pytest.mark.parametrize("dtype,shape", [(np.complex64, (2, 2, 200, 333)), (np.complex128, (2, 2, 200, 333)),
                                         (np.complex64, (3, 150, 260))])
def test_single_cover_equals_composition(dtype, shape):
    from rfi_toolbox_amd.inference import predict_flags
    model = _unet()
    data = _observation(shape, dtype)
    _, _, wp, thr, _ = _composition(model, data, 64, 1)
    f, p = predict_flags(model, data, patch_size=64, threshold=thr, return_probabilities=True)
    assert f.shape == data.shape and f.dtype == bool and p.dtype == np.float32
    _agree(f, p, wp, thr)


def test_views_equal_reconstruct_flags():
    from rfi_toolbox_amd.inference import predict_flags
    model = _unet()
    data = _observation((1, 2, 150, 200), np.complex64, seed=3)
    for combine in ("mean", "max"):
        prep, out, wp, thr, wf = _composition(model, data, 64, 4, combine)
        f, p = predict_flags(model, data, patch_size=64, views=4, combine=combine, threshold=thr,
                             return_probabilities=True)
        _agree(f, p, wp, thr)
        rf = prep.reconstruct_flags(out, threshold=thr, combine=combine, logits=True)
        sure = np.abs(wp - thr) > 1e-6
        assert rf.shape == data.shape and np.array_equal(rf[sure], wf[sure])
        rf4 = prep.reconstruct_flags(torch.from_numpy(out[:, None]), threshold=thr, combine=combine, logits=True)
        assert np.array_equal(rf4, rf)                                                     # (N, 1, ps, ps) input


def test_reproducible_and_batch_independent():
    from rfi_toolbox_amd.inference import predict_flags
    model = _unet()
    data = _observation((2, 2, 200, 333), np.complex64, seed=5)
    kw = dict(patch_size=64, stride=32, views=2, return_probabilities=True)
    f1, p1 = predict_flags(model, data, **kw)
    thr = float(np.median(p1))
    f1, p1 = predict_flags(model, data, threshold=thr, **kw)
    f2, p2 = predict_flags(model, data, threshold=thr, **kw)
    assert np.array_equal(f1, f2) and np.array_equal(p1.view(np.uint32), p2.view(np.uint32))
    f7, p7 = predict_flags(model, data, batch_size=7, threshold=thr, **kw)
    _agree(f7, p7, p1, thr)


def test_train_mode_model_is_left_alone():
    from rfi_toolbox_amd.inference import predict_flags
    model = _unet().train()
    x = torch.randn(2, 64, 64, 3)
    y = (torch.rand(2, 64, 64) > 0.7).to(torch.uint8)
    model.train_step(x, y, lr=1e-3)                    # running statistics away from their initial values
    before = {k: v.clone() for k, v in model.state_dict().items()}
    data = _observation((1, 2, 128, 192), np.complex64)
    f, p = predict_flags(model, data, patch_size=64, return_probabilities=True)
    assert model.training
    after = model.state_dict()
    for k, v in before.items():
        assert v.numpy().tobytes() == after[k].numpy().tobytes(), k
    model.eval()
    _, _, wp, thr, _ = _composition(model, data, 64, 1)    # the eval forward: running statistics, not batch statistics
    assert np.abs(p - wp).max() <= BAND


def test_device_input_stays_on_device():
    from rfi_toolbox_amd.inference import predict_flags
    model = _unet()
    data = _observation((2, 2, 200, 333), np.complex64, seed=9)
    f, p = predict_flags(model, data, patch_size=64, stride=48, edge="shift", return_probabilities=True)
    td = torch.from_numpy(data).to("cuda:0")
    tf, tp = predict_flags(model, td, patch_size=64, stride=48, edge="shift", return_probabilities=True)
    assert tf.is_cuda and tf.dtype == torch.bool and tp.is_cuda and tuple(tf.shape) == data.shape
    assert np.array_equal(tf.cpu().numpy(), f) and np.array_equal(tp.cpu().numpy(), p)
    assert np.array_equal(predict_flags(model, torch.from_numpy(data), patch_size=64, stride=48, edge="shift"), f)


def test_sigmoid_head_is_not_sigmoided_twice():
    from rfi_toolbox_amd.inference import predict_flags
    from rfi_toolbox_amd.models import UNetOverfit
    model = _unet(UNetOverfit, 3, 1, 8)
    data = _observation((1, 2, 150, 200), np.complex64, seed=11)
    _, out, wp, thr, _ = _composition(model, data, 64, 1, logits=False)
    assert out.min() >= 0 and out.max() <= 1
    f, p = predict_flags(model, data, patch_size=64, threshold=thr, return_probabilities=True)
    _agree(f, p, wp, thr)


def test_bfloat16_and_other_models():
    from rfi_toolbox_amd.inference import predict_flags
    from rfi_toolbox_amd.models import SimpleCNN, UNetResNet18
    data = _observation((1, 2, 150, 200), np.complex64, seed=13)
    mb = _unet().set_compute_dtype("bfloat16")
    f, p = predict_flags(mb, data, patch_size=64, return_probabilities=True)
    _, _, wp, thr, _ = _composition(mb, data, 64, 1)
    assert np.abs(p - wp).max() <= 2e-3 and np.isfinite(p).all()
    for model in (_unet(SimpleCNN, 3, 1, 8), _unet(UNetResNet18, 3, 1, 8)):
        _, _, wp, thr, _ = _composition(model, data, 64, 1)
        f, p = predict_flags(model, data, patch_size=64, threshold=thr, return_probabilities=True)
        _agree(f, p, wp, thr)


def test_value_errors_with_a_model():
    from rfi_toolbox_amd.inference import predict_flags
    from rfi_toolbox_amd.preprocessing import Preprocessor
    data = _observation((1, 2, 100, 120), np.complex64)
    for args in ((1, 1, 8), (3, 2, 8)):
        with pytest.raises(ValueError, match="channel"):
            predict_flags(_unet(None, *args), data, patch_size=64)
    with pytest.raises(ValueError, match="multiple"):
        predict_flags(_unet(), data, patch_size=40)
    prep = Preprocessor(data, flags=np.zeros(data.shape, dtype=bool))
    ds = prep.create_dataset(64, enable_augmentation=False)                      # training mode
    with pytest.raises(ValueError, match="inference_mode"):
        prep.reconstruct_flags(np.zeros((len(ds), 64, 64), dtype=np.float32))
    ds = prep.create_dataset(64, inference_mode=True, enable_augmentation=False, num_patches=3)
    with pytest.raises(ValueError, match="truncated"):
        prep.reconstruct_flags(np.zeros((len(ds), 64, 64), dtype=np.float32))
    ds = prep.create_dataset(64, inference_mode=True, enable_augmentation=False)
    with pytest.raises(ValueError, match="expected"):
        prep.reconstruct_flags(np.zeros((len(ds) - 1, 64, 64), dtype=np.float32))
