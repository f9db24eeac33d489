"""Whole-observation flag prediction for 8-channel models on the GPU: the gather kernel (tile_observation) bit for
bit against Normalizer.transform cut by the NumPy restatement (tests/pol_tiling_ref.py), stitch_patches against
tests/stitch_ref.py, and predict_flags against the composition tile_observation -> forward_nhwc -> stitch_ref.stitch."""
import ctypes as C

import numpy as np
import pytest
import torch

import pol_tiling_ref as pref
import stitch_ref as sref
from test_gpu_predict_flags import BAND          # probabilities of two paths whose forwards ran in different batch sizes

pytestmark = pytest.mark.gpu

PS = 32
SHAPES = [(50, 77), (77, 50), (20, 70), (64, 64), (65, 63)]       # edge padding, a short axis, on / off a 32 x 32 tile edge
METHODS = ("global_min_max", "standardize", "robust_scale")
FORMS = [(m, s) for m in (None,) + METHODS for s in ("dataset", "sample")]


def _observation(shape, dtype, seed=0, n=3):
    """(n, 4, C, T): noise with a few bright channels and a burst, every baseline on its own scale and offset."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 4) + tuple(shape)) + 1j * rng.standard_normal((n, 4) + tuple(shape))
    C_, T_ = shape
    d[..., C_ // 3: C_ // 3 + 3, :] *= 40.0
    d[..., :, T_ // 2: T_ // 2 + 2] *= 25.0
    d *= np.array([1.0, 7.5, 0.02])[:n].reshape(n, 1, 1, 1)
    d += np.array([0.0, 3.0 - 2.0j, 0.01j])[:n].reshape(n, 1, 1, 1)
    return d.astype(dtype)


def _fitted(method, scope, data):
    """-> (normalizer to pass, the (n, 8, C, T) planes Normalizer.transform makes, one (centre, scale) per sample)"""
    from rfi_toolbox_amd.preprocessing import Normalizer
    nz = Normalizer(method, scope).fit(data)
    norm = nz.transform(data, out="nchw")
    n = len(data)
    pairs = list(zip(nz.centres, nz.scales)) if scope == "sample" else [(nz.centres[0], nz.scales[0])] * n
    return (None if method is None else nz), norm, pairs


def _unet(in_ch=8, seed=0):
    from rfi_toolbox_amd.models import UNet
    torch.manual_seed(seed)
    return UNet(in_ch, 1, 8, device="cuda:0").eval()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- 1, 2: the gather
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("shape", SHAPES)
def test_gather_is_transform_cut_by_the_restatement(shape, dtype):
    from rfi_toolbox_amd.inference import tile_observation
    from rfi_toolbox_amd.preprocessing import Normalizer
    data = _observation(shape, dtype, seed=shape[0])
    for method, scope in FORMS:
        nz, norm, pairs = _fitted(method, scope, data)
        assert scope == "dataset" or method is None or len(set(pairs)) == len(data)      # every baseline its own pair
        passed = Normalizer(method, "sample") if scope == "sample" else nz  # sample scope: fitted or not, the same
        for stride in (32, 24, 16):
            for views in (1, 2, 4):
                for edge in ("pad", "shift"):
                    want = pref.cut_channels(norm, pairs, PS, stride, views, edge)
                    got = tile_observation(data, PS, stride, views, edge, normalizer=passed).numpy()
                    assert got.shape == want.shape and got.dtype == np.float32
                    assert np.array_equal(_bits(got), _bits(want)), (method, scope, stride, views, edge,
                                                                     int((_bits(got) != _bits(want)).sum()))


def test_single_sample_and_fitted_sample_scope_agree():
    from rfi_toolbox_amd.inference import tile_observation
    from rfi_toolbox_amd.preprocessing import Normalizer
    data = _observation((50, 77), np.complex64, seed=2)
    a = tile_observation(data, PS, 24, 4, normalizer=Normalizer("standardize", "sample")).numpy()
    stale = Normalizer("standardize", "sample").fit(data[::-1].copy())     # a stored fit of other data is ignored
    assert np.array_equal(_bits(a), _bits(tile_observation(data, PS, 24, 4, normalizer=stale).numpy()))
    one = tile_observation(data[1], PS, 24, 4, normalizer=Normalizer("standardize", "sample")).numpy()      # (4, C, T)
    per = len(a) // 3
    assert np.array_equal(_bits(one), _bits(a[per:2 * per]))


def test_constant_baseline_gives_zeros_padding_included():
    from rfi_toolbox_amd.inference import tile_observation
    from rfi_toolbox_amd.preprocessing import Normalizer
    data = _observation((20, 70), np.complex64, seed=3)
    data[1] = 2.0 + 2.0j
    got = tile_observation(data, PS, 24, 4, normalizer=Normalizer("global_min_max", "sample")).numpy()
    per = len(got) // 3
    assert not _bits(got[per:2 * per]).any()                              # +0.0 everywhere
    assert got[:per].any() and got[2 * per:].any()
    want = pref.tile(data, pref.pairs_of(data, "global_min_max", "sample"), PS, 24, 4)
    assert np.array_equal(_bits(got), _bits(want))


# ---------------------------------------------------------------- 3: stitch_patches
@pytest.mark.parametrize("views,stride,edge,combine", [(1, 32, "pad", "mean"), (2, 24, "shift", "max"), (4, 16, "pad", "mean"),
                                                       (4, 24, "shift", "max")])
def test_stitch_patches_matches_restatement(views, stride, edge, combine):
    from rfi_toolbox_amd.inference import stitch_patches
    from rfi_toolbox_amd.runtime import Context, DeviceArray
    Cn, Tn, n = 50, 77, 3
    rng = np.random.default_rng(views * 100 + stride)
    N = n * sref.patches_per_plane(Cn, Tn, PS, stride, views, edge)
    probs = rng.random((N, PS, PS), dtype=np.float32)
    kw = dict(stride=stride, views=views, edge=edge, combine=combine, return_probabilities=True)
    f, p = stitch_patches(probs, Cn, Tn, PS, logits=False, **kw)
    wf, wp = sref.stitch(probs, n, Cn, Tn, PS, stride, views, edge, combine, 0.5, logits=False)
    assert f.dtype == bool and f.shape == (n, Cn, Tn) and p.dtype == np.float32
    assert np.array_equal(_bits(p), _bits(wp)) and np.array_equal(f, wf)
    assert np.array_equal(stitch_patches(probs[..., None], Cn, Tn, PS, logits=False, **kw)[0], wf)     # (N, ps, ps, 1)
    logits = (rng.standard_normal((N, PS, PS)) * 3).astype(np.float32)
    f, p = stitch_patches(logits, Cn, Tn, PS, threshold=0.4, **kw)
    wf, wp = sref.stitch(logits, n, Cn, Tn, PS, stride, views, edge, combine, 0.4, logits=True)
    assert np.abs(p - wp).max() <= 1e-6
    sure = np.abs(wp - 0.4) > 1e-6
    assert np.array_equal(f[sure], wf[sure])
    df, dp = stitch_patches(Context.get(0).to_device(logits), Cn, Tn, PS, threshold=0.4, **kw)          # stays on the device
    assert isinstance(df, DeviceArray) and df.dtype == np.bool_ and isinstance(dp, DeviceArray)
    assert np.array_equal(df.numpy(), f) and np.array_equal(_bits(dp.numpy()), _bits(p))
    tf, tp = stitch_patches(torch.from_numpy(logits).to("cuda:0"), Cn, Tn, PS, threshold=0.4, **kw)
    assert tf.is_cuda and tf.dtype == torch.bool and np.array_equal(tf.cpu().numpy(), f)
    assert np.array_equal(_bits(tp.cpu().numpy()), _bits(p))


# ---------------------------------------------------------------- 4 .. 9: predict_flags
def _normalizer(form, data):
    from rfi_toolbox_amd.preprocessing import Normalizer
    if form == "none":
        return None
    if form == "dataset":
        return Normalizer("standardize", "dataset").fit(data)
    return Normalizer(form, "sample")


def _composition(model, data, normalizer, stride=None, views=1, edge="pad", combine="mean"):
    """tile_observation -> forward_nhwc -> the restatement: (combined probabilities (n, C, T), a threshold at their
    median, so that both flag values occur)."""
    from rfi_toolbox_amd.inference import tile_observation
    d4 = data if data.ndim == 4 else data[None]
    tiles = tile_observation(data, PS, stride, views, edge, normalizer=normalizer).numpy()
    out = model.forward_nhwc(tiles)[..., 0]
    n, _, Cn, Tn = d4.shape
    _, wp = sref.stitch(out, n, Cn, Tn, PS, stride, views, edge, combine, 0.5, logits=True)
    return wp, float(np.median(wp))


def _agree(f, p, wp, thr, band=BAND):
    f, p = np.asarray(f), np.asarray(p)
    print("max |p - expected| =", float(np.abs(p - wp).max()))
    assert p.shape == wp.shape and np.abs(p - wp).max() <= band, np.abs(p - wp).max()
    sure = np.abs(wp - thr) > band
    assert np.array_equal(f[sure], (wp > np.float32(thr))[sure])
    assert 0 < f[sure].sum() < sure.sum()                                  # both flag values among the sure pixels


@pytest.mark.parametrize("tiling", [dict(views=1), dict(views=4, combine="mean"), dict(views=4, stride=24, combine="max"),
                                    dict(views=2, stride=16, edge="shift")])
@pytest.mark.parametrize("form", ["none", "dataset", "robust_scale", "standardize", "global_min_max"])
def test_predict_flags_equals_composition(form, tiling):
    from rfi_toolbox_amd.inference import predict_flags
    model = _unet()
    data = _observation((50, 77), np.complex64, seed=5)
    nz = _normalizer(form, data)
    wp, thr = _composition(model, data, nz, **tiling)
    f, p = predict_flags(model, data, patch_size=PS, threshold=thr, normalizer=nz, broadcast_pols=False,
                         return_probabilities=True, **tiling)
    assert f.shape == (3, 50, 77) and f.dtype == bool and p.dtype == np.float32
    _agree(f, p, wp, thr)


@pytest.mark.parametrize("dtype,shape", [(np.complex128, (77, 50)), (np.complex64, (20, 70)), (np.complex128, (65, 63))])
def test_predict_flags_other_shapes_and_small_batches(dtype, shape):
    from rfi_toolbox_amd.inference import predict_flags
    model = _unet()
    data = _observation(shape, dtype, seed=6)
    nz = _normalizer("robust_scale", data)
    wp, thr = _composition(model, data, nz, stride=24, views=4)
    for batch in (64, 5):
        f, p = predict_flags(model, data, patch_size=PS, stride=24, views=4, threshold=thr, batch_size=batch, normalizer=nz,
                             broadcast_pols=False, return_probabilities=True)
        _agree(f, p, wp, thr)


def test_sample_scope_in_several_groups(monkeypatch):
    from rfi_toolbox_amd import inference
    model = _unet()
    data = _observation((50, 77), np.complex64, seed=7)
    nz = _normalizer("robust_scale", data)
    kw = dict(patch_size=PS, stride=24, views=2, normalizer=nz, broadcast_pols=False, return_probabilities=True)
    _, p1 = inference.predict_flags(model, data, **kw)
    thr = float(np.median(p1))
    f1, p1 = inference.predict_flags(model, data, threshold=thr, **kw)
    monkeypatch.setattr(inference, "_SAMPLE_GROUP_BYTES", data[0].nbytes)
    assert inference._sample_groups(3, data[0].nbytes) == [(0, 1), (1, 2), (2, 3)]
    for d in (data, torch.from_numpy(data).to("cuda:0")):                  # one upload per group / views of the tensor
        fg, pg = inference.predict_flags(model, d, threshold=thr, **kw)
        _agree(fg.cpu().numpy() if torch.is_tensor(fg) else fg, pg.cpu().numpy() if torch.is_tensor(pg) else pg, p1, thr)


def test_reproducible():
    from rfi_toolbox_amd.inference import predict_flags
    model = _unet()
    data = _observation((50, 77), np.complex64, seed=8)
    kw = dict(patch_size=PS, stride=16, views=4, normalizer=_normalizer("standardize", data), return_probabilities=True)
    f1, p1 = predict_flags(model, data, **kw)
    f2, p2 = predict_flags(model, data, **kw)
    assert f1.tobytes() == f2.tobytes() and p1.tobytes() == p2.tobytes()


def test_input_forms_and_result_shapes():
    from rfi_toolbox_amd.inference import predict_flags
    from rfi_toolbox_amd.runtime import DeviceArray
    model = _unet()
    data = _observation((50, 77), np.complex64, seed=9)
    for form in ("none", "global_min_max"):
        nz = _normalizer(form, data)
        kw = dict(patch_size=PS, stride=24, views=2, normalizer=nz, return_probabilities=True)
        _, p = predict_flags(model, data, **kw)
        kw["threshold"] = float(np.median(p))
        f, p = predict_flags(model, data, **kw)
        assert f.shape == data.shape and f.dtype == bool and p.shape == (3, 50, 77)
        assert all(np.array_equal(f[:, 0], f[:, k]) for k in range(1, 4)) and 0 < f.sum() < f.size
        fb, pb = predict_flags(model, data, broadcast_pols=False, **kw)
        assert fb.shape == (3, 50, 77) and np.array_equal(fb, f[:, 0]) and np.array_equal(pref.broadcast(fb), f)
        assert pb.tobytes() == p.tobytes()
        tf, tp = predict_flags(model, torch.from_numpy(data).to("cuda:0"), **kw)            # CUDA in, CUDA out
        assert tf.is_cuda and tf.dtype == torch.bool and tp.is_cuda and tuple(tf.shape) == data.shape
        assert np.array_equal(tf.cpu().numpy(), f) and tp.cpu().numpy().tobytes() == p.tobytes()
        cf = predict_flags(model, torch.from_numpy(data), **{**kw, "return_probabilities": False})
        assert isinstance(cf, np.ndarray) and np.array_equal(cf, f)
        dev = model.ctx.to_device(data)                                                      # DeviceArray in
        hf, hp = predict_flags(model, dev, **kw)
        assert isinstance(hf, np.ndarray) and np.array_equal(hf, f) and hp.tobytes() == p.tobytes()
        for src in (data, dev):                                                              # out="device"
            df, dp = predict_flags(model, src, out="device", **kw)
            assert isinstance(df, DeviceArray) and isinstance(dp, DeviceArray) and df.dtype == np.bool_
            assert df.shape == data.shape and dp.shape == (3, 50, 77)
            assert np.array_equal(df.numpy(), f) and dp.numpy().tobytes() == p.tobytes()
        df = predict_flags(model, dev, out="device", broadcast_pols=False, **{**kw, "return_probabilities": False})
        assert df.shape == (3, 50, 77) and np.array_equal(df.numpy(), fb)
        f1, p1 = predict_flags(model, data[1], **kw)                                         # (4, C, T)
        assert f1.shape == (4, 50, 77) and p1.shape == (50, 77)
        assert np.abs(p1 - p[1]).max() <= BAND      # (the baseline's own pair either way; another forward batch)


def test_train_mode_model_is_left_alone():
    from rfi_toolbox_amd.inference import predict_flags
    model = _unet().train()
    x = torch.randn(2, PS, PS, 8)
    y = (torch.rand(2, PS, PS) > 0.7).to(torch.uint8)
    model.train_step(x, y, lr=1e-3)                    # running statistics away from their initial values
    before = {k: v.clone() for k, v in model.state_dict().items()}
    data = _observation((50, 77), np.complex64, seed=10)
    nz = _normalizer("standardize", data)
    f, p = predict_flags(model, data, patch_size=PS, normalizer=nz, broadcast_pols=False, return_probabilities=True)
    assert model.training
    after = model.state_dict()
    for k, v in before.items():
        assert v.numpy().tobytes() == after[k].numpy().tobytes(), k
    model.eval()
    wp, _ = _composition(model, data, nz)               # the eval forward: running statistics, not batch statistics
    assert np.abs(p - wp).max() <= BAND


def test_bfloat16():
    from rfi_toolbox_amd.inference import predict_flags
    model = _unet().set_compute_dtype("bfloat16")
    data = _observation((50, 77), np.complex64, seed=11)
    nz = _normalizer("robust_scale", data)
    wp, thr = _composition(model, data, nz, views=2)
    f, p = predict_flags(model, data, patch_size=PS, views=2, threshold=thr, normalizer=nz, broadcast_pols=False,
                         return_probabilities=True)
    print("bfloat16: max |p - expected| =", float(np.abs(p - wp).max()))
    assert np.isfinite(p).all() and np.abs(p - wp).max() <= 2e-3


# ---------------------------------------------------------------- 10: the 3-channel path
def test_three_channel_path_is_unchanged():
    from rfi_toolbox_amd._lib import COMPLEX_CODES, EDGE_PAD, HOST, Tiling, check, lib
    from rfi_toolbox_amd.inference import predict_flags
    model = _unet(3)
    data = _observation((50, 77), np.complex64, seed=12, n=2)[:, :2].copy()          # (2, 2, C, T)
    flags = np.empty(data.shape, dtype=np.uint8)
    prob = np.empty(data.shape, dtype=np.float32)
    check(lib.rfi_model_predict_flags(model._h, data.ctypes.data_as(C.c_void_p), HOST, COMPLEX_CODES[data.dtype], 4, 50, 77,
                                      C.byref(Tiling(PS, 24, EDGE_PAD, 2)), 64, 0, 0.5, flags.ctypes.data_as(C.c_void_p), HOST,
                                      prob.ctypes.data_as(C.c_void_p), HOST))
    f, p = predict_flags(model, data, patch_size=PS, stride=24, views=2, return_probabilities=True)
    assert f.dtype == bool and f.tobytes() == flags.tobytes() and p.tobytes() == prob.tobytes()
    df, dp = predict_flags(model, data, patch_size=PS, stride=24, views=2, return_probabilities=True, out="device")
    assert df.numpy().tobytes() == flags.tobytes() and dp.numpy().tobytes() == prob.tobytes()
