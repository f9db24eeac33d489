"""-m gpu: a K-class flagger after training -- per-class evaluation, K-channel stitching and whole-observation flags.

test_eval_batch_counts_per_class   eval_batch (K, 3) equals NumPy counts of the device's own probabilities against the label
                                   bits, exactly, with the cut planted on one element's probability (strict >: not flagged)
test_evaluate_rfi_model_per_class  per_class / macro of evaluate_rfi_model from those counts under the reference's rules
test_stitch_classes_is_stitch_per_class   stitch_patches on (N, 8, 8, 3) equals three calls on values[..., k], bit for bit
test_predict_flags_is_the_composition     predict_flags on a UNet(8, 3, ...) equals tile_observation -> forward_nhwc (eval) ->
                                   stitch_patches, bit for bit (one forward batch holds every tile in both paths)
test_refusals                      3 input channels with K > 1, broadcast_pols=False, eval_sweep
test_class_bits_pass_the_augmenter the augmenter copies label bytes: no new byte value, a flip-only sample is an exact copy
"""
import numpy as np
import pytest
import torch

from rfi_toolbox_amd.class_labels import unpack_class_bits

pytestmark = pytest.mark.gpu


def _unet(in_ch, K, feat, depth, seed=0, **kw):
    from rfi_toolbox_amd.models import UNet
    torch.manual_seed(seed)
    return UNet(in_ch, K, feat, depth=depth, device="cuda:0", **kw)


def _device_probs(logits_nhwk):
    """sigmoid as the device computes it, through the stitch of one tile per plane (the mean of one value is the value)"""
    from rfi_toolbox_amd.inference import stitch_patches
    n, h, w, K = logits_nhwk.shape
    assert h == w
    _, p = stitch_patches(logits_nhwk, h, w, h, return_probabilities=True)
    assert p.shape == (n, K, h, w)
    return p.transpose(0, 2, 3, 1)


def _counts(pred, truth):
    return np.array([[int((pred[..., k] & truth[..., k]).sum()), int((pred[..., k] & ~truth[..., k]).sum()),
                      int((~pred[..., k] & truth[..., k]).sum())] for k in range(pred.shape[-1])], np.int64)


def _eval_setup(K=3):
    m = _unet(3, K, 4, 1, seed=4).set_targets("class_bits").eval()
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 16, 16, 3)).astype(np.float32)
    y = rng.integers(0, 256, (3, 16, 16), dtype=np.uint8)
    return m, x, y


def test_eval_batch_counts_per_class():
    K = 3
    m, x, y = _eval_setup(K)
    truth = unpack_class_bits(y, K, channel_axis=-1)
    probs = _device_probs(m.forward_nhwc(x))
    planted = float(np.sort(probs.ravel())[probs.size // 3])          # exactly one element's probability (and its ties')
    for thr in (0.5, planted, 0.0, 1.0):
        got = m.eval_batch(x, y, thr)
        assert got.shape == (K, 3) and got.dtype == np.int64
        want = _counts(probs > np.float32(thr), truth)
        assert np.array_equal(got, want), (thr, got, want)
    assert (probs == np.float32(planted)).any() and not (probs > np.float32(planted)).all()
    # bits at and above K are ignored
    assert np.array_equal(m.eval_batch(x, y & np.uint8(7), 0.5), m.eval_batch(x, y, 0.5))
    # the K = 1 class-bit count is the label-map count of bit 0
    m1 = _unet(3, 1, 4, 1, seed=6).eval()
    tp_fp_fn = m1.eval_batch(x, y & np.uint8(1), 0.5)
    assert np.array_equal(m1.set_targets("class_bits").eval_batch(x, y, 0.5), np.array([tp_fp_fn], np.int64))


def test_evaluate_rfi_model_per_class():
    from rfi_toolbox_amd.evaluation.metrics import _dice, _f1, _iou, _precision, _recall
    from rfi_toolbox_amd.training import evaluate_rfi_model
    K = 3
    m, x, y = _eval_setup(K)
    m.train()
    names = ["a", "b", "c"]
    res = evaluate_rfi_model(m, (x, y), batch_size=2, threshold=0.4, class_names=names)
    assert m.training                                                  # the mode is put back
    m.eval()
    batches = [m.eval_batch(x[:2], y[:2], 0.4), m.eval_batch(x[2:], y[2:], 0.4)]
    rules = {"iou": _iou, "precision": _precision, "recall": _recall, "f1": _f1, "dice": _dice}
    assert [c["name"] for c in res["per_class"]] == names and set(res) == {"per_class", "macro"}
    for k in range(K):
        for key, f in rules.items():
            want = float(np.mean([f(*(int(v) for v in b[k])) for b in batches]))
            assert res["per_class"][k][key] == want, (k, key)
    for key in rules:
        assert res["macro"][key] == float(np.mean([c[key] for c in res["per_class"]]))
    assert [c["name"] for c in evaluate_rfi_model(m, (x, y))["per_class"]] == ["class0", "class1", "class2"]
    with pytest.raises(ValueError):
        evaluate_rfi_model(m, (x, y), class_names=["a"])
    one = _unet(3, 1, 4, 1, seed=6)
    assert set(evaluate_rfi_model(one, (x, y & np.uint8(1)))) == set(rules)      # a label-map model: the five metrics, as before
    with pytest.raises(ValueError):
        evaluate_rfi_model(one, (x, y), class_names=["rfi"])


@pytest.mark.parametrize("combine", ["mean", "max"])
def test_stitch_classes_is_stitch_per_class(combine):
    from rfi_toolbox_amd.inference import stitch_patches, tiling_count
    Cn, Tn, ps, stride, views, K = 19, 27, 8, 5, 4, 3
    ppp = tiling_count(Cn, Tn, ps, stride, views, "pad")
    rng = np.random.default_rng(7)
    vals = (3.0 * rng.standard_normal((2 * ppp, ps, ps, K))).astype(np.float32)
    kw = dict(stride=stride, views=views, edge="pad", combine=combine, return_probabilities=True)
    for logits, v in ((True, vals), (False, (1.0 / (1.0 + np.exp(-vals))).astype(np.float32))):
        thr = 0.45
        f, p = stitch_patches(v, Cn, Tn, ps, threshold=thr, logits=logits, **kw)
        assert f.shape == p.shape == (2, K, Cn, Tn) and f.dtype == np.bool_ and p.dtype == np.float32
        for k in range(K):
            fk, pk = stitch_patches(np.ascontiguousarray(v[..., k]), Cn, Tn, ps, threshold=thr, logits=logits, **kw)
            assert fk.shape == (2, Cn, Tn)
            assert np.array_equal(f[:, k], fk) and p[:, k].tobytes() == pk.tobytes(), (logits, k)
        assert 0 < f.sum() < f.size
        assert np.array_equal(stitch_patches(v, Cn, Tn, ps, threshold=thr, logits=logits, **{**kw, "return_probabilities": False}), f)
    # a DeviceArray in, DeviceArrays out
    from rfi_toolbox_amd.runtime import Context
    fd, pd = stitch_patches(Context.get(0).to_device(vals), Cn, Tn, ps, threshold=0.45, **kw)
    f, p = stitch_patches(vals, Cn, Tn, ps, threshold=0.45, **kw)
    assert np.array_equal(fd.numpy().view(np.bool_), f) and pd.numpy().tobytes() == p.tobytes()


def _observation(seed=0):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((2, 4, 40, 52)) + 1j * rng.standard_normal((2, 4, 40, 52))
    d[:, :, 13:16, :] *= 40.0
    d[:, :, :, 26:28] *= 25.0
    d[1] = d[1] * 7.5 + (3.0 - 2.0j)
    return d.astype(np.complex64)


@pytest.mark.parametrize("combine", ["mean", "max"])
def test_predict_flags_is_the_composition(combine):
    from rfi_toolbox_amd.inference import predict_flags, stitch_patches, tile_observation, tiling_count
    from rfi_toolbox_amd.preprocessing import Normalizer
    K, ps, stride, views = 3, 16, 12, 2
    data = _observation()
    model = _unet(8, K, 4, 2, seed=8).set_targets("class_bits").train()       # any mode: the forward runs in eval mode
    nz = Normalizer("robust_scale", "sample")
    n_tiles = 2 * tiling_count(40, 52, ps, stride, views, "pad")
    tiles = tile_observation(data, ps, stride, views, "pad", normalizer=nz)
    assert tiles.shape == (n_tiles, ps, ps, 8)
    model.eval()
    out = model.forward_nhwc(tiles.numpy())                                    # one batch of every tile ...
    model.train()
    assert out.shape == (n_tiles, ps, ps, K)
    probs = stitch_patches(out, 40, 52, ps, stride, views, "pad", combine, return_probabilities=True)[1]
    thr = float(np.median(probs))
    wf, wp = stitch_patches(out, 40, 52, ps, stride, views, "pad", combine, threshold=thr, return_probabilities=True)
    kw = dict(patch_size=ps, stride=stride, views=views, combine=combine, threshold=thr, normalizer=nz,
              batch_size=n_tiles)                                              # ... as here
    f, p = predict_flags(model, data, return_probabilities=True, **kw)
    assert model.training
    assert f.shape == p.shape == (2, K, 40, 52) and f.dtype == np.bool_ and p.dtype == np.float32
    assert p.tobytes() == wp.tobytes() and np.array_equal(f, wf)
    assert 0 < f.sum() < f.size and min(np.abs(p[:, a] - p[:, b]).max() for a in range(K) for b in range(a)) > 1e-3
    assert np.array_equal(predict_flags(model, data, **kw), f)
    f1, p1 = predict_flags(model, data[1], return_probabilities=True, **{**kw, "batch_size": n_tiles // 2})     # (4, C, T)
    assert f1.shape == (K, 40, 52) and np.abs(p1 - p[1]).max() <= 1e-5         # (another forward batch)
    fd = predict_flags(model, data, out="device", **kw)
    assert fd.shape == (2, K, 40, 52) and np.array_equal(fd.numpy().view(np.bool_), f)


def test_refusals():
    from rfi_toolbox_amd.inference import predict_flags
    data = _observation()
    with pytest.raises(ValueError, match="output channel"):
        predict_flags(_unet(3, 2, 4, 2), data, patch_size=16)
    m = _unet(8, 3, 4, 2).set_targets("class_bits")
    with pytest.raises(ValueError, match="broadcast_pols"):
        predict_flags(m, data, patch_size=16, broadcast_pols=False)
    x, y = np.zeros((1, 16, 16, 8), np.float32), np.zeros((1, 16, 16), np.uint8)
    with pytest.raises(RuntimeError, match="eval_sweep"):
        m.eval_sweep(x, y, [0.5])
    with pytest.raises(RuntimeError, match="eval_sweep"):
        _unet(8, 1, 4, 2).set_targets("class_bits").eval_sweep(x, y, [0.5])


def test_class_bits_pass_the_augmenter():
    from rfi_toolbox_amd.training import Augmenter
    rng = np.random.default_rng(9)
    n, h, w = 8, 24, 40
    x = rng.standard_normal((n, h, w, 2)).astype(np.float32)
    allowed = np.array([0, 1, 2, 4, 8, 16, 3, 5, 9, 17, 6, 10, 18, 12, 20, 24, 31, 0x80, 0xFF], np.uint8)
    y = allowed[rng.integers(0, len(allowed), (n, h, w))]
    y[:, 0, 0] = 0
    aug = Augmenter(seed=3)
    _, yo = aug(x, y, call=2)
    yo = yo.numpy()
    gates, _ = aug.params(n, h, w, call=2)
    assert gates[:, 2:].any() and (gates[:, 2:] == 0).all(axis=1).any()        # warped samples and flip-only ones
    assert set(np.unique(yo).tolist()) <= set(allowed.tolist())
    for i in range(n):
        if not gates[i, 2:].any():
            want = y[i]
            want = want[:, ::-1] if gates[i, 0] else want
            want = want[::-1] if gates[i, 1] else want
            assert np.array_equal(yo[i], want), i
        else:
            assert not np.array_equal(yo[i], y[i])
