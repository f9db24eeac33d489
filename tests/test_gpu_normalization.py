"""Input normalisation on the GPU (csrc/dataset_norm.hip, preprocessing.Normalizer, datasets.RFIMaskDataset) against the
fixtures captured from the reference and scikit-learn (tests/golden/make_normalization_golden.py) at 64x64, and against
the NumPy restatement tests/normalize_ref.py at 1024x1024.

Tolerances (normalize_ref.check_attrs / check_outputs, the same as for restatement vs golden): min, max, median, IQR and
the min-max / robust outputs bit-equal; mean and std within 1e-12 relative; standardize outputs within 1 float32 ulp with
at most a share of 1e-3 of the elements differing at all (the count is printed).

For float32 and complex64 sources the expectation is the restatement on the values WIDENED TO FP64: the device forms
(double(x) - centre) / scale and rounds once.  NumPy's own float32 arithmetic is not the target."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import normalize_ref as R

pytestmark = pytest.mark.gpu

ATTRS = ("global_min", "global_max", "mean", "std", "robust_median", "robust_iqr")


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = {"inputs": np.load(os.path.join(golden_dir, "normalization_inputs.npz")),
         "expected": np.load(os.path.join(golden_dir, "normalization_expected.npz"))}
    for m in R.METHODS:
        g["dataset_" + m] = np.load(os.path.join(golden_dir, f"normalization_expected_dataset_{m}.npz"))
        g["sample_" + m] = np.load(os.path.join(golden_dir, f"normalization_expected_sample_{m}.npz"))
    return g


@pytest.fixture(scope="module")
def big():
    """8 simulator samples of 1024 x 1024, complex128 (n, 4, T, F), as generate_batch leaves them in HBM"""
    from rfi_toolbox_amd.core import RFISimulator
    batch = RFISimulator(1024, 1024, seed=77, device="cuda:0").generate_batch(8, out="complex128")
    return batch.data, batch.data.numpy()


def _attrs(nz):
    return {k: getattr(nz, k) for k in ATTRS}


def _norm(*a, **k):
    from rfi_toolbox_amd.preprocessing import Normalizer
    return Normalizer(*a, device="cuda:0", **k)


def _nhwc_to_nchw(a):
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2))


# ---------------------------------------------------------------- goldens at 64 x 64
@pytest.mark.parametrize("method", R.METHODS)
def test_dataset_scope_matches_reference_dataset(golden, method):
    x = golden["inputs"]["inputs"]
    nz = _norm(method).fit(x)
    R.check_attrs(_attrs(nz), R.golden_attrs(golden["expected"], "four.", method), method, "four")
    want = golden["dataset_" + method]["items"]
    nchw = nz.transform(x, out="nchw")
    R.check_outputs(nchw, want, method, "dataset scope, device")
    assert np.array_equal(_nhwc_to_nchw(nz.transform(x, out="nhwc")).view(np.uint32), nchw.view(np.uint32))
    # parameters carried as plain floats give the same transform
    nz2 = _norm(None).load_state_dict(nz.state_dict())
    assert np.array_equal(nz2.transform(x, out="nchw").view(np.uint32), nchw.view(np.uint32))


@pytest.mark.parametrize("method", R.METHODS)
def test_sample_scope_matches_normalize_array(golden, method):
    from rfi_toolbox_amd.preprocessing import normalize_array
    gi = golden["inputs"]
    six = np.concatenate([gi["inputs"], gi["constant"][None], gi["two_valued"][None]])
    want = golden["sample_" + method]["outputs"]
    got = _norm(method, scope="sample").fit_transform(six, out="nchw")          # all six populations in the same launches
    R.check_outputs(got, want, method, "sample scope, device")
    one = normalize_array(six[2], method)
    assert one.dtype == np.float32 and np.array_equal(one.view(np.uint32), got[2].view(np.uint32))


@pytest.mark.parametrize("name", ["constant", "two_valued"])
@pytest.mark.parametrize("method", R.METHODS)
def test_degenerate_samples_behave_as_the_goldens(golden, name, method):
    x = golden["inputs"][name][None]
    nz = _norm(method).fit(x)
    R.check_attrs(_attrs(nz), R.golden_attrs(golden["expected"], name + ".", method), method, name)
    R.check_outputs(nz.transform(x, out="nchw"), golden["expected"][f"{name}.{method}.items"], method, name)
    if name == "constant":
        assert nz.mean == 0.5 and nz.std == 1e-8                # sums of 0.5 are exact
        if method == "global_min_max":
            assert nz.scales == [0.0] and not nz.transform(x).any()
    sp = _norm(method, scope="sample").fit(x)
    want = R.sample_params(x[0], method)
    assert (sp.centres[0], sp.scales[0]) == (want if want is not None else (0.0, 0.0))


# ---------------------------------------------------------------- statistics
def _check_raw(st, v):
    """one population's device statistics against sorted values v (fp64)"""
    from rfi_toolbox_amd.preprocessing.normalization import bracket
    n = v.size
    mean, var = R.moments(v)
    assert st["count"] == n and st["min"] == v[0] and st["max"] == v[-1]
    assert abs(st["mean"] - mean) <= R.REL_MOMENT * abs(mean), (st["mean"], mean)
    assert abs(st["var"] - var) <= R.REL_MOMENT * var, (st["var"], var)
    for j, q in enumerate((0.5, 0.25, 0.75)):
        lo, hi, _ = bracket(n, q)
        assert st["q"][j] == (v[lo], v[hi]), (q, st["q"][j], v[lo], v[hi])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_statistics_small_odd_sizes_chunking_and_reproducibility(dtype):
    """samples of 8 * 9 * 7 = 504 scalars: tiles of 512 straddle samples and chunks; negative values, ties and zeros"""
    rng = np.random.RandomState(5)
    x = (rng.standard_normal((9, 8, 9, 7)) * np.logspace(-6, 4, 9)[:, None, None, None]).astype(dtype)
    x[3, :, :2] = 0.0
    x[4] = np.round(x[4])
    whole = _norm("robust_scale").statistics(x)
    assert whole == _norm("robust_scale").statistics(x)                                      # two runs: bit-identical
    for cuts in ((3, 4), (1, 2, 8), (0, 9)):
        parts = [p for p in np.split(x, cuts)]
        assert _norm("robust_scale").statistics(parts) == whole, cuts                        # chunking: bit-identical
    mixed = [x[:2], np.ascontiguousarray(x[2:].transpose(0, 2, 3, 1))]                       # a channel-last chunk
    got = _norm("robust_scale").statistics(mixed)[0]
    _check_raw(got, np.sort(x.astype(np.float64).ravel()))
    assert (got["min"], got["max"], got["q"]) == (whole[0]["min"], whole[0]["max"], whole[0]["q"])
    _check_raw(whole[0], np.sort(x.astype(np.float64).ravel()))
    per = _norm("robust_scale", scope="sample").statistics(x)
    assert len(per) == 9
    for i in range(9):
        _check_raw(per[i], np.sort(x[i].astype(np.float64).ravel()))
    assert per[5] == _norm("robust_scale", scope="sample").statistics(x[5:6])[0]             # independent of the batch


def test_fit_over_chunks_equals_fit_over_concatenation(golden):
    x = golden["inputs"]["inputs"]
    for method in R.METHODS:
        a = _norm(method).fit(x)
        b = _norm(method).fit([x[:1], x[1:3], x[3:]])
        assert a.state_dict() == b.state_dict() == _norm(method).fit(x).state_dict()


def test_non_finite_input_raises():
    x = np.random.RandomState(1).standard_normal((2, 8, 16, 16))
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[1, 3, 5, 7] = bad
        for scope in ("dataset", "sample"):
            with pytest.raises(ValueError, match="non-finite"):
                _norm("standardize", scope=scope).fit(y)
    _norm("standardize").fit(x)


# ---------------------------------------------------------------- sizes users run: 1024 x 1024
def test_per_sample_batch_of_8_at_1024(big):
    dev, host = big
    x = R.to_nchw(host)                                                          # (8, 8, 1024, 1024) fp64
    stats = _norm("robust_scale", scope="sample").statistics(dev)
    assert len(stats) == 8
    for i in (0, 5):
        _check_raw(stats[i], np.sort(x[i].ravel()))
    for method in R.METHODS:
        nz = _norm(method, scope="sample")
        out = nz.fit_transform(dev, out="nhwc")                                  # DeviceArray in, DeviceArray out
        assert tuple(out.shape) == (8, 1024, 1024, 8) and out.dtype == np.float32
        got = _nhwc_to_nchw(out.numpy())
        R.check_outputs(got, R.normalize_samples(x, method), method, f"8 x 1024 x 1024 {method}")


def test_dataset_scope_chunks_at_1024(big):
    dev, host = big
    x = R.to_nchw(host[:3])
    chunks = [host[:1], host[1:3]]
    for method in R.METHODS:
        nz = _norm(method).fit(chunks)
        attrs, outs = R.normalize_dataset([x], method)
        R.check_attrs(_attrs(nz), attrs, method, "3 x 1024 x 1024")
        R.check_outputs(nz.transform(host[:3], out="nchw"), outs[0], method, f"dataset 1024 {method}")
        assert _norm(method).fit(host[:3]).state_dict() == nz.state_dict()


SOURCES = ["c128", "c64", "f64_nchw", "f64_nhwc", "f32_nchw", "f32_nhwc"]


def _source(host, kind):
    """one 1024 x 1024 sample in the given dtype / layout, and the (1, 8, T, F) fp64 values it holds"""
    z = host[:1]
    if kind == "c128":
        return z, None
    if kind == "c64":
        return z.astype(np.complex64), None
    planar = R.to_nchw(z)
    a = planar.astype(np.float32 if kind.startswith("f32") else np.float64)
    if kind.endswith("nhwc"):
        return np.ascontiguousarray(a.transpose(0, 2, 3, 1)), "nhwc"
    return a, "nchw"


@pytest.mark.parametrize("kind", SOURCES)
def test_every_source_layout_to_both_destinations_at_1024(big, kind):
    _, host = big
    src, layout = _source(host, kind)
    x = R.to_nchw(src, layout)                                                   # the values widened to fp64
    for method, scope in (("global_min_max", "dataset"), ("robust_scale", "dataset"), ("robust_scale", "sample"),
                          ("standardize", "sample")):
        nz = _norm(method, scope=scope)
        nchw = nz.fit_transform(src, out="nchw", layout=layout)
        nhwc = nz.transform(src, out="nhwc", layout=layout)
        assert nchw.shape == (1, 8, 1024, 1024) and nhwc.shape == (1, 1024, 1024, 8)
        assert np.array_equal(_nhwc_to_nchw(nhwc).view(np.uint32), nchw.view(np.uint32)), (kind, method)
        want = R.normalize_dataset([x], method)[1][0] if scope == "dataset" else R.normalize_samples(x, method)
        R.check_outputs(nchw, want, method, f"{kind} {scope} {method}")


def test_apply_in_place_and_overlap_check():
    from rfi_toolbox_amd._lib import F32, NORM_NHWC, NORM_NCHW, lib
    from rfi_toolbox_amd.runtime import Context
    ctx = Context.get("cuda:0")
    x = np.random.RandomState(3).standard_normal((2, 33, 17, 8)).astype(np.float32)
    want = ((x.astype(np.float64) - 0.25) / 3.0).astype(np.float32)
    src, dst = ctx.to_device(x), ctx.empty(x.shape, np.float32)
    args = (F32, NORM_NHWC, 2, 33 * 17, 0.25, 3.0, None)
    assert lib.rfi_norm_apply(ctx.handle, C.c_void_p(src.ptr), *args, C.c_void_p(dst.ptr), NORM_NHWC) == 0
    assert lib.rfi_norm_apply(ctx.handle, C.c_void_p(src.ptr), *args, C.c_void_p(src.ptr), NORM_NHWC) == 0    # in place
    assert np.array_equal(dst.numpy(), want) and np.array_equal(src.numpy(), want)
    assert lib.rfi_norm_apply(ctx.handle, C.c_void_p(src.ptr), *args, C.c_void_p(src.ptr), NORM_NCHW) != 0    # other layout
    assert b"overlap" in lib.rfi_last_error()


# ---------------------------------------------------------------- RFIMaskDataset and the training chain
def _write_dir(root, golden):
    gi = golden["inputs"]
    for name, x, m in zip(gi["names"], gi["inputs"], gi["masks"]):
        d = os.path.join(root, str(name))
        os.makedirs(d)
        np.save(os.path.join(d, "input.npy"), x)
        np.save(os.path.join(d, "rfi_mask.npy"), m)
    return [str(n) for n in gi["names"]]


@pytest.mark.parametrize("method", R.METHODS)
def test_rfi_mask_dataset_reproduces_reference(golden, tmp_path, method):
    from rfi_toolbox_amd.datasets import RFIMaskDataset
    names = _write_dir(str(tmp_path), golden)
    ds = RFIMaskDataset(str(tmp_path), normalization=method, device="cuda:0")
    assert len(ds) == 4 and [os.path.basename(d) for d in ds.sample_dirs] == \
        [d for d in os.listdir(str(tmp_path)) if os.path.isdir(os.path.join(str(tmp_path), d))]
    R.check_attrs({k: getattr(ds, k) for k in ATTRS}, R.golden_attrs(golden["expected"], "four.", method), method, "dataset")
    g = golden["dataset_" + method]
    order = [names.index(os.path.basename(d)) for d in ds.sample_dirs]              # this machine's listdir order
    items = np.stack([ds[i][0].numpy() for i in range(4)])
    masks = np.stack([ds[i][1].numpy() for i in range(4)])
    x0, m0 = ds[0]
    assert x0.dtype == torch.float32 and tuple(x0.shape) == (8, 64, 64) and m0.dtype == torch.float32 and tuple(m0.shape) == (1, 64, 64)
    R.check_outputs(items, g["items"][order], method, "RFIMaskDataset items")
    assert np.array_equal(masks, g["masks"][order])
    assert ds.images.shape == (4, 64, 64, 8) and ds.images.dtype == np.float32
    assert ds.labels.shape == (4, 64, 64) and ds.labels.dtype == np.uint8
    assert np.array_equal(ds.labels, golden["inputs"]["masks"][order].astype(np.uint8))
    assert np.array_equal(ds.device_images().numpy(), ds.images) and np.array_equal(ds.device_labels().numpy(), ds.labels)
    flipped = RFIMaskDataset(str(tmp_path), transform=lambda a, b: (a.flip(-1), b.flip(-1)), normalization=method, device="cuda:0")
    assert torch.equal(flipped[1][0], ds[1][0].flip(-1)) and torch.equal(flipped[1][1], ds[1][1].flip(-1))


def test_rfi_mask_dataset_through_training_and_evaluation(golden, tmp_path):
    from rfi_toolbox_amd.datasets import RFIMaskDataset
    from rfi_toolbox_amd.models import UNet
    from rfi_toolbox_amd.training import evaluate_rfi_model, train_rfi_model
    _write_dir(str(tmp_path), golden)
    ds = RFIMaskDataset(str(tmp_path), normalization="robust_scale", device="cuda:0")
    torch.manual_seed(3)
    model = UNet(8, 1, 4, device="cuda:0")
    hist = train_rfi_model(model, ds, ds, num_epochs=1, batch_size=2, lr=1e-3, log=lambda s: None)
    assert len(hist) == 1 and np.isfinite(hist[0]["train_loss"]) and np.isfinite(hist[0]["val_loss"])
    metrics = evaluate_rfi_model(model, ds, batch_size=2)
    assert set(metrics) == {"iou", "precision", "recall", "f1", "dice"} and all(0.0 <= v <= 1.0 for v in metrics.values())


@pytest.mark.parametrize("method", R.METHODS)
def test_generate_normalise_train_chain(method):
    """generate_batch(out="complex128") -> fit_transform(out="nhwc") -> UNet(8, 1, 4).train_step, all in HBM"""
    from rfi_toolbox_amd.core import RFISimulator
    from rfi_toolbox_amd.models import UNet
    batch = RFISimulator(64, 64, seed=11, device="cuda:0").generate_batch(4, out="complex128")
    x = _norm(method).fit_transform(batch.data, out="nhwc")
    torch.manual_seed(0)
    loss = UNet(8, 1, 4, device="cuda:0").train_step(x, batch.mask)
    assert np.isfinite(loss)
    raw = np.abs(R.to_nchw(batch.data.numpy())).max()
    assert raw > 100.0 and np.abs(x.numpy()).max() < raw                       # the raw input spans orders of magnitude
    if method != "standardize":
        _, (want,) = R.normalize_dataset([batch.data.numpy()], method)
        host = np.ascontiguousarray(want.transpose(0, 2, 3, 1))
        torch.manual_seed(0)
        ref_loss = UNet(8, 1, 4, device="cuda:0").train_step(host, batch.mask.numpy())
        assert np.float32(loss).tobytes() == np.float32(ref_loss).tobytes(), (loss, ref_loss)
