"""-m gpu: every public entry point whose array plumbing goes through runtime.operand gives, for the same data as a NumPy
array, a torch CPU tensor, a torch CUDA tensor (contiguous, and as a transposed-then-sliced view) and a DeviceArray, the
result of the NumPy call bit for bit; inputs of another context or GPU are refused; result buffers have the documented
types and keep their inputs alive."""
import gc
import weakref

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FORMS = ("torch", "cuda", "cuda-view", "device")
HOST_FORMS = ("torch", "device")                     # for the entry points that take no CUDA tensor


@pytest.fixture(scope="module")
def ctx():
    from rfi_toolbox_amd.runtime import Context
    return Context.get(0)


@pytest.fixture(scope="module")
def data():
    """The inputs every case shares (never modified): 2 planes of 8 x 16, 256 flat elements as 16 x 16."""
    rng = np.random.default_rng(5)
    d = {"values": rng.standard_normal((2, 8, 16)).astype(np.float32),
         "flags": rng.random((2, 8, 16)) < 0.3,
         "scores": rng.random((16, 16)).astype(np.float32),
         "pred": (rng.random((16, 16)) < 0.5).astype(np.uint8),
         "true": (rng.random((16, 16)) < 0.4).astype(np.uint8),
         "vis": (rng.standard_normal((16, 16)) + 1j * rng.standard_normal((16, 16))).astype(np.complex64),
         "vflags": rng.random((16, 16)) < 0.2,
         "norm": rng.standard_normal((2, 8, 4, 4)).astype(np.float32),
         "images": rng.standard_normal((2, 8, 16, 3)).astype(np.float32),
         "labels": (rng.random((2, 8, 16)) < 0.3).astype(np.uint8),
         "features": rng.standard_normal((1, 4, 4, 4)).astype(np.float32),
         "rois": np.array([[0, 0.5, 0.25, 3.0, 2.5], [0, 1.0, 1.0, 3.5, 3.75]], np.float32)}
    d["values"][0, 3, 4:9] += 6.0
    for v in d.values():
        v.setflags(write=False)
    return d


def _form(a, form, ctx):
    """`a` in another form holding the same values."""
    if form == "torch":
        return torch.from_numpy(a.copy())
    if form == "cuda":
        return torch.from_numpy(a.copy()).cuda()
    if form == "cuda-view":                          # the transpose of a wider tensor, every other row: same values, no stride 1 layout
        t = torch.from_numpy(a.copy()).cuda()
        wide = torch.zeros(t.shape[:-2] + (t.shape[-1], 2 * t.shape[-2]), dtype=t.dtype, device=t.device)
        wide[..., ::2] = t.transpose(-1, -2)
        v = wide.transpose(-1, -2)[..., ::2, :]
        assert not v.is_contiguous() and torch.equal(v, t)
        return v
    return ctx.to_device(a.view(np.uint8) if a.dtype == np.bool_ else a)


def _host(r):
    """A result as NumPy (tuples element by element)."""
    from rfi_toolbox_amd.runtime import DeviceArray
    if isinstance(r, (tuple, list)):
        return tuple(_host(x) for x in r)
    if isinstance(r, DeviceArray):
        return r.numpy()
    if isinstance(r, torch.Tensor):
        return r.cpu().numpy()
    return np.asarray(r)


def _same(got, want, what):
    got, want = _host(got), _host(want)
    if isinstance(want, tuple):
        assert len(got) == len(want), what
        for g, w in zip(got, want):
            _same(g, w, what)
        return
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert got.tobytes() == want.tobytes(), what


def _entry_points(data):
    """name -> (call(*arrays), names of its array arguments in `data`, the forms it takes today)."""
    from rfi_toolbox_amd import components, flagging
    from rfi_toolbox_amd.evaluation import flag_statistics
    from rfi_toolbox_amd.evaluation.metrics import confusion_counts
    from rfi_toolbox_amd.evaluation.sweep import threshold_sweep
    from rfi_toolbox_amd.models.detection_ops import roi_align
    from rfi_toolbox_amd.preprocessing.normalization import Normalizer
    from rfi_toolbox_amd.training import Augmenter

    def sweep(s, t):
        r = threshold_sweep(s, t, thresholds=[0.25, 0.5, 0.75])
        return r.tp, r.fp, r.fn

    def stats(z, f):
        a, c = flag_statistics(z, f)
        return np.array(a[:8], np.float64), np.array(c[:8], np.float64)

    return {
        "confusion_counts": (lambda p, t: np.array(confusion_counts(p, t)), ("pred", "true"), FORMS),
        "threshold_sweep": (sweep, ("scores", "true"), FORMS),
        "flag_statistics": (stats, ("vis", "vflags"), FORMS),
        "label_components": (lambda m: components.label_components(m), ("flags",), FORMS),
        "remove_small_components": (lambda m: components.remove_small_components(m, 3, out="device"), ("flags",), FORMS),
        "sumthreshold_pass": (lambda v, f: flagging.sumthreshold_pass(v, f, 4, 1.5), ("values", "flags"), FORMS),
        "extend_flags": (lambda f: flagging.extend_flags(f, growaround=True, flagneartime=True, growtime=30.0, out="device"),
                         ("flags",), FORMS),
        "Normalizer.fit_transform": (lambda x: Normalizer("standardize", scope="sample", device=0).fit_transform(x, out="nhwc"),
                                     ("norm",), HOST_FORMS),
        "Augmenter.__call__": (lambda x, y: Augmenter(seed=3, device=0)(x, y, call=1), ("images", "labels"), FORMS),
        "roi_align": (lambda x: roi_align(x, data["rois"], output_size=(2, 2), device=0), ("features",), HOST_FORMS),
    }


ENTRY_POINTS = ("confusion_counts", "threshold_sweep", "flag_statistics", "label_components", "remove_small_components",
                "sumthreshold_pass", "extend_flags", "Normalizer.fit_transform", "Augmenter.__call__", "roi_align")


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_every_input_form_gives_the_numpy_result(name, data, ctx):
    call, args, forms = _entry_points(data)[name]
    arrays = [data[a] for a in args]
    want = _host(call(*arrays))
    assert any(np.asarray(w).any() for w in (want if isinstance(want, tuple) else (want,))), "the case shows nothing"
    for form in forms:
        _same(call(*(_form(a, form, ctx) for a in arrays)), want, f"{name} {form}")
    if len(arrays) == 2:                                                 # mixed: a CUDA view with a host array
        _same(call(_form(arrays[0], "cuda-view", ctx), arrays[1]), want, f"{name} mixed")


def _five():
    """The entry points that did not all refuse foreign memory before: name -> call(first, second, device)."""
    from rfi_toolbox_amd import components, flagging
    from rfi_toolbox_amd.evaluation import flag_statistics
    from rfi_toolbox_amd.evaluation.metrics import confusion_counts
    from rfi_toolbox_amd.evaluation.sweep import threshold_sweep
    return {"confusion_counts": (lambda a, b, device: confusion_counts(a, b, device=device), ("pred", "true")),
            "threshold_sweep": (lambda a, b, device: threshold_sweep(a, b, device=device), ("scores", "true")),
            "flag_statistics": (lambda a, b, device: flag_statistics(a, b, device=device), ("vis", "vflags")),
            "sumthreshold_pass": (lambda a, b, device: flagging.sumthreshold_pass(a, b, 4, 1.5, device=device), ("values", "flags")),
            "label_components": (lambda a, b, device: components.label_components(b, device=device), ("values", "flags"))}


def test_device_arrays_of_another_context_are_refused(data, ctx):
    from rfi_toolbox_amd.runtime import Context
    other = Context(0)                               # a second context (one more stream) on the same GPU; collected, not destroyed
    assert other is not ctx
    for name, (call, args) in _five().items():
        a, b = (data[k] for k in args)
        mine = [_form(x, "device", ctx) for x in (a, b)]
        theirs = [_form(x, "device", other) for x in (a, b)]
        with pytest.raises(ValueError, match="another context"):          # device=0 names the cached context
            call(*theirs, device=0)
        if name != "label_components":                                    # two inputs of two contexts
            with pytest.raises(ValueError, match="another context"):
                call(mine[0], theirs[1], device=None)
            with pytest.raises(ValueError, match="another context"):
                call(theirs[0], mine[1], device=None)
        call(*mine, device=0)                                             # and the context stays usable


def test_tensors_on_another_gpu_are_refused(data):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    for name, (call, args) in _five().items():
        a, b = (torch.from_numpy(data[k].copy()).to("cuda:1") for k in args)
        with pytest.raises(ValueError, match="tensor is on cuda:1, the context on GPU 0"):
            call(a, b, device=0)


def test_extend_flags_result_buffers(data, ctx):
    from rfi_toolbox_amd.flagging import extend_flags
    from rfi_toolbox_amd.runtime import DeviceArray
    f = data["flags"]
    want = extend_flags(f, flagneartime=True)
    assert isinstance(want, np.ndarray) and want.dtype == np.bool_ and want.shape == f.shape and (want & ~f).any()
    for form in ("numpy", "cuda", "device"):
        x = f if form == "numpy" else _form(f, form, ctx)
        got = extend_flags(x, flagneartime=True, out="host")
        if form == "cuda":
            assert isinstance(got, torch.Tensor) and got.dtype == torch.bool and got.device == x.device
        else:
            assert isinstance(got, np.ndarray) and got.dtype == np.bool_
        _same(got, want, f"host {form}")
        got = extend_flags(x, flagneartime=True, out="device")
        assert isinstance(got, DeviceArray) and got.dtype == np.uint8 and got.shape == f.shape and got.ctx is ctx
        _same(got, want.view(np.uint8), f"device {form}")


def test_device_results_keep_their_inputs(data, ctx):
    from rfi_toolbox_amd.components import label_components
    from rfi_toolbox_amd.flagging import extend_flags, sumthreshold_flags
    f = data["flags"]
    want = extend_flags(f, flagneartime=True).view(np.uint8)
    # a DeviceArray input: the result holds the very object
    d = ctx.to_device(f.view(np.uint8))
    ref = weakref.ref(d)
    res = extend_flags(d, flagneartime=True, out="device")
    del d
    gc.collect()
    assert ref() is not None and res._keep[0] is ref() and res._keep[1] is None
    _same(res, want, "kept DeviceArray")
    # a CUDA tensor input: the result holds a tensor on the caller's memory
    t = torch.from_numpy(f.copy()).cuda()
    ptr = t.data_ptr()
    res = extend_flags(t, flagneartime=True, out="device")
    del t
    gc.collect()
    kept = res._keep[0]
    assert isinstance(kept, torch.Tensor) and kept.data_ptr() == ptr and np.array_equal(kept.cpu().numpy(), f.view(np.uint8))
    _same(res, want, "kept tensor")
    # data and prior flags: both are held
    z, p = ctx.to_device(data["vis"]), ctx.to_device(data["vflags"].view(np.uint8))
    refs = weakref.ref(z), weakref.ref(p)
    res = sumthreshold_flags(z, p, out="device")
    del z, p
    gc.collect()
    assert res._keep[0] is refs[0]() is not None and res._keep[1] is refs[1]() is not None
    # label_components: the labels hold the input
    m = ctx.to_device(f.view(np.uint8))
    ref = weakref.ref(m)
    labels, k = label_components(m, out="device")
    del m
    gc.collect()
    assert labels._keep is ref() is not None
    _same((labels, k), label_components(f), "kept labels")
