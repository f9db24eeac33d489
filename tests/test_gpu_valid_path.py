"""Prior flags and non-finite samples through the 8-channel path on the GPU (include/rfi_hip.h, "validity-aware
8-channel input"): rfi_valid_map, rfi_valid_statistics, rfi_valid_apply, rfi_valid_gather and
rfi_model_predict_flags_valid, and the Python surface over them, against the NumPy restatement tests/valid_norm_ref.py.

Working shape: 3 samples of (4, 40, 52), 16640 scalars each -- two 8192-scalar sum tiles and a ragged third, a
non-square plane, nothing a multiple of 64; (4, 77, 50) too for the gather and the prediction.  About 10 % random prior
flags plus planted NaN (real parts only), +inf (imaginary parts only) and -inf (tests/valid_path_cases.py).

Tolerances: the map, count, min, max, the six brackets, the min-max and robust outputs, the filled places, the tiles and
the prediction are compared bit for bit; mean and std within 1e-12 relative and the standardize outputs within 1
float32 ulp in a share of at most 1e-3 of the elements (normalize_ref's bounds; test_valid_path_host.py checks on these
very inputs that moments formed by np.mean / np.var stay inside that cap)."""
import ctypes as C

import numpy as np
import pytest
import torch

import normalize_ref as nref
import valid_norm_ref as V
import valid_path_cases as cases

pytestmark = pytest.mark.gpu

PS = 32
FORMS = [(k, pb) for k in cases.KINDS for pb in (False, True)]


def _norm(*a, **k):
    from rfi_toolbox_amd.preprocessing import Normalizer
    return Normalizer(*a, device="cuda:0", **k)


def _ctx():
    from rfi_toolbox_amd.runtime import Context
    return Context.get("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _nhwc_to_nchw(a):
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2))


def _same_record(got, want, label=""):
    """count, min, max and the brackets equal; mean and std within 1e-12 relative (NaN record: NaN everywhere)"""
    assert got["count"] == want["count"], (label, got["count"], want["count"])
    if want["count"] == 0:
        assert all(np.isnan(got[k]) for k in ("min", "max", "mean", "var")) and np.isnan(np.array(got["q"])).all(), (label, got)
        return
    assert got["min"] == want["min"] and got["max"] == want["max"], (label, got, want)
    assert got["q"] == want["q"], (label, got["q"], want["q"])
    assert abs(got["mean"] - want["mean"]) <= nref.REL_MOMENT * abs(want["mean"]), (label, got["mean"], want["mean"])
    gs, ws = np.sqrt(got["var"]), np.sqrt(want["var"])
    assert abs(gs - ws) <= nref.REL_MOMENT * ws, (label, gs, ws)


def _identical(a, b):
    """two lists of records, bit for bit (NaN == NaN)"""
    return repr(a) == repr(b)


# ---------------------------------------------------------------- 1: the map
def _device_map(x, layout, flags):
    from rfi_toolbox_amd._lib import NORM_NCHW, NORM_NHWC, VALID_FLAGS_BASELINE, VALID_FLAGS_POL, VALUE_CODES, check, lib
    ctx = _ctx()
    n, px = len(x), cases.SHAPE[0] * cases.SHAPE[1]
    src = ctx.to_device(x)
    fl = None if flags is None else ctx.to_device(flags)
    vmap = ctx.empty((n, 4, px), np.uint8)
    counts = np.full(n, -1, dtype=np.int64)
    check(lib.rfi_valid_map(ctx.handle, C.c_void_p(src.ptr), VALUE_CODES[np.dtype(x.dtype)], NORM_NHWC if layout == "nhwc" else NORM_NCHW,
                            n, px, None if fl is None else C.c_void_p(fl.ptr),
                            VALID_FLAGS_BASELINE if flags is not None and flags.ndim == 3 else VALID_FLAGS_POL, C.c_void_p(vmap.ptr),
                            counts.ctypes.data_as(C.c_void_p), 0))
    return vmap.numpy().reshape((n, 4) + cases.SHAPE), counts


@pytest.mark.parametrize("kind,per_baseline", FORMS)
def test_map_equals_restatement(kind, per_baseline):
    x, layout, f = cases.working(kind, per_baseline)
    want = V.invalid_map(x, f, layout)
    got, counts = _device_map(x, layout, f)
    assert np.array_equal(got, want.astype(np.uint8)) and counts.tolist() == want.reshape(3, -1).sum(axis=1).tolist()
    got, counts = _device_map(x, layout, None)                                         # no prior flags: non-finite only
    want = V.invalid_map(x, None, layout)
    assert np.array_equal(got, want.astype(np.uint8)) and counts.tolist() == [15, 15, 15]


# ---------------------------------------------------------------- 2: statistics
@pytest.mark.parametrize("kind,per_baseline", FORMS)
def test_statistics_of_the_valid_scalars(kind, per_baseline):
    x, layout, f = cases.working(kind, per_baseline)
    got = _norm("robust_scale", scope="sample").statistics(x, layout, flags=f)
    want = V.sample_stats(x, f, layout)
    assert len(got) == 3
    for i in range(3):
        assert 0 < want[i]["count"] < 16640
        _same_record(got[i], want[i], f"sample {i}")
    _same_record(_norm("robust_scale").statistics(x, layout, flags=f)[0], V.dataset_stats([x], [f], [layout]), "dataset")
    only = _norm("robust_scale", scope="sample").statistics(x, layout, flags="nonfinite")
    assert [s["count"] for s in only] == [16640 - 30] * 3
    _same_record(only[1], V.sample_stats(x, None, layout)[1], "nonfinite")
    moments = _norm("standardize", scope="sample").statistics(x, layout, quantiles=False, flags=f)      # two passes, no quantiles
    for g, m in zip(got, moments):
        assert (m["count"], m["min"], m["max"], m["mean"], m["var"]) == (g["count"], g["min"], g["max"], g["mean"], g["var"])
        assert np.isnan(np.array(m["q"])).all()


@pytest.mark.parametrize("kind", cases.KINDS)
def test_statistics_without_an_invalid_scalar_are_the_unmasked_ones(kind):
    x, layout = cases.as_kind(cases.observation(seed=4), kind)
    for scope in ("sample", "dataset"):
        plain = _norm("robust_scale", scope=scope).statistics(x, layout)
        assert plain == _norm("robust_scale", scope=scope).statistics(x, layout, flags="nonfinite")
        assert plain == _norm("robust_scale", scope=scope).statistics(x, layout, flags=np.zeros((3,) + cases.SHAPE, bool))
        assert plain == _norm("robust_scale", scope=scope).statistics(x, layout, flags=np.zeros((3, 4) + cases.SHAPE, np.uint8))
    assert _norm("standardize").fit(x, layout).state_dict() == _norm("standardize").fit(x, layout, flags="nonfinite").state_dict()


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_statistics_of_planted_populations(dtype):
    d, f = cases.planted(dtype)
    got = _norm("robust_scale", scope="sample").statistics(d, flags=f)
    want = V.sample_stats(d, f)
    for name, g, w in zip(cases.PLANTED, got, want):
        _same_record(g, w, name)
    assert [g["count"] for g in got[:6]] == [0, 2, 4, 6, 2000, 2002]
    i = cases.PLANTED.index("all_equal")
    assert got[i]["min"] == got[i]["max"] == got[i]["mean"] == 2.0 and got[i]["var"] == 0.0 and got[i]["q"] == ((2.0, 2.0),) * 3
    for method in nref.METHODS:
        nz = _norm(method, scope="sample").fit(d, flags=f)
        pairs = V.sample_pairs(d, method, f)
        for name, c, s, w in zip(cases.PLANTED, nz.centres, nz.scales, pairs):
            if w is None:
                assert (c, s) == (0.0, 0.0), (method, name)
            elif method == "standardize":
                assert abs(c - w[0]) <= nref.REL_MOMENT * abs(w[0]) and abs(s - w[1]) <= nref.REL_MOMENT * abs(w[1]), (name, c, s, w)
            else:
                assert (c, s) == w, (method, name, c, s, w)
        assert (nz.centres[0], nz.scales[0]) == (0.0, 0.0)                            # no valid scalar: the all-zeros transform
        out = nz.transform(d, out="nchw", flags=f, fill=-1.5)
        assert np.isfinite(out).all() and (out[0] == np.float32(-1.5)).all()


def test_statistics_do_not_depend_on_chunking_or_on_the_batch():
    d, f = cases.planted()
    w, _, wf = cases.working("c128")
    d, f = np.concatenate([d, w]), np.concatenate([f, wf])                            # 12 samples
    whole = _norm("robust_scale").statistics(d, flags=f)
    _same_record(whole[0], V.dataset_stats([d], [f]), "dataset of 12")
    assert _identical(whole, _norm("robust_scale").statistics(d, flags=f))            # two runs
    for cuts in ((3, 4), (1, 2, 11), (5,)):
        parts, fparts = np.split(d, cuts), np.split(f, cuts)
        assert _identical(_norm("robust_scale").statistics(parts, flags=fparts), whole), cuts
    mixed = [d[:5], cases.as_kind(d[5:], "f64_nchw")[0]]                              # a planar chunk, per-baseline flags on it
    base = np.concatenate([f[:5].any(axis=1), f[5:].any(axis=1)])
    want = _norm("robust_scale").statistics(d, flags=base)[0]
    got = _norm("robust_scale").statistics(mixed, flags=[base[:5], base[5:]])[0]        # (other scalar order: other sum order)
    assert all(repr(got[k]) == repr(want[k]) for k in ("count", "min", "max", "q"))
    _same_record(got, want, "mixed forms")
    per = _norm("robust_scale", scope="sample").statistics(d, flags=f)
    for i in (0, 4, 6, 10):
        assert _identical([per[i]], _norm("robust_scale", scope="sample").statistics(d[i:i + 1], flags=f[i:i + 1])), i


# ---------------------------------------------------------------- 3: the transform
@pytest.mark.parametrize("kind,per_baseline", FORMS)
def test_transform_fills_the_invalid_and_keeps_the_rest(kind, per_baseline):
    x, layout, f = cases.working(kind, per_baseline)
    bad = np.repeat(V.invalid_map(x, f, layout), 2, axis=1)
    for method, scope in [(m, s) for m in nref.METHODS for s in ("sample", "dataset")]:
        for fill in (0.0, -1.5):
            nz = _norm(method, scope=scope)
            nchw = nz.fit_transform(x, out="nchw", layout=layout, flags=f, fill=fill)
            nhwc = nz.transform(x, out="nhwc", layout=layout, flags=f, fill=fill)
            assert np.array_equal(_bits(_nhwc_to_nchw(nhwc)), _bits(nchw)), (method, scope)
            assert np.array_equal(_bits(nchw[bad]), _bits(np.full(int(bad.sum()), fill, np.float32))) and np.isfinite(nchw).all()
            pairs = V.sample_pairs(x, method, f, layout) if scope == "sample" else [V.dataset_pair(x, method, f, layout)[1]] * 3
            nref.check_outputs(nchw, V.transform(x, pairs, f, fill, layout), method, f"{kind} {scope} {method} fill {fill}")


def test_transform_on_the_device_in_place_and_without_flags():
    from rfi_toolbox_amd._lib import F32, NORM_NCHW, NORM_NHWC, check, lib
    from rfi_toolbox_amd.runtime import DeviceArray
    ctx = _ctx()
    x, layout, f = cases.working("f32_nhwc")
    n, px = 3, cases.SHAPE[0] * cases.SHAPE[1]
    bad = V.invalid_map(x, f, layout)
    want = V.transform(x, [(0.25, 3.0)] * 3, f, -1.5, layout)                        # (n, 8, T, F)
    src, vmap, dst = ctx.to_device(x), ctx.to_device(bad.astype(np.uint8)), ctx.empty(x.shape, np.float32)
    args = (F32, NORM_NHWC, n, px, 0.25, 3.0, None, C.c_void_p(vmap.ptr), -1.5)
    check(lib.rfi_valid_apply(ctx.handle, C.c_void_p(src.ptr), *args, C.c_void_p(dst.ptr), NORM_NHWC))
    check(lib.rfi_valid_apply(ctx.handle, C.c_void_p(src.ptr), *args, C.c_void_p(src.ptr), NORM_NHWC))               # in place
    assert np.array_equal(_bits(_nhwc_to_nchw(dst.numpy())), _bits(want)) and np.array_equal(_bits(src.numpy()), _bits(dst.numpy()))
    assert lib.rfi_valid_apply(ctx.handle, C.c_void_p(src.ptr), *args, C.c_void_p(src.ptr), NORM_NCHW) != 0          # other layout
    assert b"overlap" in lib.rfi_last_error()
    # DeviceArray in, DeviceArray out
    z, _, fz = cases.working("c128")
    nz = _norm("robust_scale", scope="sample")
    out = nz.fit_transform(ctx.to_device(z), out="nchw", flags=ctx.to_device(fz), fill=-1.5)
    assert isinstance(out, DeviceArray)
    assert np.array_equal(_bits(out.numpy()), _bits(nz.transform(z, out="nchw", flags=torch.from_numpy(fz).bool(), fill=-1.5)))
    # without flags: the existing entry point, bit for bit
    clean = cases.observation(seed=5)
    nz = _norm("robust_scale").fit(clean)
    got = nz.transform(clean, out="nhwc")
    d, o = ctx.to_device(clean), ctx.empty((3,) + cases.SHAPE + (8,), np.float32)
    from rfi_toolbox_amd._lib import C128
    check(lib.rfi_norm_apply(ctx.handle, C.c_void_p(d.ptr), C128, NORM_NCHW, 3, px, nz.centres[0], nz.scales[0], None, C.c_void_p(o.ptr),
                             NORM_NHWC))
    assert np.array_equal(_bits(got), _bits(o.numpy()))
    assert np.array_equal(_bits(got), _bits(nz.transform(clean, out="nhwc", flags="nonfinite")))       # nothing invalid: the same


def test_normalize_array_with_flags():
    from rfi_toolbox_amd.preprocessing import normalize_array
    x, layout, f = cases.working("f64_nchw")
    for flags in (f[1], f[1].any(axis=0).astype(np.uint8), "nonfinite"):
        fl = None if isinstance(flags, str) else flags[None]
        got = normalize_array(x[1], "robust_scale", flags=flags, fill=-1.5)
        want = V.transform(x[1:2], V.sample_pairs(x[1:2], "robust_scale", fl, layout), fl, -1.5, layout)[0]
        assert got.shape == (8,) + cases.SHAPE and np.array_equal(_bits(got), _bits(want))
    with pytest.raises(ValueError, match="non-finite"):
        normalize_array(x[1], "robust_scale")


# ---------------------------------------------------------------- 4: the gather
def _normalizers(data, flags, fl):
    """(what to pass, one (centre, scale) or None per sample) for: none, a fitted dataset scope, a sample scope"""
    ds = _norm("standardize").fit(data, flags=flags)
    return [(None, [(0.0, 1.0)] * len(data)), (ds, [(ds.centres[0], ds.scales[0])] * len(data)),
            (_norm("robust_scale", scope="sample"), V.sample_pairs(data, "robust_scale", fl))]


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("shape", [cases.SHAPE, cases.SHAPE2])
def test_gather_is_the_restatement_transform_cut(shape, dtype):
    from rfi_toolbox_amd.inference import tile_observation
    data, _, f = cases.working("c128" if dtype == np.complex128 else "c64", False, shape, seed=shape[0])
    fb = cases.prior_flags(data.shape, 9, per_baseline=True)
    for flags in (f, fb, "nonfinite"):
        fl = None if isinstance(flags, str) else flags
        for nz, pairs in _normalizers(data, flags, fl):
            for ps in (32, 48):
                for edge in ("pad", "shift"):
                    for fill in (0.0, -1.5):
                        want = V.tile(data, pairs, ps, 24, 4, edge, fl, fill)
                        got = tile_observation(data, ps, 24, 4, edge, normalizer=nz, flags=flags, fill=fill).numpy()
                        assert got.shape == want.shape and np.isfinite(got).all()
                        assert np.array_equal(_bits(got), _bits(want)), (ps, edge, fill, int((_bits(got) != _bits(want)).sum()))
    one = tile_observation(data[1], 32, 24, 4, normalizer=_norm("robust_scale", scope="sample"), flags=fb[1]).numpy()     # (4, C, T)
    pairs = V.sample_pairs(data, "robust_scale", fb)
    assert np.array_equal(_bits(one), _bits(V.tile(data[1:2], pairs[1:2], 32, 24, 4, "pad", fb[1:2])))


def test_gather_padding_and_flag_operands():
    from rfi_toolbox_amd._lib import COMPLEX_CODES, DEVICE, HOST, VALID_FLAGS_POL, check, lib
    from rfi_toolbox_amd.inference import tile_observation, tiling_table
    ctx = _ctx()
    data, _, f = cases.working("c64", False, cases.SHAPE2, seed=3)
    n, (Cn, Tn) = 3, cases.SHAPE2
    plain = tile_observation(np.nan_to_num(data, nan=1.0, posinf=1.0, neginf=1.0), 48, 24, 4, normalizer=_norm("standardize").fit(
        data, flags=f)).numpy()
    nz = _norm("standardize").fit(data, flags=f)
    got = tile_observation(data, 48, 24, 4, normalizer=nz, flags=f, fill=-1.5).numpy()
    table = tiling_table(n, Cn, Tn, 48, 24, 4)
    pad = np.zeros(got.shape[:3], bool)
    for e, (_, v, r0, c0) in enumerate(table):
        H, W = (Cn, Tn) if v < 2 else (Tn, Cn)
        pad[e, max(0, H - r0):, :] = True
        pad[e, :, max(0, W - c0):] = True
    assert pad.any() and np.array_equal(_bits(got[pad]), _bits(plain[pad]))             # padding pixels: unchanged, never `fill`
    assert (got[pad] == np.float32((0.0 - nz.centres[0]) / nz.scales[0])).all()
    # prior flags as a host and as a device operand of the entry point
    outs = []
    d = ctx.to_device(data)
    for ptr, mem, keep in ((f.ctypes.data, HOST, f), (None, DEVICE, ctx.to_device(f))):
        out = ctx.empty(got.shape, np.float32)
        check(lib.rfi_valid_gather(ctx.handle, C.c_void_p(d.ptr), DEVICE, COMPLEX_CODES[np.dtype(np.complex64)], n, Cn, Tn,
                                   table.ctypes.data_as(C.c_void_p), len(table), 48, nz.centres[0], nz.scales[0], None,
                                   C.c_void_p(ptr if ptr is not None else keep.ptr), mem, VALID_FLAGS_POL, -1.5, C.c_void_p(out.ptr), DEVICE))
        outs.append(out.numpy())
    assert np.array_equal(_bits(outs[0]), _bits(got)) and np.array_equal(_bits(outs[1]), _bits(got))


# ---------------------------------------------------------------- 5: the prediction
def _unet(out_ch=1, seed=0):
    from rfi_toolbox_amd.models import UNet
    torch.manual_seed(seed)
    return UNet(8, out_ch, 4, device="cuda:0").eval()


def _normalizer(form, data, flags):
    if form == "none":
        return None
    if form == "dataset":
        return _norm("standardize").fit(data, flags=flags)
    return _norm(form, scope="sample")


def _composition(model, data, nz, flags, fill, thr, batch, combine="mean"):
    """tile_observation(flags=) -> the model, `batch` tiles at a time as predict_flags runs it -> stitch_patches"""
    from rfi_toolbox_amd.inference import stitch_patches, tile_observation
    tiles = tile_observation(data, PS, 24, 4, normalizer=nz, flags=flags, fill=fill).numpy()
    assert len(tiles) % batch == 0
    out = np.concatenate([model.forward_nhwc(tiles[i:i + batch]) for i in range(0, len(tiles), batch)])
    Cn, Tn = data.shape[-2:]
    return stitch_patches(out, Cn, Tn, PS, 24, 4, combine=combine, threshold=thr, return_probabilities=True)


@pytest.mark.parametrize("shape", [cases.SHAPE2, cases.SHAPE])
@pytest.mark.parametrize("form", ["none", "dataset", "robust_scale"])
def test_predict_flags_with_prior_flags_equals_the_composition(form, shape):
    from rfi_toolbox_amd.inference import predict_flags, tiling_count
    model = _unet()
    data, _, f = cases.working("c64", False, shape, seed=11)
    ppp = tiling_count(shape[0], shape[1], PS, 24, 4)                # one baseline's tiles: the forward batch of both paths
    fb = cases.prior_flags(data.shape, 12, per_baseline=True)
    for flags, fill in ((f, 0.0), (fb, -1.5), ("nonfinite", 0.0)):
        nz = _normalizer(form, data, flags)
        kw = dict(patch_size=PS, stride=24, views=4, batch_size=ppp, normalizer=nz, flags=flags, fill=fill, return_probabilities=True)
        _, p0 = predict_flags(model, data, broadcast_pols=False, **kw)
        assert np.isfinite(p0).all()                                 # although the data holds NaN and infinities
        thr = float(np.median(p0))
        wf, wp = _composition(model, data, nz, flags, fill, thr, ppp)
        mf, p = predict_flags(model, data, broadcast_pols=False, threshold=thr, **kw)
        assert mf.shape == (3,) + shape and mf.dtype == bool and 0 < mf.sum() < mf.size
        assert np.array_equal(_bits(p), _bits(wp)) and np.array_equal(mf, wf)          # the model's flags alone
        merged, p2 = predict_flags(model, data, threshold=thr, **kw)
        invalid = V.invalid_map(data, None if isinstance(flags, str) else flags)
        assert merged.shape == data.shape and merged.dtype == bool and p2.tobytes() == p.tobytes()
        assert np.array_equal(merged, mf[:, None] | invalid) and merged[invalid].all()
        again, p3 = predict_flags(model, data, threshold=thr, **kw)                     # run twice
        assert again.tobytes() == merged.tobytes() and p3.tobytes() == p.tobytes()


def test_predict_flags_input_forms_groups_and_class_bits(monkeypatch):
    from rfi_toolbox_amd import inference
    from rfi_toolbox_amd.runtime import DeviceArray
    model = _unet()
    data, _, f = cases.working("c128", False, cases.SHAPE, seed=13)
    ppp = inference.tiling_count(cases.SHAPE[0], cases.SHAPE[1], PS, 24, 4)
    nz = _norm("robust_scale", scope="sample")
    kw = dict(patch_size=PS, stride=24, views=4, batch_size=ppp, normalizer=nz, fill=-1.5, return_probabilities=True)
    _, p = inference.predict_flags(model, data, flags=f, **kw)
    kw["threshold"] = float(np.median(p))
    m, p = inference.predict_flags(model, data, flags=f, **kw)
    # device operands and results
    dm, dp = inference.predict_flags(model, model.ctx.to_device(data), flags=model.ctx.to_device(f), out="device", **kw)
    assert isinstance(dm, DeviceArray) and dm.dtype == np.bool_ and dm.numpy().tobytes() == m.tobytes() and dp.numpy().tobytes() == p.tobytes()
    tm, tp = inference.predict_flags(model, torch.from_numpy(data).to("cuda:0"), flags=torch.from_numpy(f).bool().to("cuda:0"), **kw)
    assert tm.is_cuda and tm.dtype == torch.bool and tm.cpu().numpy().tobytes() == m.tobytes() and tp.cpu().numpy().tobytes() == p.tobytes()
    m1, p1 = inference.predict_flags(model, data[1], flags=f[1], **kw)                   # (4, C, T)
    assert m1.shape == (4,) + cases.SHAPE and m1.tobytes() == m[1].tobytes() and p1.tobytes() == p[1].tobytes()
    # several sample groups
    monkeypatch.setattr(inference, "_SAMPLE_GROUP_BYTES", data[0].nbytes)
    assert inference._sample_groups(3, data[0].nbytes) == [(0, 1), (1, 2), (2, 3)]
    for d, fl in ((data, f), (model.ctx.to_device(data), model.ctx.to_device(f))):
        gm, gp = inference.predict_flags(model, d, flags=fl, **kw)
        assert gm.tobytes() == m.tobytes() and gp.tobytes() == p.tobytes()
    monkeypatch.undo()
    # flags=None: unchanged -- a sample-scope normalizer still refuses non-finite input
    with pytest.raises(ValueError, match="non-finite"):
        inference.predict_flags(model, data, **kw)
    # a class-bit model: (B, 2, C, T), unmerged
    two = _unet(2, seed=1).set_targets("class_bits")
    cf, cp = inference.predict_flags(two, data, flags=f, **kw)
    assert cf.shape == (3, 2) + cases.SHAPE and cf.dtype == bool and cp.shape == cf.shape and np.isfinite(cp).all()
    tiles = inference.tile_observation(data, PS, 24, 4, normalizer=nz, flags=f, fill=-1.5).numpy()
    out = np.concatenate([two.forward_nhwc(tiles[i:i + ppp]) for i in range(0, len(tiles), ppp)])
    wf, wp = inference.stitch_patches(out, *cases.SHAPE, PS, 24, 4, threshold=kw["threshold"], return_probabilities=True)
    assert np.array_equal(_bits(cp), _bits(wp)) and np.array_equal(cf, wf)
