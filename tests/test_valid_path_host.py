"""The validity-aware 8-channel input without a GPU: the NumPy restatement (tests/valid_norm_ref.py) against
normalize_ref where nothing is invalid, the ctypes prototypes of the five entry points against the header, the Python
argument checks, and the planted cases of the GPU test (tests/valid_path_cases.py) against what they claim."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import normalize_ref as nref
import pol_tiling_ref as pref
import valid_norm_ref as V
import valid_path_cases as cases

ENTRIES = ("rfi_valid_map", "rfi_valid_statistics", "rfi_valid_apply", "rfi_valid_gather", "rfi_model_predict_flags_valid")


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("kind", cases.KINDS)
def test_restatement_equals_normalize_ref_when_nothing_is_invalid(kind):
    x, layout = cases.as_kind(cases.observation(seed=3), kind)
    assert not V.invalid_map(x, None, layout).any()
    zeros = np.zeros((3,) + cases.SHAPE, dtype=np.uint8)
    planar = nref.to_nchw(x, layout)
    for method in nref.METHODS:
        pairs = V.sample_pairs(x, method, zeros, layout)
        assert pairs == [nref.sample_params(s, method) for s in planar]
        got = V.transform(x, pairs, zeros, -1.5, layout)
        assert np.array_equal(got.view(np.uint32), nref.normalize_samples(x, method, layout).view(np.uint32))
        attrs, pair = V.dataset_pair(x, method, None, layout)
        want_attrs, want_pair = nref.dataset_params([planar], method)
        assert pair == want_pair and attrs == want_attrs
    st = V.sample_stats(x, None, layout)[1]
    v = np.sort(planar[1].ravel())
    assert (st["count"], st["min"], st["max"]) == (v.size, v[0], v[-1]) and (st["mean"], st["var"]) == nref.moments(v)
    assert st["q"][0] == (v[v.size // 2 - 1], v[v.size // 2])


def test_restatement_brackets_are_numpys():
    rng = np.random.default_rng(0)
    for count in (1, 2, 3, 4, 5, 6, 2000, 2002, 16640):
        v = np.sort(rng.standard_normal(count))
        for q in (0.5, 0.25, 0.75):
            lo, hi, t = V.bracket(count, q)
            assert 0 <= lo <= hi < count
            d = v[hi] - v[lo]
            assert (v[hi] - d * (1.0 - t) if t >= 0.5 else v[lo] + d * t) == np.percentile(v, 100 * q)


def test_restatement_fill_padding_and_tiles():
    x, _, f = cases.working("c64")
    bad = V.invalid_map(x, f)
    assert bad.shape == x.shape and bad[f != 0].all() and bad[~np.isfinite(x.real) | ~np.isfinite(x.imag)].all()
    assert 0.09 < bad.mean() < 0.12 and (bad & (f == 0)).sum() >= 15 * 3 * 0.8      # planted values outside the prior flags
    pairs = V.sample_pairs(x, "robust_scale", f)
    out = V.transform(x, pairs, f, -1.5)
    assert np.isfinite(out).all() and (out[np.repeat(bad, 2, axis=1)] == np.float32(-1.5)).all()
    tiles = V.tile(x, pairs, 32, 24, 4, "pad", f, -1.5)
    assert np.isfinite(tiles).all() and tiles.shape[1:] == (32, 32, 8)
    assert tiles[1, 31, 31, 0] == pref.pad_value(pairs[0])          # row0 24 + 31 >= 40: past the view's edge


# ---------------------------------------------------------------- the planted cases hold what they claim
def test_planted_populations():
    d, f = cases.planted()
    assert d.shape == (len(cases.PLANTED), 4) + cases.SHAPE and d[0].size * 2 == 2 * cases.SUM_TILE + 256
    bad = V.invalid_map(d, f)
    visible = [int((~b).sum()) for b in bad]
    assert visible[:6] == [0, 1, 2, 3, 1000, 1001]
    st = V.sample_stats(d, f)
    assert [s["count"] for s in st[:6]] == [0, 2, 4, 6, 2000, 2002] and np.isnan(st[0]["mean"]) and np.isnan(st[0]["q"][2][1])
    assert V.bracket(2000, 0.25)[2] != 0.0 and V.bracket(2002, 0.25)[2] != V.bracket(2000, 0.25)[2]
    i = cases.PLANTED.index("tile_invalid")
    scalars_bad = np.repeat(bad[i].reshape(-1), 2)                   # complex input: scalar 2 k and 2 k + 1 of visibility k
    assert scalars_bad[cases.SUM_TILE: 2 * cases.SUM_TILE].all() and not scalars_bad[:cases.SUM_TILE].any() \
        and not scalars_bad[2 * cases.SUM_TILE:].any()
    i = cases.PLANTED.index("extremes_flagged")
    everything = nref.to_nchw(d[i:i + 1]).ravel()
    assert st[i]["min"] > everything.min() and st[i]["max"] < everything.max() and st[i]["count"] == everything.size - 4
    i = cases.PLANTED.index("all_equal")
    assert st[i]["min"] == st[i]["max"] == 2.0 and st[i]["var"] == 0.0 and 0 < st[i]["count"] < everything.size
    assert V.sample_pairs(d, "global_min_max", f)[i] is None and V.sample_pairs(d, "standardize", f)[i] == (2.0, 1.0)
    assert V.sample_pairs(d, "robust_scale", f)[0] is None


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("per_baseline", [False, True])
def test_standardize_cap_holds_for_pairwise_sums_on_the_gpu_tests_inputs(kind, per_baseline):
    """The GPU test lets standardize outputs differ from the restatement by <= 1 float32 ulp in a share of at most
    normalize_ref.MAX_SHARE of the elements.  That cap is only meaningful if moments formed another way stay inside it on
    these very inputs: the restatement with np.mean / np.var in place of math.fsum does."""
    x, layout, f = cases.working(kind, per_baseline)
    bad = V.invalid_map(x, f, layout)
    exact = V.sample_pairs(x, "standardize", f, layout)
    other = []
    for i in range(len(x)):
        v = V.valid_scalars(x[i:i + 1], bad[i:i + 1], layout)
        other.append((float(np.mean(v)), float(np.sqrt(np.var(v)))))
    nref.check_outputs(V.transform(x, other, f, 0.0, layout), V.transform(x, exact, f, 0.0, layout), "standardize", f"{kind} np.mean / np.var")


# ---------------------------------------------------------------- the C ABI
def _header_prototypes():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "rfi_hip.h")).read()
    assert "validity-aware 8-channel input" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"\(\*(\w+)\)\[2\]", r"*\1", src)                  # const double (*params_host)[2] -> a pointer
    return {m.group(1): [a.strip() for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(rfi_(?:valid_[a-z_]+|model_predict_flags_valid))\s*\(([^)]*)\)\s*;", src)}


def test_symbols_resolve_with_declared_signatures():
    from rfi_toolbox_amd import _lib
    protos = _header_prototypes()
    assert set(protos) == set(ENTRIES)
    ctype_of = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double, "float": C.c_float}
    pointers = (C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_double),
                C.POINTER(_lib.NormStats), C.POINTER(_lib.Tiling))
    for name, args in protos.items():
        fn = getattr(_lib.lib, name)
        assert name in _lib.EXPORTED and fn.restype is C.c_int
        assert len(fn.argtypes) == len(args), (name, args)
        for decl, ct in zip(args, fn.argtypes):
            if "*" in decl:
                assert ct in pointers, (name, decl, ct)
            else:
                assert ct is ctype_of[decl.rsplit(" ", 1)[0].replace("const ", "").strip()], (name, decl, ct)
    assert (_lib.VALID_FLAGS_POL, _lib.VALID_FLAGS_BASELINE) == (0, 1)
    assert (_lib.VALID_SRC_COMPLEX, _lib.VALID_SRC_PLANAR, _lib.VALID_SRC_NHWC) == (0, 1, 2)


def test_entry_points_refuse_bad_arguments_without_a_device():
    from rfi_toolbox_amd._lib import lib
    assert lib.rfi_valid_map(None, None, 0, 0, 1, 16, None, 0, None, None, 0) != 0 and b"valid_map" in lib.rfi_last_error()
    assert lib.rfi_valid_apply(None, None, 0, 0, 1, 16, 0.0, 1.0, None, None, 0.0, None, 0) != 0
    assert lib.rfi_valid_statistics(None, None, None, None, None, None, 1, 2, 0, 1, None, 1) != 0
    assert lib.rfi_valid_gather(None, None, 0, 0, 1, 8, 8, None, 1, 8, 0.0, 1.0, None, None, 0, 0, 0.0, None, 0) != 0


# ---------------------------------------------------------------- Python argument checks (no device is touched)
def test_normalizer_flag_checks():
    from rfi_toolbox_amd.preprocessing import Normalizer, normalize_array
    x = np.zeros((2, 4, 8, 6), dtype=np.complex64)
    for bad in (np.zeros((2, 4, 8, 5), np.uint8), np.zeros((3, 8, 6), np.uint8), np.zeros((2, 8, 8, 6), np.uint8),
                np.zeros((8, 6), np.uint8)):
        with pytest.raises(ValueError, match="flags"):
            Normalizer("standardize", "sample").fit(x, flags=bad)
        with pytest.raises(ValueError, match="flags"):
            Normalizer("standardize", "dataset").statistics(x, flags=bad)
    with pytest.raises(TypeError, match="uint8 or bool"):
        Normalizer("standardize").fit(x, flags=np.zeros((2, 8, 6), np.float32))
    with pytest.raises(ValueError, match="nonfinite"):
        Normalizer("standardize").fit(x, flags="finite")
    with pytest.raises(ValueError, match="chunk"):
        Normalizer("standardize").fit([x, x], flags=[np.zeros((2, 8, 6), np.uint8)])
    with pytest.raises(ValueError, match="chunk"):
        Normalizer("standardize").fit([x, x], flags=np.zeros((2, 8, 6), np.uint8))
    nz = Normalizer("standardize").load_state_dict({"method": "standardize", "scope": "dataset", "centres": [0.0], "scales": [1.0]})
    with pytest.raises(ValueError, match="flags"):
        nz.transform(x, flags=np.zeros((2, 4, 6, 8), np.uint8))
    with pytest.raises(ValueError, match="flags"):
        normalize_array(np.zeros((8, 8, 6)), "standardize", flags=np.zeros((2, 8, 6), np.uint8))


def test_parameters_of_a_population_without_a_valid_scalar():
    from rfi_toolbox_amd.preprocessing.normalization import dataset_parameters, sample_parameters
    nan = float("nan")
    st = {"count": 0, "min": nan, "max": nan, "mean": nan, "var": nan, "q": ((nan, nan),) * 3}
    for method in nref.METHODS + (None,):
        assert sample_parameters(method, st) == (0.0, 0.0)
        assert dataset_parameters(method, st)[1] == (0.0, 0.0)


def test_inference_flag_checks():
    from rfi_toolbox_amd.inference import _prior_flags, tile_observation
    from rfi_toolbox_amd._lib import VALID_FLAGS_BASELINE, VALID_FLAGS_POL
    x = np.zeros((2, 4, 40, 52), dtype=np.complex64)
    assert _prior_flags(np.zeros(x.shape, bool), x.shape, 2, 40, 52)[0] == VALID_FLAGS_POL
    assert _prior_flags(np.zeros((2, 40, 52), np.uint8), x.shape, 2, 40, 52)[0] == VALID_FLAGS_BASELINE
    assert _prior_flags(np.zeros((40, 52), np.uint8), (4, 40, 52), 1, 40, 52)[0] == VALID_FLAGS_BASELINE
    assert _prior_flags("nonfinite", x.shape, 2, 40, 52) == (VALID_FLAGS_POL, None)
    for bad in (np.zeros((2, 4, 40, 51), np.uint8), np.zeros((40, 52), np.uint8), np.zeros((3, 40, 52), np.uint8)):
        with pytest.raises(ValueError, match="flags"):
            tile_observation(x, 32, flags=bad)
    with pytest.raises(TypeError, match="uint8 or bool"):
        tile_observation(x, 32, flags=np.zeros(x.shape, np.int32))
    with pytest.raises(ValueError, match="nonfinite"):
        tile_observation(x, 32, flags="all")


def test_flags_with_a_three_channel_model_raise():
    from rfi_toolbox_amd.inference import predict_flags
    from rfi_toolbox_amd.models import UNet
    model = object.__new__(UNet)                       # (no device: the check comes before anything touches one)
    model._h, model.in_channels, model.out_channels, model.targets = None, 3, 1, "map"
    x = np.zeros((2, 2, 40, 52), dtype=np.complex64)
    for flags in (np.zeros(x.shape, np.uint8), "nonfinite"):
        with pytest.raises(ValueError, match="8 input channels"):
            predict_flags(model, x, patch_size=32, flags=flags)
    model.in_channels = 8
    with pytest.raises(ValueError, match="flags must have the data's shape"):
        predict_flags(model, np.zeros((2, 4, 40, 52), np.complex64), patch_size=32, flags=np.zeros((2, 4, 40, 50), np.uint8))
