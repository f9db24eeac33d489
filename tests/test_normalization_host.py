"""CPU-only: the NumPy restatement of the normalisation (tests/normalize_ref.py) against fixtures captured from the
reference and scikit-learn 1.7.2 (tests/golden/make_normalization_golden.py); the new C-ABI symbols; and the argument
checks of Normalizer / normalize_array / RFIMaskDataset, which must raise before any GPU context exists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import normalize_ref as R


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = {"inputs": np.load(os.path.join(golden_dir, "normalization_inputs.npz")),
         "expected": np.load(os.path.join(golden_dir, "normalization_expected.npz"))}
    for m in R.METHODS:
        g["dataset_" + m] = np.load(os.path.join(golden_dir, f"normalization_expected_dataset_{m}.npz"))
        g["sample_" + m] = np.load(os.path.join(golden_dir, f"normalization_expected_sample_{m}.npz"))
    return g


@pytest.mark.parametrize("method", R.METHODS)
def test_restatement_dataset_scope_matches_reference(golden, method):
    x = golden["inputs"]["inputs"]
    attrs, (out,) = R.normalize_dataset([x], method)
    R.check_attrs(attrs, R.golden_attrs(golden["expected"], "four.", method), method, "four")
    R.check_outputs(out, golden["dataset_" + method]["items"], method, "dataset scope")
    # split into chunks of mixed layout: the same parameters
    attrs2, _ = R.normalize_dataset([x[:1], x[1:].transpose(0, 2, 3, 1)], method)
    assert attrs2 == attrs


@pytest.mark.parametrize("method", R.METHODS)
def test_restatement_sample_scope_matches_normalize_array(golden, method):
    gi = golden["inputs"]
    six = np.concatenate([gi["inputs"], gi["constant"][None], gi["two_valued"][None]])
    R.check_outputs(R.normalize_samples(six, method), golden["sample_" + method]["outputs"], method, "sample scope")


@pytest.mark.parametrize("name", ["constant", "two_valued"])
@pytest.mark.parametrize("method", R.METHODS)
def test_restatement_degenerate_datasets(golden, name, method):
    x = golden["inputs"][name][None]
    attrs, (out,) = R.normalize_dataset([x], method)
    R.check_attrs(attrs, R.golden_attrs(golden["expected"], name + ".", method), method, name)
    R.check_outputs(out, golden["expected"][f"{name}.{method}.items"], method, name)
    if name == "constant":
        assert not out.any()                         # min-max: zeros; the others: (0.5 - 0.5) / 1e-8


def test_degenerate_sample_rules(golden):
    gi = golden["inputs"]
    assert R.sample_params(gi["constant"], "standardize") == (0.5, 1.0)
    assert R.sample_params(gi["constant"], "robust_scale") == (0.5, 1.0)
    assert R.sample_params(gi["constant"], "global_min_max") is None
    assert R.sample_params(gi["two_valued"], "robust_scale") == (1.0, 1.0)     # q25 == q75: the scale becomes 1


def _header_prototypes():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "rfi_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): [a.strip() for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(rfi_norm_[a-z_]+)\s*\(([^)]*)\)\s*;", src)}


def test_symbols_resolve_with_declared_signatures():
    from rfi_toolbox_amd import _lib
    protos = _header_prototypes()
    assert set(protos) == {"rfi_norm_bracket", "rfi_norm_statistics", "rfi_norm_apply"}
    ctype_of = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}
    for name, args in protos.items():
        fn = getattr(_lib.lib, name)
        assert name in _lib.EXPORTED and fn.restype is C.c_int
        assert len(fn.argtypes) == len(args), (name, args)
        for decl, ct in zip(args, fn.argtypes):
            base = decl.rsplit(" ", 1)[0].replace("const ", "").strip()
            if "*" in decl:
                assert ct in (C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                              C.POINTER(_lib.NormStats)), (name, decl, ct)
            else:
                assert ct is ctype_of[base], (name, decl, ct)
    assert C.sizeof(_lib.NormStats) == 2 * 8 + 4 * 8 + 6 * 8
    assert _lib.lib.rfi_abi_version() == 1


@pytest.mark.parametrize("count", [1, 2, 3, 4, 5, 8, 4097, 8 * 64 * 64, 8 * 96 * 80 * 6, 8 * 1024 * 1024 * 16 + 3])
def test_bracket_ranks_follow_numpy_linear_method(count):
    """rfi_norm_bracket (host only) against NumPy's virtual index (n - 1) q, and through it np.percentile itself."""
    from rfi_toolbox_amd.preprocessing.normalization import _lerp, bracket
    for q in (0.5, 0.25, 0.75):
        lo, hi, t = bracket(count, q)
        v = (count - 1) * q
        assert (lo, hi, t) == (int(np.floor(v)), min(int(np.floor(v)) + 1, count - 1), v - np.floor(v))
    if count <= 8 * 96 * 80 * 6:
        x = np.sort(np.random.RandomState(count).standard_normal(count) * 100.0)
        for q in (0.25, 0.75):
            lo, hi, t = bracket(count, q)
            assert _lerp(float(x[lo]), float(x[hi]), t) == float(np.percentile(x, 100 * q))


def test_parameters_from_statistics_match_restatement(golden):
    """the host half of the device path (brackets -> quantiles -> parameters) fed with exact statistics"""
    from rfi_toolbox_amd.preprocessing.normalization import bracket, dataset_parameters, sample_parameters
    for x in (golden["inputs"]["inputs"], golden["inputs"]["two_valued"][None], golden["inputs"]["constant"][None]):
        v = np.sort(x.ravel())
        mean, var = R.moments(v)
        st = {"count": v.size, "min": float(v[0]), "max": float(v[-1]), "mean": mean, "var": var,
              "q": tuple((float(v[bracket(v.size, q)[0]]), float(v[bracket(v.size, q)[1]])) for q in (0.5, 0.25, 0.75))}
        for m in R.METHODS:
            attrs, pair = dataset_parameters(m, st)
            want_attrs, want_pair = R.dataset_params([x], m)
            assert attrs == want_attrs and pair == (want_pair if want_pair is not None else (0.0, 0.0))
            want = R.sample_params(v, m)
            assert sample_parameters(m, st) == (want if want is not None else (0.0, 0.0))


def test_argument_errors_before_any_context(monkeypatch, tmp_path):
    from rfi_toolbox_amd import runtime
    from rfi_toolbox_amd.datasets import RFIMaskDataset
    from rfi_toolbox_amd.preprocessing import Normalizer, normalize_array

    def no_context(*a, **k):
        raise AssertionError("a device context was created before the arguments were checked")
    monkeypatch.setattr(runtime.Context, "__init__", no_context)
    monkeypatch.setattr(runtime.Context, "get", classmethod(no_context))
    with pytest.raises(ValueError, match="Unsupported normalization method"):
        Normalizer("z_score")
    with pytest.raises(ValueError, match="Unsupported normalization method"):
        normalize_array(np.zeros((8, 4, 4)), method="z_score")
    with pytest.raises(ValueError, match="scope"):
        Normalizer("standardize", scope="batch")
    with pytest.raises(ValueError, match="8 channels"):
        Normalizer("standardize").fit(np.zeros((2, 3, 16, 16)))
    with pytest.raises(ValueError, match=r"\(n, 4, T, F\)"):
        Normalizer("standardize").fit(np.zeros((2, 8, 16, 16), dtype=np.complex128))
    with pytest.raises(ValueError, match="ambiguous"):
        Normalizer("standardize").fit(np.zeros((2, 8, 16, 8)))
    with pytest.raises(TypeError):
        Normalizer("standardize").fit(np.zeros((2, 8, 16, 16), dtype=np.int32))
    with pytest.raises(ValueError, match="same precision"):
        Normalizer("standardize").fit([np.zeros((1, 8, 16, 16)), np.zeros((1, 8, 16, 16), dtype=np.float32)])
    with pytest.raises(ValueError, match="one array"):
        Normalizer("standardize", scope="sample").fit([np.zeros((1, 8, 16, 16))] * 2)
    with pytest.raises(ValueError, match=r"\(8, T, F\)"):
        normalize_array(np.zeros((4, 16, 16)))
    with pytest.raises(RuntimeError, match="before fit"):
        Normalizer("standardize").transform(np.zeros((1, 8, 16, 16)))
    with pytest.raises(ValueError, match="out must be"):
        Normalizer("standardize").transform(np.zeros((1, 8, 16, 16)), out="hwc")
    with pytest.raises(ImportError, match="CASA is required for use_ms=True"):
        RFIMaskDataset(str(tmp_path), use_ms=True, ms_name="x.ms")
    with pytest.raises(ValueError, match="ms_name must be provided"):
        RFIMaskDataset(str(tmp_path), use_ms=True)
    with pytest.raises(ValueError, match="Unsupported normalization method"):
        RFIMaskDataset(str(tmp_path), normalization="z_score")
    with pytest.raises(ValueError, match="no sample directories"):
        RFIMaskDataset(str(tmp_path))


def test_state_dict_round_trip_is_plain_python():
    from rfi_toolbox_amd.preprocessing import Normalizer
    a = Normalizer("robust_scale")
    a.global_min, a.global_max, a.mean, a.std, a.robust_median, a.robust_iqr = -1.0, 2.0, 0.25, 1.5, 0.125, 0.75
    a.centres, a.scales = [0.125], [0.75]
    sd = a.state_dict()
    assert all(v is None or isinstance(v, (str, float, list)) for v in sd.values())
    b = Normalizer(None).load_state_dict(sd)
    assert b.state_dict() == sd and b.method == "robust_scale" and b.scope == "dataset"
