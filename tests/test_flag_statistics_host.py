"""CPU-only checks of the flagging-statistics fixtures and of the Python layer's argument errors (no device call).

The magnitude rule the device implements (csrc/flag_stats.hip, cabs_np) is written here in NumPy with an exact fma
and compared with the reference host's stored ``np.abs`` values."""
import importlib.util
import json
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _maker():
    spec = importlib.util.spec_from_file_location("make_statistics_golden",
                                                  os.path.join(GOLDEN, "make_statistics_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    keep, sys.dont_write_bytecode = sys.dont_write_bytecode, True      # no __pycache__ under tests/golden/
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.dont_write_bytecode = keep
    return mod


def _round_to(q, ft):
    """exact rational q -> nearest ft value (ties to even)"""
    f = ft(float(q))
    cands = [f, np.nextafter(f, ft(np.inf)), np.nextafter(f, ft(-np.inf))]
    best = min(cands, key=lambda c: (abs(Fraction(float(c)) - q), int(np.array(c).view(np.int64 if ft is np.float64 else np.int32)) & 1))
    return best


def magnitude_rule(z):
    """|z| = L * sqrt(fma(S/L, S/L, 1)) in the precision of z, fma exact"""
    ft = np.float32 if z.dtype == np.complex64 else np.float64
    out = np.empty(z.shape, ft)
    for k, v in enumerate(z.ravel()):
        a, b = abs(ft(v.real)), abs(ft(v.imag))
        if np.isinf(a) or np.isinf(b):
            out[k] = np.inf
        elif np.isnan(a) or np.isnan(b):
            out[k] = np.nan
        else:
            L, S = max(a, b), min(a, b)
            if L == 0:
                out[k] = 0
                continue
            r = ft(S / L)
            t = _round_to(Fraction(float(r)) ** 2 + 1, ft)
            out[k] = ft(L * ft(np.sqrt(t)))
    return out


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "statistics_expected.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def arrays():
    return np.load(os.path.join(GOLDEN, "statistics_inputs.npz"))


def test_fixture_loads(fixture, arrays):
    assert set(fixture["large"]) == {"waterfall_c64", "waterfall_c128", "real_f32", "real_f64"}
    assert len(fixture["small"]) >= 20
    for name, out in fixture["small"].items():
        assert f"small/{name}/data" in arrays.files, name
        assert {"stats_flags", "stats_all", "ffi", "cq"} <= set(out), name
    assert fixture["small"]["empty"]["stats_flags"]["count"] == 0
    assert fixture["small"]["constant"]["ffi"] == {"error": "ZeroDivisionError"}
    assert fixture["small"]["constant"]["cq"]["calcquality"] == np.inf


@pytest.mark.parametrize("name", ["waterfall_c64", "waterfall_c128", "real_f32", "real_f64"])
def test_large_inputs_match_their_sha256(fixture, name):
    mk = _maker()
    data, flags = mk.large_input(name)
    exp = fixture["large"][name]
    assert (data.size, str(data.dtype)) == (exp["size"], exp["dtype"])
    assert mk.sha256(data, flags) == exp["sha256"], "the large-case generator changed: regenerate the fixture"


@pytest.mark.parametrize("dt", ["complex64", "complex128"])
def test_magnitude_rule_matches_stored_np_abs(arrays, dt):
    z, want = arrays[f"crafted/{dt}/z"], arrays[f"crafted/{dt}/abs"]
    got = magnitude_rule(z)
    assert got.dtype == want.dtype
    assert np.array_equal(got, want, equal_nan=True), np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[:10]


@pytest.mark.parametrize("name", ["waterfall_c64", "waterfall_c128"])
def test_magnitude_rule_matches_large_case_sample(arrays, name):
    data, _ = _maker().large_input(name)
    idx = arrays[f"abs/{name}/index"][:2048]
    want = arrays[f"abs/{name}/abs"][:2048]
    assert np.array_equal(magnitude_rule(data.ravel()[idx]), want)


def test_argument_errors_raise_before_any_device_call(monkeypatch):
    from rfi_toolbox_amd.evaluation import statistics as st
    from rfi_toolbox_amd.evaluation import compute_ffi, flag_statistics

    def no_device(*a, **k):
        raise AssertionError("a device context was requested")
    monkeypatch.setattr(st.Context, "get", no_device)
    with pytest.raises(TypeError):
        flag_statistics(np.zeros(4, np.float16))
    with pytest.raises(TypeError):
        flag_statistics(np.array(["a", "b"]))
    with pytest.raises(TypeError):
        flag_statistics(np.zeros(4, np.float32), np.zeros(4, np.int32))
    with pytest.raises(ValueError):
        flag_statistics(np.zeros(4, np.complex64), np.zeros(5, bool))
    with pytest.raises(ValueError):
        compute_ffi(np.zeros((2, 3)), np.zeros((3, 3), bool))
    with pytest.raises(ValueError):
        st.compute_statistics(np.zeros(6, np.int16), np.zeros(2, np.uint8))


def test_reference_names_are_exported():
    import rfi_toolbox_amd.evaluation as ev
    from rfi_toolbox_amd.evaluation.statistics import compute_mad      # noqa: F401
    for n in ("compute_statistics", "compute_ffi", "compute_calcquality", "print_statistics_comparison",
              "flag_statistics", "evaluate_segmentation"):
        assert n in ev.__all__ and callable(getattr(ev, n))
