"""Flagging-quality statistics on the device against the reference's outputs (tests/golden/make_statistics_golden.py).

Exact: median, MAD, max, counts, flagged fractions and every NaN / inf / edge-case dict.  Bounded: mean and std
(relative), and the differences of close numbers (std_reduction, ffi, calcquality and its components): absolute up
to magnitude 1 and relative beyond it, since e.g. sdiff = fstd - rstd ~ -12 inherits the reference's own float32 std
error (NumPy's pairwise float32 sums are off by ~5e-7 relative; the device's fp64 sums are checked against an fp64
computation separately)."""
import importlib.util
import json
import math
import os
import sys
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL = {True: 2e-6, False: 1e-12}            # mean / std, keyed by float32 origin
ABS = {True: 4e-6, False: 1e-11}            # std_reduction, ffi, calcquality components
WORST = {}


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


with open(os.path.join(GOLDEN, "statistics_expected.json")) as _f:
    FIX = json.load(_f)
ARR = np.load(os.path.join(GOLDEN, "statistics_inputs.npz"))


def _same(a, b):
    """equal, NaN equal to NaN"""
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def _check(tag, got, want, exact, rel=(), absol=(), f32=False):
    assert set(got) == set(want), (tag, set(got) ^ set(want))
    for k, w in want.items():
        g = got[k]
        if isinstance(w, dict):
            _check(f"{tag}.{k}", g, w, exact, rel, absol, f32)
            continue
        if k in exact or not math.isfinite(w) or not math.isfinite(g):
            assert _same(g, w), (tag, k, g, w)
        elif k in rel:
            e = abs(g - w) / max(abs(w), 1e-300)
            WORST[(f32, "rel", k)] = max(WORST.get((f32, "rel", k), 0.0), e)
            assert e <= REL[f32], (tag, k, g, w, e)
        else:
            assert k in absol, (tag, k)
            e = abs(g - w) / max(1.0, abs(w))
            WORST[(f32, "abs", k)] = max(WORST.get((f32, "abs", k), 0.0), e)
            assert e <= ABS[f32], (tag, k, g, w, e)


STATS = dict(exact={"median", "mad", "count", "flagged_fraction"}, rel={"mean", "std"})
FFI = dict(exact={"mad_reduction", "flagged_fraction"}, absol={"std_reduction", "ffi"})
CQ = dict(exact={"flagged_pct", "rmax", "overflagging_penalty"}, rel={"rmean", "rstd", "fmean", "fstd"},
          absol={"calcquality", "sensitivity", "mean_shift", "std_shift", "maxdev", "fdiff", "sdiff"})


def _call(fn, *args):
    try:
        return fn(*args)
    except Exception as e:          # noqa: BLE001
        return {"error": type(e).__name__}


def _compare(tag, data, flags, ref, want):
    from rfi_toolbox_amd.evaluation import statistics as st
    f32 = np.asarray(data).dtype in (np.float32, np.complex64)
    got = {"stats_flags": _call(st.compute_statistics, data, flags), "stats_all": _call(st.compute_statistics, data),
           "ffi": _call(st.compute_ffi, data, flags), "cq": _call(st.compute_calcquality, data, flags)}
    if "cq_ref" in want:
        got["cq_ref"] = _call(st.compute_calcquality, data, flags, ref)
    if "mad" in want:
        got["mad"] = _call(lambda d: float(st.compute_mad(d)), data)
    for k, w in want.items():
        if isinstance(w, dict) and "error" in w:
            assert got[k] == w, (tag, k, got[k])
        elif k == "mad":
            assert _same(got[k], w), (tag, k, got[k], w)
        else:
            rules = STATS if k.startswith("stats") else (FFI if k == "ffi" else CQ)
            _check(f"{tag}.{k}", got[k], w, f32=f32, **rules)
    return got


@pytest.mark.parametrize("name", sorted(FIX["small"]))
def test_small_cases_match_reference(name):
    data = ARR[f"small/{name}/data"]
    flags = ARR[f"small/{name}/flags"] if f"small/{name}/flags" in ARR.files else None
    ref = ARR[f"small/{name}/ref"] if f"small/{name}/ref" in ARR.files else None
    _compare(name, data, flags, ref, FIX["small"][name])


@pytest.mark.parametrize("name", ["waterfall_c64", "waterfall_c128", "real_f32", "real_f64"])
def test_large_cases_match_reference(name):
    WORST.clear()
    mk = _maker()
    data, flags = mk.large_input(name)
    want = FIX["large"][name]
    assert mk.sha256(data, flags) == want["sha256"]
    ref = data.ravel()[: data.size // 2] if "cq_ref" in want else None
    _compare(name, data, flags, ref, {k: v for k, v in want.items() if k not in ("sha256", "size", "dtype")})
    if data.dtype in (np.float32, np.complex64):      # float32 origin: mean / std within float32 rounding of fp64
        a = (np.abs(data) if np.iscomplexobj(data) else data).astype(np.float64).ravel()
        from rfi_toolbox_amd.evaluation import flag_statistics
        got = flag_statistics(data, flags)
        for s, v in zip(got, (a, a[~flags.ravel()])):
            for k, want_ in (("mean", v.mean()), ("std", v.std())):
                e = abs(getattr(s, k) - want_) / want_
                WORST[(True, "vs fp64", k)] = max(WORST.get((True, "vs fp64", k), 0.0), e)
                assert e <= 1.2e-7, (k, e)
    print(f"\n{name}: worst deviations " + ", ".join(f"{k[1]} {k[2]} ({'f32' if k[0] else 'f64'}) {v:.2e}"
                                                    for k, v in sorted(WORST.items())))


def _bits(fs):
    return tuple(struct.pack("<d", v) if isinstance(v, float) else v for v in fs)


@pytest.mark.parametrize("name", ["waterfall_c64", "real_f64"])
def test_no_flags_is_bit_identical_to_all(name):
    from rfi_toolbox_amd.evaluation import compute_calcquality, compute_ffi, flag_statistics
    data, _ = _maker().large_input(name)
    for flags in (None, np.zeros(data.shape, bool)):
        a, c = flag_statistics(data, flags)
        assert _bits(a) == _bits(c)
        cq = compute_calcquality(data, flags)
        assert cq["mean_shift"] == -1.0 and cq["std_shift"] == 0.0
        ffi = compute_ffi(data, flags)
        assert ffi["mad_reduction"] == 0.0 and ffi["std_reduction"] == 0.0 and ffi["ffi"] == 0.0


@pytest.mark.parametrize("name", ["waterfall_c64", "waterfall_c128", "real_f32"])
def test_reproducible(name):
    from rfi_toolbox_amd.evaluation import flag_statistics
    data, flags = _maker().large_input(name)
    r1 = [_bits(s) for s in flag_statistics(data, flags)]
    r2 = [_bits(s) for s in flag_statistics(data, flags)]
    assert r1 == r2


@pytest.mark.parametrize("name", ["waterfall_c64", "real_f64"])
def test_input_forms_agree(name):
    from rfi_toolbox_amd.evaluation import flag_statistics
    from rfi_toolbox_amd.runtime import Context, DeviceArray
    data, flags = _maker().large_input(name)
    want = [_bits(s) for s in flag_statistics(data, flags)]
    dt, ft = torch.from_numpy(data), torch.from_numpy(flags)
    assert [_bits(s) for s in flag_statistics(dt, ft)] == want
    assert [_bits(s) for s in flag_statistics(dt.cuda(), ft.cuda())] == want
    assert [_bits(s) for s in flag_statistics(dt, flags.astype(np.uint8) * 3)] == want      # uint8: non-zero == flagged
    ctx = Context.get(0)
    dd, df = DeviceArray(ctx, data.shape, data.dtype), DeviceArray(ctx, flags.shape, np.uint8)
    dd.copy_from(data)
    df.copy_from(flags.astype(np.uint8))
    assert [_bits(s) for s in flag_statistics(dd, df)] == want


def test_integer_input_is_widened():
    from rfi_toolbox_amd.evaluation import flag_statistics
    x = np.random.default_rng(3).integers(-1000, 1000, 100_001)
    f = np.arange(x.size) % 3 == 0
    want = [_bits(s) for s in flag_statistics(x.astype(np.float64), f)]
    assert [_bits(s) for s in flag_statistics(x, f)] == want
    assert [_bits(s) for s in flag_statistics(torch.from_numpy(x).cuda(), torch.from_numpy(f).cuda())] == want


@pytest.mark.parametrize("dt", ["complex64", "complex128"])
def test_device_magnitudes_match_stored_np_abs(dt):
    """max of a one-element array is its |z|: the device rule against NumPy on special and wide-exponent values"""
    from rfi_toolbox_amd.evaluation import flag_statistics
    z, want = ARR[f"crafted/{dt}/z"], ARR[f"crafted/{dt}/abs"]
    pick = np.r_[0:289, 289:z.size:7]
    bad = []
    for i in pick:
        got = flag_statistics(z[i:i + 1], medians=False)[0].max
        if not _same(got, float(want[i])):
            bad.append((z[i], got, float(want[i])))
    assert not bad, bad[:5]
    # the medians see the same values: a whole-array check of the sample
    a = flag_statistics(z[289:])[0]
    assert a.median == float(np.median(want[289:]))


def _closed_form_view(n, clean):
    """counts of x = i mod 1021 over i < n (clean: i mod 7 != 0)"""
    v = np.arange(1021)
    cnt = (n - 1 - v) // 1021 + 1
    if clean:
        c = np.array([next(u + 1021 * k for k in range(7) if (u + 1021 * k) % 7 == 0) for u in v])
        cnt = cnt - np.where(c < n, (n - 1 - c) // 7147 + 1, 0)
    return v, cnt


def _select(vals, cnt, r):
    order = np.argsort(vals, kind="stable")
    cs = np.cumsum(cnt[order])
    return vals[order][np.searchsorted(cs, r, side="right")]


def _median32(vals, cnt):
    N = int(cnt.sum())
    a, b = _select(vals, cnt, (N - 1) // 2), _select(vals, cnt, N // 2)
    return float(np.float32((np.float32(a) + np.float32(b)) / np.float32(2)))


def test_device_resident_beyond_2_31_elements():
    from rfi_toolbox_amd.evaluation import flag_statistics
    n = (1 << 31) + (1 << 20)
    x = torch.empty(n, dtype=torch.float32, device="cuda")
    f = torch.empty(n, dtype=torch.bool, device="cuda")
    step = 1 << 27
    for s in range(0, n, step):
        i = torch.arange(s, min(s + step, n), dtype=torch.int64, device="cuda")
        x[s:s + i.numel()] = (i % 1021).to(torch.float32)
        f[s:s + i.numel()] = i % 7 == 0
        del i
    try:
        a, c = flag_statistics(x, f)
    finally:
        del x, f
        torch.cuda.empty_cache()
    for s, clean in ((a, False), (c, True)):
        v, cnt = _closed_form_view(n, clean)
        N = int(cnt.sum())
        assert s.count == N and s.flagged == n - int(_closed_form_view(n, True)[1].sum()) and s.size == n
        assert s.max == 1020.0
        med = _median32(v.astype(np.float64), cnt)
        assert s.median == med, (clean, s.median, med)
        d = np.abs(v.astype(np.float32) - np.float32(med)).astype(np.float64)
        assert s.mad == _median32(d, cnt), (clean, s.mad)
        mean = float(sum(int(a_) * int(b_) for a_, b_ in zip(v, cnt))) / N
        var = float(sum(int(b_) * (float(a_) - mean) ** 2 for a_, b_ in zip(v, cnt))) / N
        assert abs(s.mean - mean) / mean <= REL[True] and abs(s.std - math.sqrt(var)) / math.sqrt(var) <= REL[True]
