#!/usr/bin/env python3
"""Generate tests/golden/statistics_expected.json and statistics_inputs.npz by RUNNING THE REFERENCE's
``evaluation.statistics`` (compute_statistics, compute_mad, compute_ffi, compute_calcquality).

Run from the repository root on a host that has the reference package (preshanth/rfi_toolbox v0.2.0) on its
path; the GPU tests never import it:

    PYTHONDONTWRITEBYTECODE=1 CI=1 PYTHONPATH=<reference checkout> python tests/golden/make_statistics_golden.py

Small edge cases are stored verbatim (inputs in the .npz, outputs in the .json).  The large cases (up to 2^22
values) are NOT stored: ``large_input(name)`` below regenerates them from a seeded ``np.random.default_rng`` recipe,
and the fixture keeps each input's sha256 next to the reference outputs, so a changed generator fails loudly
instead of comparing the wrong data.  ``large_input`` needs NumPy only; the tests import it from this file.

The .npz also pins NumPy's complex ``np.abs`` of the generating host (the values the reference's statistics see):
a sample of the large complex inputs (indices + magnitudes) and crafted special values (stored verbatim).
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
JSON_PATH = os.path.join(HERE, "statistics_expected.json")
NPZ_PATH = os.path.join(HERE, "statistics_inputs.npz")

LARGE = ("waterfall_c64", "waterfall_c128", "real_f32", "real_f64")


def large_input(name):
    """-> (data, flags) of a large case, regenerated from its seed."""
    if name.startswith("waterfall"):
        c64 = name.endswith("c64")
        rng = np.random.default_rng(20261015 if c64 else 20261016)
        nchan, ntime = (1024, 4096) if c64 else (512, 4096)
        z = (rng.standard_normal((nchan, ntime)) + 1j * rng.standard_normal((nchan, ntime))) * np.sqrt(0.5)
        rows = rng.choice(nchan, nchan // 25, replace=False)          # narrow-band RFI (whole channels)
        cols = rng.choice(ntime, ntime // 60, replace=False)          # broadband bursts (whole time steps)
        z[rows, :] += (rng.uniform(5, 200, len(rows)) * np.exp(1j * rng.uniform(0, 2 * np.pi, len(rows))))[:, None]
        z[:, cols] += (rng.uniform(5, 50, len(cols)) * np.exp(1j * rng.uniform(0, 2 * np.pi, len(cols))))[None, :]
        flags = np.zeros((nchan, ntime), dtype=bool)
        flags[rows[: len(rows) * 4 // 5], :] = True                   # a flagger that finds most of it ...
        flags[:, cols[: len(cols) * 3 // 4]] = True
        flags |= rng.random((nchan, ntime)) < (0.03 if c64 else 0.12)  # ... plus false positives
        return z.astype(np.complex64 if c64 else np.complex128), flags
    f32 = name.endswith("f32")
    rng = np.random.default_rng(20261017 if f32 else 20261018)
    n = 1 << 22 if f32 else 1 << 21
    x = rng.standard_normal(n) * 2.5 - 0.75
    spikes = rng.choice(n, n // 100, replace=False)
    x[spikes] += rng.choice([-1.0, 1.0], len(spikes)) * rng.uniform(20, 400, len(spikes))
    flags = rng.random(n) < (0.22 if f32 else 0.05)
    flags[spikes[: len(spikes) // 2]] = True
    return x.astype(np.float32 if f32 else np.float64), flags


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def crafted_complex(dtype):
    """special and wide-exponent complex values (the magnitude rule's corners)"""
    ft = np.float32 if dtype == np.complex64 else np.float64
    fi = np.finfo(ft)
    sp = np.array([0.0, -0.0, fi.smallest_subnormal, fi.tiny, 1e-30, 0.5, 1.0, 3.0, 4.0, 7.0, fi.max / 2, fi.max,
                   np.inf, -np.inf, np.nan, -1.0, -3.0], dtype=ft)
    re, im = np.meshgrid(sp, sp)
    rng = np.random.default_rng(7 if dtype == np.complex64 else 8)
    lim = 120 if dtype == np.complex64 else 1000
    m = 2000
    r2 = (rng.uniform(0.5, 1.0, m) * 2.0 ** rng.integers(-lim, lim, m) * rng.choice([-1, 1], m)).astype(ft)
    i2 = (r2.astype(np.float64) * rng.uniform(0, 2, m) * 2.0 ** rng.integers(-30, 30, m)).astype(ft)
    z = np.concatenate([(re.ravel() + 1j * im.ravel()), (r2 + 1j * i2)]).astype(dtype)
    z.real[: re.size], z.imag[: re.size] = re.ravel(), im.ravel()        # keep -0.0 / NaN parts exactly
    return z


def small_cases():
    """name -> (data, flags or None, reference_data or None)"""
    rng = np.random.default_rng(99)
    f32, f64 = np.float32, np.float64
    c = {}
    c["empty"] = (np.zeros(0, f32), np.zeros(0, bool), None)
    c["all_flagged"] = (rng.standard_normal(16).astype(f32), np.ones(16, bool), None)
    c["none_flagged"] = (rng.standard_normal(17), np.zeros(17, bool), None)
    c["flags_none"] = (rng.standard_normal(10), None, None)
    c["single"] = (np.array([3.5], f32), np.array([False]), None)
    c["odd_f32"] = (rng.standard_normal(11).astype(f32) * 3, rng.random(11) < 0.2, None)
    c["even_f32"] = (rng.standard_normal(12).astype(f32) * 3, np.arange(12) % 3 == 0, None)
    c["even_f64"] = (rng.standard_normal((4, 6)) - 2, rng.random((4, 6)) < 0.25, None)
    x = rng.standard_normal(20)
    fl = np.arange(20) % 4 == 1
    xa = x.copy(); xa[5] = np.nan
    c["nan_flagged"] = (xa, fl, None)
    xb = x.copy(); xb[6] = np.nan
    c["nan_unflagged"] = (xb, fl, None)
    xc = x.astype(f32); xc[2] = np.inf; xc[7] = -np.inf
    c["inf_both_signs"] = (xc, fl, None)
    xd = x.copy(); xd[3] = np.inf
    c["pos_inf"] = (xd, fl, None)
    c["inf_minus_inf"] = (np.array([np.inf, np.inf, np.inf, 1.0, 2.0], f32), np.array([0, 0, 0, 0, 1], bool), None)
    z = (rng.standard_normal(12) + 1j * rng.standard_normal(12)).astype(np.complex64)
    z[0] = 0
    z[3] = complex(np.inf, np.nan)
    c["complex_special"] = (z, np.arange(12) % 5 == 2, None)
    z2 = (rng.standard_normal(9) + 1j * rng.standard_normal(9)).astype(np.complex128)
    z2[4] = complex(np.nan, 0.0)
    c["complex_nan_flagged"] = (z2, np.arange(9) == 4, None)
    c["complex_nan_unflagged"] = (z2, np.arange(9) == 5, None)
    c["int32"] = (rng.integers(-50, 50, 31).astype(np.int32), rng.random(31) < 0.3, None)
    c["int64_even"] = (rng.integers(0, 1000, 40), rng.random(40) < 0.5, None)
    c["bool"] = (rng.random(25) < 0.4, rng.random(25) < 0.3, None)
    c["constant"] = (np.full(64, 2.0, f32), np.arange(64) % 8 == 0, None)
    c["ref_other_size"] = (rng.standard_normal(50) * 2, rng.random(50) < 0.2, rng.standard_normal(80))
    c["ref_complex"] = ((rng.standard_normal(30) + 1j * rng.standard_normal(30)).astype(np.complex64),
                        rng.random(30) < 0.3, (rng.standard_normal(40) + 1j * rng.standard_normal(40)).astype(np.complex64))
    c["heavy_overflag"] = (rng.standard_normal(40).astype(f32), rng.random(40) < 0.85, None)
    return c


def _run(fn, *args):
    try:
        return _jsonable(fn(*args))
    except Exception as e:                       # noqa: BLE001  (the reference's own error is the expected output)
        return {"error": type(e).__name__}


def _jsonable(v):
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    return float(v)


def outputs(st, data, flags, ref):
    o = {"stats_flags": _run(st.compute_statistics, data, flags),
         "stats_all": _run(st.compute_statistics, data),
         "ffi": _run(st.compute_ffi, data, flags),
         "cq": _run(st.compute_calcquality, data, flags)}
    if ref is not None:
        o["cq_ref"] = _run(st.compute_calcquality, data, flags, ref)
    if not np.iscomplexobj(data):
        o["mad"] = _run(st.compute_mad, data)
    return o


def main():
    import warnings
    warnings.simplefilter("ignore")
    from rfi_toolbox.evaluation import statistics as st
    arrays, fixture = {}, {"numpy": np.__version__, "small": {}, "large": {}}
    for name, (data, flags, ref) in small_cases().items():
        arrays[f"small/{name}/data"] = data
        if flags is not None:
            arrays[f"small/{name}/flags"] = flags
        if ref is not None:
            arrays[f"small/{name}/ref"] = ref
        fixture["small"][name] = outputs(st, data, flags, ref)
    for name in LARGE:
        data, flags = large_input(name)
        half = data.ravel()[: data.size // 2] if name == "waterfall_c64" else None
        fixture["large"][name] = {"sha256": sha256(data, flags), "size": int(data.size), "dtype": str(data.dtype),
                                  **outputs(st, data, flags, half)}
        if np.iscomplexobj(data):
            idx = np.sort(np.random.default_rng(5).choice(data.size, 8192, replace=False)).astype(np.int64)
            arrays[f"abs/{name}/index"] = idx
            arrays[f"abs/{name}/abs"] = np.abs(data.ravel()[idx])
        print(name, fixture["large"][name]["ffi"], file=sys.stderr)
    for dt in (np.complex64, np.complex128):
        z = crafted_complex(dt)
        arrays[f"crafted/{np.dtype(dt).name}/z"] = z
        arrays[f"crafted/{np.dtype(dt).name}/abs"] = np.abs(z)
    np.savez_compressed(NPZ_PATH, **arrays)
    with open(JSON_PATH, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
    print(f"wrote {JSON_PATH} ({os.path.getsize(JSON_PATH)} B), {NPZ_PATH} ({os.path.getsize(NPZ_PATH)} B)")


if __name__ == "__main__":
    main()
