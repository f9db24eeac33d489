"""CPU-only: the library reads no environment variable beyond a short, documented list.

Experiment switches (A/B paths, tuning knobs, timing modes that skip work) do not belong in the shipped library: an A/B run
compares two builds through RFI_HIP_LIB instead (tools/ab.sh).  This test finds every environment read in the package's
C++/HIP and Python sources and checks the names against the list below."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rfi_toolbox_amd")

KEEP_NATIVE = {
    "RFI_NO_OVERLAP",           # context default of rfi_ctx_set_overlap (api.cpp)
    "RFI_SYNC_ALWAYS",          # documented in include/rfi_hip.h
    "RFI_NO_BUCKETS",           # bench.py's fallback attempt
    "RFI_NO_STOP_EVENTS",       # bench.py's fallback attempt
    "RFI_BUCKET_MIN_FLOATS",    # set by tests/test_gpu_comm.py
}
KEEP_PYTHON = {
    "RFI_HIP_LIB",              # _lib.py: the library to load (A/B runs of two builds)
    "RFI_RDZV_TIMEOUT",         # distributed.py
    "RFI_DIAG_STAMPS",          # build.py: diagnostic build, never shipped
}

NATIVE_READ = re.compile(r"\bgetenv\s*\(\s*\"(RFI_\w*)\"")
PY_READ = re.compile(r"\bos\.(?:environ\.get|getenv)\s*\(\s*[\"'](RFI_\w*)[\"']|\bos\.environ\s*\[\s*[\"'](RFI_\w*)[\"']\s*\]")


def _reads(exts, pattern):
    found = {}
    for d, _, files in os.walk(PKG):
        for f in files:
            if not f.endswith(exts):
                continue
            path = os.path.join(d, f)
            for m in pattern.finditer(open(path, encoding="utf-8").read()):
                name = next(g for g in m.groups() if g)
                found.setdefault(name, set()).add(os.path.relpath(path, ROOT))
    return found


def test_native_sources_read_only_the_kept_variables():
    found = _reads((".cpp", ".hpp", ".hip", ".h"), NATIVE_READ)
    assert "RFI_NO_OVERLAP" in found, "the scan found nothing: has the source layout changed?"
    extra = {k: sorted(v) for k, v in found.items() if k not in KEEP_NATIVE}
    assert not extra, f"environment switches outside the keep-list: {extra}"


def test_python_sources_read_only_the_kept_variables():
    found = _reads((".py",), PY_READ)
    assert "RFI_HIP_LIB" in found, "the scan found nothing: has the source layout changed?"
    extra = {k: sorted(v) for k, v in found.items() if k not in KEEP_PYTHON}
    assert not extra, f"environment switches outside the keep-list: {extra}"
