"""CPU-only checks of the one place that turns an array argument into what the C ABI takes (rfi_toolbox_amd/runtime.py:
describe, operand, as_pointer, result_buffer, ptr_mem) on NumPy and torch-CPU input: every `other` policy over layouts and
dtypes, against a NumPy expression of the rule.  No test here may reach a device context."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from rfi_toolbox_amd import runtime
from rfi_toolbox_amd._lib import DEVICE, HOST, VALUE_CODES
from rfi_toolbox_amd.runtime import as_pointer, describe, operand

DTYPES = (np.bool_, np.uint8, np.int32, np.float16, np.float32, np.float64, np.complex64, np.complex128)
LAYOUTS = ("c", "fortran", "sliced", "empty", "0d")
KINDS = ("numpy", "torch")
U8, F32, F64 = np.dtype(np.uint8), np.dtype(np.float32), np.dtype(np.float64)


class _NoContext:
    """Stands in for the context: host input must not look at it."""

    def __getattr__(self, name):
        raise AssertionError(f"the context was dereferenced ({name})")


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    def no_context(cls, device=None):
        raise AssertionError("a device context was requested")
    monkeypatch.setattr(runtime.Context, "get", classmethod(no_context))


def _array(dtype, layout):
    base = (np.arange(24).reshape(4, 6) % 5) - 1                    # -1 .. 3: zeros, a negative value, values > 1
    dt = np.dtype(dtype)
    if dt.kind == "c":
        a = (base + 1j * base[::-1]).astype(dt)
    elif dt.kind == "f":
        a = (base * 0.75).astype(dt)
    elif dt == np.bool_:
        a = base > 0
    else:
        a = base.astype(dt)                                           # (uint8: -1 wraps to 255)
    return {"c": a, "fortran": np.asfortranarray(a), "sliced": a[:, ::2], "empty": a[:0], "0d": np.array(a[1, 3])}[layout]


def _as_kind(a, kind):
    return a if kind == "numpy" else torch.from_numpy(a)


def _behind(o):
    """What lies behind the operand's pointer, as an array of its dtype and shape."""
    raw = C.string_at(o.ptr, o.size * o.dtype.itemsize) if o.size else b""
    return np.frombuffer(raw, o.dtype).reshape(o.shape)


def _bytes(x):
    return np.ascontiguousarray(x).reshape(-1).view(np.uint8)


def _check(o, a, want):
    """The operand of `a` holds `want` (a NumPy expression of the rule), bit for bit, with the input's shape and size."""
    assert o.mem == HOST and o.shape == a.shape and o.size == a.size and o.dtype == want.dtype
    assert isinstance(o.keep, np.ndarray) and o.keep.flags.c_contiguous and o.keep.dtype == want.dtype
    assert o.ptr == o.keep.ctypes.data
    assert np.array_equal(_bytes(o.keep), _bytes(want)) and np.array_equal(_bytes(_behind(o)), _bytes(want))


def _quiet(fn):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                               # (complex -> real casts warn, in NumPy and in torch)
        return fn()


CASES = [(k, d, lay) for k in KINDS for d in DTYPES for lay in LAYOUTS]


@pytest.mark.parametrize("kind,dtype,layout", CASES)
def test_describe_is_pure(kind, dtype, layout):
    a = _array(dtype, layout)
    x = _as_kind(a, kind)
    before = a.copy()
    shape, dt, gpu, owner = describe(x)
    assert shape == a.shape and all(type(s) is int for s in shape)
    assert dt == a.dtype and isinstance(dt, np.dtype) and gpu is None and owner is None
    assert np.array_equal(a, before)


def test_describe_of_lists_scalars_and_torch_only_dtypes():
    assert describe([[1, 2, 3], [4, 5, 6]])[:2] == ((2, 3), np.dtype(np.int64))
    assert describe(2.5) == ((), F64, None, None)
    assert describe(torch.zeros(3, 2, dtype=torch.bfloat16)) == ((3, 2), None, None, None)
    assert describe(torch.zeros(2, requires_grad=True))[:2] == ((2,), F32)


@pytest.mark.parametrize("kind,dtype,layout", CASES)
def test_cast_is_what_as_pointer_did(kind, dtype, layout):
    a = _array(dtype, layout)
    for target in (F32, U8):
        want = _quiet(lambda: np.ascontiguousarray(a, dtype=target))
        if a.dtype == np.bool_ and target == U8:
            want = a.view(np.uint8)                                   # bool as its bytes: no value changes
        _check(_quiet(lambda: operand(_as_kind(a, kind), _NoContext(), (target,), "cast")), a, want)
        ptr, mem, keep = _quiet(lambda: as_pointer(_as_kind(a, kind), target, _NoContext()))
        assert mem == HOST and ptr == keep.ctypes.data and np.array_equal(_bytes(keep), _bytes(want))


@pytest.mark.parametrize("kind", KINDS)
def test_as_pointer_copies_nothing_it_need_not(kind):
    a = _array(np.float32, "c")
    ptr, mem, keep = as_pointer(_as_kind(a, kind), np.float32, _NoContext())
    assert ptr == a.ctypes.data and mem == HOST and np.shares_memory(keep, a)
    b = _array(np.bool_, "c")
    ptr, mem, keep = as_pointer(_as_kind(b, kind), np.uint8, _NoContext())
    assert ptr == b.ctypes.data and keep.dtype == np.uint8


@pytest.mark.parametrize("kind,dtype,layout", CASES)
def test_nonzero(kind, dtype, layout):
    a = _array(dtype, layout)
    want = a if a.dtype in (U8, F32) else (a.view(np.uint8) if a.dtype == np.bool_ else (a != 0).astype(np.uint8))
    o = operand(_as_kind(a, kind), _NoContext(), (np.uint8, np.float32), "nonzero")
    _check(o, a, want)
    assert set(np.unique(o.keep)) <= {0, 1} or a.dtype in (U8, F32)


@pytest.mark.parametrize("kind,dtype,layout", CASES)
def test_widen(kind, dtype, layout):
    a = _array(dtype, layout)

    def refuse(dt):
        return TypeError(f"data must be real or complex, not {dt}")
    if a.dtype == np.float16:
        with pytest.raises(TypeError, match="not float16"):
            operand(_as_kind(a, kind), _NoContext(), tuple(VALUE_CODES), "widen", error=refuse)
        return
    want = a.astype(np.float64) if a.dtype.kind in "biu" else a
    _check(operand(_as_kind(a, kind), _NoContext(), tuple(VALUE_CODES), "widen", error=refuse), a, want)


@pytest.mark.parametrize("kind,dtype,layout", CASES)
def test_reject_raises_the_callers_class(kind, dtype, layout):
    a = _array(dtype, layout)
    if a.dtype in (np.bool_, U8):
        _check(operand(_as_kind(a, kind), _NoContext(), (np.uint8,)), a, a.view(np.uint8))
        return
    for cls in (TypeError, ValueError):
        with pytest.raises(cls, match=f"flags must be bool or uint8, not {a.dtype}"):
            operand(_as_kind(a, kind), _NoContext(), (np.uint8,), "reject", error=lambda dt: cls(f"flags must be bool or uint8, not {dt}"))
    with pytest.raises(TypeError):                                    # without a caller's error: TypeError
        operand(_as_kind(a, kind), _NoContext(), (np.uint8,))


def test_torch_dtypes_numpy_lacks():
    t = torch.arange(6, dtype=torch.float32).reshape(2, 3).to(torch.bfloat16)
    o = operand(t, _NoContext(), (np.float32,), "cast")
    _check(o, np.empty((2, 3)), np.arange(6, dtype=np.float32).reshape(2, 3))
    with pytest.raises(ValueError, match="bfloat16|None"):
        operand(t, _NoContext(), tuple(VALUE_CODES), "widen", error=lambda dt: ValueError(f"not {dt}"))
    g = torch.ones(4, requires_grad=True)                             # detached on the way
    _check(operand(g, _NoContext(), (np.float32,)), np.empty(4), np.ones(4, np.float32))


def test_to_device_uploads_the_converted_contiguous_array():
    class Uploaded:
        ptr = 0xABC0

    class Ctx:
        def to_device(self, arr):
            assert arr.flags.c_contiguous
            self.got = arr.copy()
            return Uploaded()
    a = _array(np.int32, "sliced")
    ctx = Ctx()
    o = operand(a, ctx, (np.uint8, np.float32), "nonzero", to_device=True)
    assert (o.ptr, o.mem, o.dtype, o.shape, o.size) == (0xABC0, DEVICE, U8, a.shape, a.size) and isinstance(o.keep, Uploaded)
    assert ctx.got.dtype == np.uint8 and np.array_equal(ctx.got, (a != 0).astype(np.uint8))


def test_context_for_asks_for_the_cached_context_only_for_host_input():
    with pytest.raises(AssertionError, match="context was requested"):
        runtime.context_for(None, np.zeros(3), torch.zeros(3))


def test_out_check_and_pointer_helpers():
    runtime.check_out("host")
    runtime.check_out("device")
    for bad in ("gpu", None, 0):
        with pytest.raises(ValueError, match="out must be 'host' or 'device'"):
            runtime.check_out(bad)
    assert runtime.ptr_mem(None) == (None, HOST) and runtime.P(None) is None
    a = np.zeros(4, np.float32)
    p, mem = runtime.ptr_mem(a)
    assert p.value == a.ctypes.data and mem == HOST
    res, ptr, mem = runtime.result_buffer(_NoContext(), (2, 3), np.uint8, "host", a)
    assert isinstance(res, np.ndarray) and res.shape == (2, 3) and res.dtype == np.uint8 and ptr == res.ctypes.data and mem == HOST
