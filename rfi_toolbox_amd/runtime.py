"""Thin host runtime over the C ABI: one Context per GPU (one HIP stream), device buffers,
and array plumbing between NumPy / torch and raw pointers.  No compute happens in Python."""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import DEVICE, HOST, check, lib

try:                                    # torch is plumbing only (tensor I/O, init RNG, distributed)
    import torch
except Exception:                       # pragma: no cover
    torch = None


def _parse_device(device) -> int:
    if device is None:
        return int(os.environ.get("LOCAL_RANK", "0"))
    if isinstance(device, int):
        return device
    s = str(device)
    if s == "cpu":
        raise RuntimeError("rfi_toolbox_amd runs on MI355X GPUs only; there is no CPU path "
                           "(use the reference rfi_toolbox for CPU execution)")
    if s in ("cuda", "hip", "gpu"):
        return int(os.environ.get("LOCAL_RANK", "0"))
    if ":" in s:
        return int(s.split(":")[1])
    raise ValueError(f"unknown device {device!r}")


class Context:
    """Owns a rfi_ctx (GPU + HIP stream).  Not thread-safe: one host thread per context."""

    _cache: dict = {}
    _lock = threading.Lock()

    def __init__(self, device=None):
        self.device_index = _parse_device(device)
        h = C.c_void_p()
        check(lib.rfi_ctx_create(self.device_index, C.byref(h)))
        self.handle = h
        self._comm = False

    @classmethod
    def get(cls, device=None) -> "Context":
        idx = _parse_device(device)
        with cls._lock:
            ctx = cls._cache.get((os.getpid(), idx))
            if ctx is None:
                ctx = cls(idx)
                cls._cache[(os.getpid(), idx)] = ctx
            return ctx

    # ---- memory
    def malloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        check(lib.rfi_malloc(self.handle, max(int(nbytes), 16), C.byref(p)))
        return p.value

    def free(self, ptr: int):
        check(lib.rfi_free(self.handle, C.c_void_p(ptr)))

    def synchronize(self):
        check(lib.rfi_ctx_synchronize(self.handle))

    def set_overlap(self, on: bool):
        """Backward-pass overlap of the weight-gradient kernels (side stream); default on."""
        check(lib.rfi_ctx_set_overlap(self.handle, 1 if on else 0))

    def stream_ptr(self) -> int:
        s = C.c_void_p()
        check(lib.rfi_ctx_stream(self.handle, C.byref(s)))
        return s.value or 0

    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        check(lib.rfi_ctx_device_name(self.handle, buf, 256))
        return buf.value.decode()

    def to_device(self, arr: np.ndarray) -> "DeviceArray":
        arr = np.ascontiguousarray(arr)
        d = DeviceArray(self, arr.shape, arr.dtype)
        check(lib.rfi_memcpy(self.handle, C.c_void_p(d.ptr), DEVICE, arr.ctypes.data_as(C.c_void_p), HOST,
                             arr.nbytes))
        return d

    def empty(self, shape, dtype=np.float32) -> "DeviceArray":
        return DeviceArray(self, shape, np.dtype(dtype))

    # ---- timing / profile
    def timer_start(self):
        check(lib.rfi_timer_start(self.handle))

    def timer_stop(self) -> float:
        ms = C.c_float()
        check(lib.rfi_timer_stop(self.handle, C.byref(ms)))
        return ms.value

    def profile(self, on: bool):
        check(lib.rfi_profile_enable(self.handle, 1 if on else 0))

    def profile_reset(self):
        check(lib.rfi_profile_reset(self.handle))

    def profile_dump(self, path: str):
        check(lib.rfi_profile_dump(self.handle, path.encode()))

    def profile_report(self) -> dict:
        out = {}
        for f in range(lib.rfi_profile_family_count()):
            n, ms, fl, by = C.c_int64(), C.c_double(), C.c_double(), C.c_double()
            check(lib.rfi_profile_get(self.handle, f, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)))
            if n.value:
                out[lib.rfi_profile_family_name(f).decode()] = {
                    "launches": n.value, "ms": ms.value, "flops": fl.value, "bytes": by.value}
        return out

    # ---- RCCL
    def comm_init(self, unique_id: bytes, rank: int, world: int):
        buf = C.create_string_buffer(unique_id, 128)
        check(lib.rfi_comm_init(self.handle, buf, rank, world))
        self._comm = True

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        check(lib.rfi_comm_unique_id(buf))
        return buf.raw

    def comm_emulate(self, world: int):
        """Single-GPU test mode of the bucketed gradient exchange (0 = off): see include/rfi_hip.h."""
        check(lib.rfi_comm_emulate(self.handle, int(world)))

    def comm_destroy(self):
        if self._comm:
            check(lib.rfi_comm_destroy(self.handle))
            self._comm = False


class DeviceArray:
    """A typed HBM buffer owned by a Context (freed on garbage collection)."""

    def __init__(self, ctx: Context, shape, dtype):
        self.ctx = ctx
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.ptr = ctx.malloc(self.nbytes)

    @classmethod
    def borrow(cls, ctx: Context, ptr: int, shape, dtype, owner) -> "DeviceArray":
        """A typed view of device memory that `owner` (kept referenced) holds: a slice of a DeviceArray or of a CUDA
        tensor, for the functions that take a DeviceArray.  Never freed here."""
        if owner is None:
            raise ValueError("a borrowed view needs the object that owns the memory")
        v = cls.__new__(cls)
        v.ctx, v.shape, v.dtype = ctx, tuple(int(s) for s in shape), np.dtype(dtype)
        v.nbytes = int(np.prod(v.shape, dtype=np.int64)) * v.dtype.itemsize
        v.ptr, v._owner = None, owner              # (`ptr` is set last: __del__ frees what it finds without `_owner`)
        v.ptr = int(ptr)
        return v

    def numpy(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=self.dtype)
        if self.nbytes:
            check(lib.rfi_memcpy(self.ctx.handle, out.ctypes.data_as(C.c_void_p), HOST, C.c_void_p(self.ptr),
                                 DEVICE, self.nbytes))
        return out

    def copy_from(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr, dtype=self.dtype)
        assert arr.nbytes == self.nbytes
        check(lib.rfi_memcpy(self.ctx.handle, C.c_void_p(self.ptr), DEVICE, arr.ctypes.data_as(C.c_void_p),
                             HOST, self.nbytes))

    def zero_(self):
        check(lib.rfi_memset(self.ctx.handle, C.c_void_p(self.ptr), 0, self.nbytes))

    def __del__(self):
        try:
            if getattr(self, "ptr", None) and getattr(self, "_owner", None) is None:
                self.ctx.free(self.ptr)
                self.ptr = None
        except Exception:
            pass


def is_torch(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor)


# ---------------------------------------------------------------------------------------------- array arguments
# Every public function takes NumPy arrays, torch CPU / CUDA tensors and DeviceArrays; what follows turns one into what
# the C ABI wants and is the only place that does.
_TORCH_NP = {} if torch is None else {
    torch.bool: np.bool_, torch.uint8: np.uint8, torch.int8: np.int8, torch.int16: np.int16, torch.int32: np.int32,
    torch.int64: np.int64, torch.float16: np.float16, torch.float32: np.float32, torch.float64: np.float64,
    torch.complex64: np.complex64, torch.complex128: np.complex128}
_TORCH_NP = {t: np.dtype(d) for t, d in _TORCH_NP.items()}
_NP_TORCH = {d: t for t, d in _TORCH_NP.items()}
_U8, _BOOL = np.dtype(np.uint8), np.dtype(np.bool_)

Operand = namedtuple("Operand", "ptr mem dtype shape size keep")
Operand.__doc__ = """An array argument as the C ABI takes it: pointer, HOST / DEVICE, the NumPy dtype behind the pointer,
shape and element count of the caller's array, and what must stay referenced until the work that reads it is done."""


def describe(x):
    """-> (shape, NumPy dtype or None for a torch dtype NumPy lacks, GPU index or None, owning Context or None).
    Nothing is copied, no device is touched and no context is made: argument checks build on this."""
    if isinstance(x, DeviceArray):
        return x.shape, x.dtype, x.ctx.device_index, x.ctx
    if is_torch(x):
        return tuple(int(s) for s in x.shape), _TORCH_NP.get(x.dtype), (x.device.index or 0) if x.is_cuda else None, None
    x = np.asarray(x)
    return x.shape, x.dtype, None, None


def context_for(device, *xs) -> Context:
    """The context a call runs on: that of a DeviceArray among `xs`; else, when `device` is None, the GPU of a CUDA
    tensor among them; else ``Context.get(device)``.  A `device` that names another context than the DeviceArray's is
    refused here; every other input the choice contradicts is refused by ``operand``."""
    for x in xs:
        if isinstance(x, DeviceArray):
            if device is not None and Context._cache.get((os.getpid(), _parse_device(device))) is not x.ctx:
                raise ValueError(f"device array belongs to another context than that of device={device!r}")
            return x.ctx
    if device is None:
        for x in xs:
            if is_torch(x) and x.is_cuda:
                return Context.get(x.device.index or 0)
    return Context.get(device)


def _convert(dt, accept, other, error):
    """The dtype policy of ``operand``: -> (dtype the kernel gets, None | "view" | "cast" | "nonzero" to get there)."""
    if dt is not None and dt in accept:          # (np.dtype(np.float64) == None holds: NumPy reads None as float64)
        return dt, None
    if dt is not None and dt == _BOOL and _U8 in accept:
        return _U8, "view"
    if other == "cast":
        return accept[0], "cast"
    if other == "nonzero":
        return _U8, "nonzero"
    if other == "widen" and dt is not None and dt.kind in "biu":
        return np.dtype(np.float64), "cast"
    raise error(dt) if error else TypeError(f"dtype {dt} is not accepted here ({', '.join(str(d) for d in accept)})")


def operand(x, ctx, accept, other="reject", error=None, to_device=False) -> Operand:
    """`x` (DeviceArray, NumPy array, torch CPU / CUDA tensor) as a contiguous array of one of the dtypes `accept`.

    bool passes as its bytes where uint8 is accepted.  `other` says what becomes of every other dtype: "cast" to
    ``accept[0]``, "nonzero" (``x != 0`` as uint8), "widen" (bool and integers to float64) or "reject"; what is not
    covered raises ``error(dtype)``.  A DeviceArray is never converted.  Host data stays on the host and `ctx` is not
    touched unless `to_device` uploads it (for kernels that read HBM only).  Refused with ValueError: a CUDA tensor on
    another GPU than `ctx`'s, a DeviceArray of another context."""
    accept = tuple(np.dtype(d) for d in accept)
    if isinstance(x, DeviceArray):
        dt = _U8 if x.dtype == _BOOL and _U8 in accept else x.dtype
        if dt not in accept:
            raise error(dt) if error else TypeError(f"device array has dtype {dt}, expected {' or '.join(str(a) for a in accept)}")
        if x.ctx is not ctx:
            raise ValueError("device array belongs to another context")
        return Operand(x.ptr, DEVICE, dt, x.shape, math.prod(x.shape), x)
    if is_torch(x):
        t = x.detach()
        dt, how = _convert(_TORCH_NP.get(t.dtype), accept, other, error)
        if how is not None:
            t = t.to(_NP_TORCH[dt]) if how == "cast" else (t if how == "view" else t != 0).view(torch.uint8)
        t = t.contiguous()
        if t.is_cuda:
            if t.device.index not in (None, ctx.device_index):
                raise ValueError(f"tensor is on {t.device}, the context on GPU {ctx.device_index}")
            # torch's work on the tensor is queued on torch's stream, the kernel on the context's: wait for the first
            torch.cuda.current_stream(t.device).synchronize()
            return Operand(t.data_ptr(), DEVICE, dt, tuple(x.shape), t.numel(), t)
        a = t.numpy()
    else:
        a = np.asarray(x)
        dt, how = _convert(a.dtype, accept, other, error)
        if how is not None:
            a = a.astype(dt) if how == "cast" else (a if how == "view" else a != 0).view(np.uint8)
    shape, a = a.shape, np.ascontiguousarray(a)            # (a 0-d array comes back 1-d: the shape is the caller's)
    if to_device:
        d = ctx.to_device(a)
        return Operand(d.ptr, DEVICE, dt, shape, a.size, d)
    return Operand(a.ctypes.data, HOST, dt, shape, a.size, a)


def as_pointer(x, dtype, ctx: Context):
    """-> (ptr, mem, keepalive) of `x` as contiguous `dtype`, cast where it is another."""
    o = operand(x, ctx, (dtype,), "cast")
    return o.ptr, o.mem, o.keep


def check_out(out):
    if out not in ("host", "device"):
        raise ValueError(f"out must be 'host' or 'device', got {out!r}")


def result_buffer(ctx, shape, dtype, out, like):
    """-> (result, ptr, mem): a DeviceArray for ``out="device"``; else a torch tensor on `like`'s GPU when `like` is a
    CUDA tensor, else a NumPy array."""
    if out == "device":
        res = ctx.empty(shape, dtype)
        return res, res.ptr, DEVICE
    if is_torch(like) and like.is_cuda:
        res = torch.empty(shape, dtype=_NP_TORCH[np.dtype(dtype)], device=like.device)
        # torch's allocator may hand out memory that work still queued on torch's stream uses: wait for it
        torch.cuda.current_stream(like.device).synchronize()
        return res, res.data_ptr(), DEVICE
    res = np.empty(shape, dtype)
    return res, res.ctypes.data, HOST


def P(d):
    """c_void_p of what holds a device pointer in ``.ptr`` (None stays None)."""
    return None if d is None else C.c_void_p(d.ptr)


def ptr_mem(a):
    """-> (c_void_p or None, memory kind) of a DeviceArray, a NumPy array or None."""
    if isinstance(a, DeviceArray):
        return P(a), DEVICE
    return (None if a is None else a.ctypes.data_as(C.c_void_p)), HOST
