"""RFISimulator: the reference's time-frequency RFI simulator (rfi_toolbox/core/simulator.py) on the GPU.

Same public attributes, defaults and return values as the reference class; the physics, the order of addition
and the masks are the reference's, computed in fp64 on the device by ``rfi_simulate_rfi`` (csrc/rfi_sim.hip).
The random stream is NOT NumPy's global generator: every draw comes from Philox4x32-10 keyed by ``seed`` and
counted by (position, event, stream, global sample index), with the word -> value mappings written in
include/rfi_hip.h.  The simulator keeps a running sample counter, so ``generate_batch(4)`` equals
``generate_batch(2)`` twice and four ``generate_rfi()`` calls, bit for bit.

``generate_rfi`` / ``generate_clean_data`` copy one sample back and update ``tf_plane``, ``mask`` and
``baseline_frac`` as the reference does.  ``generate_batch`` leaves its results in HBM (DeviceArray) for
``UNet(8, ...).train_step`` and leaves ``tf_plane`` / ``mask`` / ``baseline_frac`` untouched.

Injection.  ``inject`` adds the same events -- sample i of the call gets the event table and every per-pixel draw that
``generate_batch`` would give the sample of the same index; the noise stream is not drawn -- to visibilities that already
exist (``rfi_sim_inject``): per pixel in fp64, every contribution v enters as (sigma v.re, sigma v.im) with the sample's
noise scale sigma, RL / LR get the cross-hand factor times what was injected into RR, and a visibility that is
prior-flagged or that no event touches is stored exactly as it was loaded.  The mask is the injection truth, decided in
noise units, whatever the flags say.  What the truth does not cover: RFI the data already holds is unlabelled unless
the prior flags mark it -- pass those pixels as ``flags`` and treat them as invalid downstream
(``tile_labels(..., invalid=invalid_map(data, flags))``).
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

POLS = ("RR", "RL", "LR", "LL")
# rfi_sim_event of include/rfi_hip.h (64 bytes per record)
EVENT_DTYPE = np.dtype([("i0", "<i4"), ("i1", "<i4"), ("i2", "<i4"), ("i3", "<i4"), ("s0", "<f8"), ("sdot", "<f8"),
                        ("r0", "<f8"), ("phi0", "<f8"), ("v0", "<f8"), ("v1", "<f8")])
_LAYOUTS = {"complex128": 0, "complex64": 1, "nchw": 2, "nhwc": 3}
_ROWS = {"time": 0, "channel": 1}                # RFI_INJECT_ROWS_*
_CROSS = {"injected": 0, "reference": 1}         # RFI_INJECT_CROSS_*
IQR_PER_SIGMA = 1.3489795003921634               # q75 - q25 of a unit normal


def _checked_sigma(sigma):
    bad = np.flatnonzero(~(np.isfinite(sigma) & (sigma > 0)))
    if bad.size:
        raise ValueError(f"the noise scale of sample {int(bad[0])} is {sigma[bad[0]]!r}: it must be finite and positive "
                         "(a sample without a valid visibility, or constant data, has no scale of its own: pass scale=)")
    return np.ascontiguousarray(sigma, dtype=np.float64)

SimOrigin = namedtuple("SimOrigin", ["seed", "first_sample", "T", "F", "params", "power"])
SimOrigin.__doc__ = """What generated a SimBatch: the Philox key ``seed``, the global index ``first_sample`` of its sample 0,
the plane size, the filled ``SimParams`` of the call (a snapshot: detect_floor, fringes, ...) and the device power table
it drew from (held here, so it outlives a later change of ``power_range``)."""


class SimBatch(namedtuple("SimBatch", ["data", "mask", "baseline_frac", "events"])):
    """generate_batch's result, all in HBM: data DeviceArray (layout of ``out``), mask DeviceArray
    (n, T, F) uint8, baseline_frac DeviceArray (n,) float64 (None when clean), events DeviceArray
    (n, event_slots(T, F)) of EVENT_DTYPE (None when clean).  A 4-tuple of those; the attribute ``origin`` (SimOrigin,
    not a field) carries what ``event_table`` / ``event_instances`` need to recompute each event's own pixels.
    ``rows``: "time" (planes and mask (T, F)) or, for an ``inject(rows="channel")`` batch, "channel" ((F, T)); ``noise_scale``:
    the (n,) float64 sigma an ``inject`` call scaled its events by (None for a generated batch)."""
    origin = None
    rows = "time"
    noise_scale = None

    def __new__(cls, data, mask, baseline_frac, events, origin=None, rows="time", noise_scale=None):
        self = super().__new__(cls, data, mask, baseline_frac, events)
        self.origin = origin
        self.rows = rows
        self.noise_scale = noise_scale
        return self


def event_slots(time_bins, freq_bins):
    """Records per sample in the device event table (RFI_SIM_SLOTS): header, 3 broadband, int(F*0.05)
    narrowband, int(T*0.1) bursts, 5 linear and 5 quadratic sweeps."""
    return 14 + int(freq_bins * 0.05) + int(time_bins * 0.1)


class RFISimulator:
    """Drop-in for ``rfi_toolbox.core.RFISimulator`` generating on the GPU (see the module docstring).

    seed: the Philox key (None draws one from the OS); device: the GPU (None: LOCAL_RANK or 0)."""

    def __init__(self, time_bins=1024, freq_bins=1024, *, seed=None, device=None):
        for v, nm in ((time_bins, "time_bins"), (freq_bins, "freq_bins")):
            if not isinstance(v, (int, np.integer)) or v <= 0:
                raise ValueError(f"{nm} must be a positive integer, got {v!r}")
        self.time_bins = int(time_bins)
        self.freq_bins = int(freq_bins)
        self.power_range = np.logspace(-6, 4, num=100)
        self.detect_floor = 1.0
        self.drift_prob = 0.3
        self.max_time_fringes = 30.0
        self.max_freq_fringes = 8.0
        self.gibbs_ringing = False
        self._gibbs_kernel = self._make_gibbs_kernel(n_side=8, stretch=2.0)
        self.baseline_frac = 0.5
        self.tf_plane = {pol: np.empty((self.time_bins, self.freq_bins), dtype=complex) for pol in POLS}
        self.mask = np.zeros((self.time_bins, self.freq_bins), dtype=bool)
        self.seed = int(np.random.SeedSequence().entropy) & (2 ** 64 - 1) if seed is None else int(seed) & (2 ** 64 - 1)
        self.sample_counter = 0          # global index of the next sample (the Philox counter's c3)
        self.device = device
        self._ctx = None
        self._power_host = None
        self._power_dev = None

    # ---- the reference's deterministic helpers (simulator.py:92-100)
    @staticmethod
    def _phase_grid(t_idx, n_idx, params):
        s0, sdot, r0, phi0 = params
        return 2 * np.pi * ((s0 + sdot * t_idx) * n_idx + r0 * t_idx) + phi0

    @staticmethod
    def _make_gibbs_kernel(n_side=8, stretch=2.0):
        x = np.arange(-n_side, n_side + 1) / float(stretch)
        k = np.sinc(x)
        return k / k.sum()

    # ---- checks (before any context is created or anything is allocated)
    def _check(self, clean):
        T, F = self.time_bins, self.freq_bins
        if not clean and T < 4:
            raise ValueError(f"generate_rfi needs time_bins >= 4 (randint(0, time_bins // 4)), got {T}")
        if not clean and F < 52:
            raise ValueError(f"generate_rfi needs freq_bins >= 52 (randint(50, min(150, freq_bins - 1))), got {F}")
        if T * F >= 2 ** 32:
            raise ValueError("time_bins * freq_bins must stay below 2**32")
        pr = np.ascontiguousarray(np.asarray(self.power_range, dtype=np.float64).ravel())
        if not 1 <= pr.size <= 1024:
            raise ValueError(f"power_range must have 1 to 1024 entries, got {pr.size}")
        k = np.ascontiguousarray(np.asarray(self._gibbs_kernel, dtype=np.float64).ravel())
        if k.size != 17:
            raise ValueError("the Gibbs kernel must have 17 taps (n_side=8)")
        return pr, k

    def _context(self):
        from ..runtime import Context
        if self._ctx is None:
            self._ctx = Context.get(self.device)
        return self._ctx

    def _params(self, ctx, pr, k, clean, baseline_frac):
        """The filled SimParams of a call (the power table goes to the device when it changed)."""
        from .._lib import SimParams
        if self._power_host is None or not np.array_equal(self._power_host, pr):
            self._power_dev = ctx.to_device(pr)
            self._power_host = pr.copy()
        p = SimParams()
        p.time_bins, p.freq_bins, p.n_power = self.time_bins, self.freq_bins, pr.size
        p.gibbs_ringing = 1 if self.gibbs_ringing else 0
        p.clean = 1 if clean else 0
        p.fixed_baseline = 0 if baseline_frac is None else 1
        p.baseline_frac = 0.0 if baseline_frac is None else float(baseline_frac)
        p.detect_floor, p.drift_prob = float(self.detect_floor), float(self.drift_prob)
        p.max_time_fringes, p.max_freq_fringes = float(self.max_time_fringes), float(self.max_freq_fringes)
        for i in range(17):
            p.gibbs_kernel[i] = float(k[i])
        return p

    def _run(self, n, baseline_frac, clean, out):
        if out not in _LAYOUTS:
            raise ValueError(f"out must be one of {sorted(_LAYOUTS)}, got {out!r}")
        if not isinstance(n, (int, np.integer)) or n < 0:
            raise ValueError(f"n must be a non-negative integer, got {n!r}")
        n = int(n)
        pr, k = self._check(clean)
        if self.sample_counter + n > 2 ** 32:
            raise ValueError("the sample counter would pass 2**32: start a new simulator with another seed")
        from .._lib import check, lib
        T, F = self.time_bins, self.freq_bins
        ctx = self._context()
        p = self._params(ctx, pr, k, clean, baseline_frac)
        if out in ("complex128", "complex64"):
            data = ctx.empty((n, 4, T, F), np.complex128 if out == "complex128" else np.complex64)
        elif out == "nchw":
            data = ctx.empty((n, 8, T, F), np.float32)
        else:
            data = ctx.empty((n, T, F, 8), np.float32)
        mask = ctx.empty((n, T, F), np.uint8)
        events = None if clean else ctx.empty((n, event_slots(T, F)), EVENT_DTYPE)
        bl = None if clean else ctx.empty((n,), np.float64)
        check(lib.rfi_simulate_rfi(ctx.handle, self.seed, self.sample_counter, n, C.byref(p),
                                   C.c_void_p(self._power_dev.ptr), _LAYOUTS[out], C.c_void_p(data.ptr),
                                   C.c_void_p(mask.ptr), C.c_void_p(events.ptr) if events is not None else None,
                                   C.c_void_p(bl.ptr) if bl is not None else None))
        origin = SimOrigin(self.seed, self.sample_counter, T, F, p, self._power_dev)
        self.sample_counter += n
        return SimBatch(data, mask, bl, events, origin)

    # ---- the reference's surface
    def generate_clean_data(self):
        """Unit-variance complex Gaussian planes (simulator.py:137-145) -> (tf_plane, mask)."""
        r = self._run(1, None, True, "complex128")
        planes = r.data.numpy()[0]
        self.tf_plane = {pol: planes[i] for i, pol in enumerate(POLS)}
        self.mask = np.zeros((self.time_bins, self.freq_bins), dtype=bool)
        return self.tf_plane, self.mask

    def generate_rfi(self, baseline_frac=None):
        """An RFI-contaminated plane and its full-truth mask (simulator.py:147-237) -> (tf_plane, mask).
        baseline_frac: baseline length in [0, 1]; None draws one per call."""
        self._check(False)
        r = self._run(1, None if baseline_frac is None else float(baseline_frac), False, "complex128")
        planes = r.data.numpy()[0]
        self.mask = r.mask.numpy()[0].view(np.bool_)
        self.baseline_frac = float(r.baseline_frac.numpy()[0])
        self.tf_plane = {pol: planes[i] for i, pol in enumerate(POLS)}
        return self.tf_plane, self.mask

    def generate_batch(self, n, baseline_frac=None, clean=False, out="complex64"):
        """n samples generated and left in HBM -> SimBatch(data, mask, baseline_frac, events).

        out: "complex128" / "complex64" planes (n, 4, T, F) in the order RR, RL, LR, LL; "nchw" (n, 8, T, F)
        float32 in save_example_pair_npy's channel order (RR.re, RR.im, RL.re, RL.im, LR.re, LR.im, LL.re,
        LL.im); "nhwc" (n, T, F, 8) float32, the input of ``UNet(8, ...).train_step``.  clean=True gives
        generate_clean_data's planes (empty masks, no events).  Unlike generate_rfi this copies nothing back
        and does not touch ``tf_plane``, ``mask`` or ``baseline_frac``."""
        return self._run(n, None if baseline_frac is None else float(baseline_frac), bool(clean), out)

    # ---- injection into existing visibilities
    def inject(self, data, flags=None, scale="iqr", rows="time", cross_hand="injected", baseline_frac=None, inplace=False):
        """Add this simulator's emitters to visibilities that already exist -> SimBatch (module docstring, "Injection").

        data: complex64 / complex128 (n, 4, R, S), RR, RL, LR, LL (NumPy, torch or DeviceArray).  rows="time": planes
        (time_bins, freq_bins); rows="channel": MSLoader's (freq_bins, time_bins), simulator pixel (t, f) at [f, t].
        flags: prior flags (n, 4, R, S) or (n, R, S), uint8 / bool: a flagged visibility comes back bit for bit.
        scale: the data's noise sigma per sample, a float, (n,) values, or "iqr": (q75 - q25) / 1.3489795003921634 of the
        sample's valid scalars (flagged and non-finite visibilities left out).  cross_hand "injected": RL / LR get
        factor x what was added to RR; "reference": factor x the whole RR (no flags then).  inplace=True writes into a
        DeviceArray / GPU tensor; otherwise the result is a new DeviceArray.  Sample i gets the events generate_batch
        would give it, and ``sample_counter`` advances by n."""
        from ..runtime import DeviceArray, context_for, describe, operand
        if rows not in _ROWS:
            raise ValueError(f"rows must be 'time' or 'channel', got {rows!r}")
        if cross_hand not in _CROSS:
            raise ValueError(f"cross_hand must be 'injected' or 'reference', got {cross_hand!r}")
        if cross_hand == "reference" and flags is not None:
            raise ValueError("cross_hand='reference' adds factor x the whole RR, flagged or not: it takes no flags")
        shape, dt = describe(data)[:2]
        shape = tuple(int(v) for v in shape)
        if dt is None or dt not in (np.dtype(np.complex64), np.dtype(np.complex128)):
            raise TypeError(f"data must be complex64 or complex128, not {dt}")
        if len(shape) != 4 or shape[1] != 4:
            raise ValueError(f"data must be (n, 4, R, S) in the order RR, RL, LR, LL, got shape {shape}")
        T, F = self.time_bins, self.freq_bins
        want = (T, F) if rows == "time" else (F, T)
        if shape[2:] != want:
            raise ValueError(f"rows={rows!r} needs planes {want} (time_bins {T}, freq_bins {F}), got {shape[2:]}")
        n = shape[0]
        flag_pols = 0
        if flags is not None:
            fshape, fdt = describe(flags)[:2]
            fshape = tuple(int(v) for v in fshape)
            if fdt is None or fdt not in (np.dtype(np.uint8), np.dtype(np.bool_)):
                raise TypeError(f"flags must be uint8 or bool, not {fdt}")
            if fshape not in (shape, (n,) + want):
                raise ValueError(f"flags must be per polarisation {shape} or per baseline {(n,) + want}, got shape {fshape}")
            flag_pols = 4 if fshape == shape else 1
        sigma = None
        if not isinstance(scale, str):
            sigma = np.asarray(scale, dtype=np.float64)
            if sigma.shape not in ((), (n,)):
                raise ValueError(f"scale must be a float, {n} values or 'iqr', got shape {sigma.shape}")
            sigma = _checked_sigma(np.broadcast_to(sigma, (n,)).copy())
        elif scale != "iqr":
            raise ValueError(f"scale must be a float, {n} values or 'iqr', got {scale!r}")
        on_device = isinstance(data, DeviceArray) or (hasattr(data, "is_cuda") and data.is_cuda)
        if inplace and not on_device:
            raise ValueError("inplace=True needs a DeviceArray or a GPU tensor")
        if inplace and not isinstance(data, DeviceArray) and not data.is_contiguous():
            raise ValueError("inplace=True needs a contiguous tensor")
        pr, k = self._check(False)
        if self.sample_counter + n > 2 ** 32:
            raise ValueError("the sample counter would pass 2**32: start a new simulator with another seed")
        from .._lib import check, lib
        if self._ctx is None:
            self._ctx = context_for(self.device, data, flags)
        ctx = self._ctx
        p = self._params(ctx, pr, k, False, None if baseline_frac is None else float(baseline_frac))
        origin = SimOrigin(self.seed, self.sample_counter, T, F, p, self._power_dev)
        mask = ctx.empty((n,) + want, np.uint8)
        events = ctx.empty((n, event_slots(T, F)), EVENT_DTYPE)
        bl = ctx.empty((n,), np.float64)
        if n == 0:
            out = data if inplace and isinstance(data, DeviceArray) else ctx.empty(shape, dt)
            return SimBatch(out, mask, bl, events, origin, rows=rows, noise_scale=np.zeros(0) if sigma is None else sigma)
        src = operand(data, ctx, (np.complex64, np.complex128), to_device=True)
        view = data if isinstance(data, DeviceArray) else DeviceArray.borrow(ctx, src.ptr, shape, dt, src.keep)
        fo = None if flags is None else operand(flags, ctx, (np.uint8,), to_device=True)
        if sigma is None:
            fview = None if fo is None else DeviceArray.borrow(ctx, fo.ptr, fo.shape, np.uint8, fo.keep)
            sigma = _checked_sigma(self._iqr_sigma(view, fview, n))
        out = view if inplace else ctx.empty(shape, dt)
        sigma_dev = ctx.to_device(sigma)
        check(lib.rfi_sim_inject(ctx.handle, self.seed, self.sample_counter, n, C.byref(p), C.c_void_p(self._power_dev.ptr),
                                 _LAYOUTS[dt.name], _ROWS[rows], _CROSS[cross_hand], C.c_void_p(src.ptr),
                                 None if fo is None else C.c_void_p(fo.ptr), flag_pols, C.c_void_p(sigma_dev.ptr),
                                 C.c_void_p(out.ptr), C.c_void_p(mask.ptr), C.c_void_p(events.ptr), C.c_void_p(bl.ptr)))
        if src.keep is not data or (fo is not None and fo.keep is not flags):
            ctx.synchronize()                           # (an uploaded or converted copy of data / flags goes with this frame)
        self.sample_counter += n
        batch = SimBatch(out, mask, bl, events, origin, rows=rows, noise_scale=sigma)
        batch._sigma_dev = sigma_dev                    # (read by the kernel just queued: lives as long as its results)
        return batch

    @staticmethod
    def _iqr_sigma(view, flags, n):
        """(n,) float64: each sample's (q75 - q25) / 1.3489795003921634 over its valid real scalars -- the quartiles
        ``Normalizer("robust_scale", scope="sample")`` gets (NaN where a sample has no valid scalar)."""
        from ..preprocessing.normalization import Normalizer, quantiles_from_brackets
        sigma = np.full(n, np.nan)
        if n == 0:
            return sigma
        stats = Normalizer("robust_scale", scope="sample").statistics(view, flags="nonfinite" if flags is None else flags)
        for i, st in enumerate(stats):
            if st["count"]:
                _, q25, q75 = quantiles_from_brackets(st["count"], st["q"])
                sigma[i] = (q75 - q25) / IQR_PER_SIGMA
        return sigma
