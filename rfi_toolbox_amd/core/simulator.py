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

SimOrigin = namedtuple("SimOrigin", ["seed", "first_sample", "T", "F", "params", "power"])
SimOrigin.__doc__ = """What generated a SimBatch: the Philox key ``seed``, the global index ``first_sample`` of its sample 0,
the plane size, the filled ``SimParams`` of the call (a snapshot: detect_floor, fringes, ...) and the device power table
it drew from (held here, so it outlives a later change of ``power_range``)."""


class SimBatch(namedtuple("SimBatch", ["data", "mask", "baseline_frac", "events"])):
    """generate_batch's result, all in HBM: data DeviceArray (layout of ``out``), mask DeviceArray
    (n, T, F) uint8, baseline_frac DeviceArray (n,) float64 (None when clean), events DeviceArray
    (n, event_slots(T, F)) of EVENT_DTYPE (None when clean).  A 4-tuple of those; the attribute ``origin`` (SimOrigin,
    not a field) carries what ``event_table`` / ``event_instances`` need to recompute each event's own pixels."""
    origin = None

    def __new__(cls, data, mask, baseline_frac, events, origin=None):
        self = super().__new__(cls, data, mask, baseline_frac, events)
        self.origin = origin
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

    def _run(self, n, baseline_frac, clean, out):
        if out not in _LAYOUTS:
            raise ValueError(f"out must be one of {sorted(_LAYOUTS)}, got {out!r}")
        if not isinstance(n, (int, np.integer)) or n < 0:
            raise ValueError(f"n must be a non-negative integer, got {n!r}")
        n = int(n)
        pr, k = self._check(clean)
        if self.sample_counter + n > 2 ** 32:
            raise ValueError("the sample counter would pass 2**32: start a new simulator with another seed")
        from .._lib import SimParams, check, lib
        T, F = self.time_bins, self.freq_bins
        ctx = self._context()
        if self._power_host is None or not np.array_equal(self._power_host, pr):
            self._power_dev = ctx.to_device(pr)
            self._power_host = pr.copy()
        p = SimParams()
        p.time_bins, p.freq_bins, p.n_power = T, F, pr.size
        p.gibbs_ringing = 1 if self.gibbs_ringing else 0
        p.clean = 1 if clean else 0
        p.fixed_baseline = 0 if baseline_frac is None else 1
        p.baseline_frac = 0.0 if baseline_frac is None else float(baseline_frac)
        p.detect_floor, p.drift_prob = float(self.detect_floor), float(self.drift_prob)
        p.max_time_fringes, p.max_freq_fringes = float(self.max_time_fringes), float(self.max_freq_fringes)
        for i in range(17):
            p.gibbs_kernel[i] = float(k[i])
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
