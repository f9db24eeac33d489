"""TEST INFRASTRUCTURE ONLY -- NumPy restatement of RFISimulator.inject (rfi_sim_inject of rfi_toolbox_amd/csrc/rfi_sim.hip)
on top of tests/rfisim_ref.RefSimulator.

``RefInjector.inject`` runs ``RefSimulator.generate_rfi`` itself -- its draws, its event code, its order of addition --
with the four planes replaced by accumulators that apply the injection rules of include/rfi_hip.h to every ``+=`` the
event code makes: the planes start as the given data (complex64 widened), a contribution v is added as
(sigma v.re, sigma v.im), RR's contributions are also summed into S, and a visibility remembers whether anything was
added to it.  The cross-hand line ``plane += factor * RR`` becomes ``+ factor S`` where RR was touched ("injected") or
stays the reference's expression on the accumulated RR ("reference").  Flagged and untouched visibilities are copied
back from the input, bit for bit.  The noise stream is never drawn.
"""
import numpy as np

from rfisim_ref import RefSimulator, _cplx

POLS = ("RR", "RL", "LR", "LL")
IQR_PER_SIGMA = 1.3489795003921634


def valid_scalars(data, flags=None):
    """float64 real scalars (re and im) of the visibilities of one sample (4, R, S) that are finite and not flagged;
    flags: None, (4, R, S) or (R, S)."""
    data = np.asarray(data)
    ok = np.isfinite(data.real) & np.isfinite(data.imag)
    if flags is not None:
        ok &= ~np.broadcast_to(np.asarray(flags).astype(bool), data.shape)
    return np.concatenate([data.real[ok], data.imag[ok]]).astype(np.float64)


def iqr_sigma(data, flags=None):
    """(q75 - q25) / 1.3489795003921634 of the valid scalars, the quartiles formed as the device path forms them: the two
    bracketing order statistics of rank q (count - 1), then NumPy's _lerp between them.  NaN without a valid scalar."""
    x = np.sort(valid_scalars(data, flags))
    n = x.size
    if n == 0:
        return float("nan")

    def quantile(q):
        v = q * (n - 1)
        lo = int(np.floor(v))
        hi = min(lo + 1, n - 1)
        t, a, b = v - lo, float(x[lo]), float(x[hi])
        d = b - a
        return b - d * (1.0 - t) if t >= 0.5 else a + d * t
    return (quantile(0.75) - quantile(0.25)) / IQR_PER_SIGMA


class _Cross:
    """``factor * RR`` of the event code's cross-hand line, not yet formed"""

    def __init__(self, factor, rr):
        self.factor, self.rr = factor, rr


class _Slot:
    """``plane[idx]`` of an accumulating plane: ``plane[idx] += v`` lands in ``__iadd__``"""

    def __init__(self, plane, idx):
        self.plane, self.idx = plane, idx

    def __iadd__(self, v):
        p = self.plane
        v = np.asarray(v, dtype=np.complex128)
        c = _cplx(p.sigma * v.real, p.sigma * v.imag)          # each product rounded once, then added
        p.acc[self.idx] += c
        p.touched[self.idx] = True
        if p.S is not None:
            p.S[self.idx] += c
        return self


class _Plane:
    """one polarisation's fp64 accumulator; S: the array that also collects the contributions (RR only)"""
    __array_ufunc__ = None                                     # factor_array * plane -> plane.__rmul__

    def __init__(self, start, sigma, cross_hand, S=None):
        with np.errstate(invalid="ignore"):                    # (widening a signalling NaN)
            self.acc = np.array(start, dtype=np.complex128)
        self.touched = np.zeros(self.acc.shape, dtype=bool)
        self.sigma, self.cross_hand, self.S = sigma, cross_hand, S

    def __getitem__(self, idx):
        return _Slot(self, idx)

    def __setitem__(self, idx, slot):
        assert isinstance(slot, _Slot) and slot.plane is self   # (`p[idx] += v` stores the slot back: already applied)

    def __rmul__(self, factor):
        return _Cross(np.asarray(factor, dtype=np.float64), self)

    def __iadd__(self, x):
        assert isinstance(x, _Cross)
        rr = x.rr
        if self.cross_hand == "reference":                     # the reference's expression on the whole accumulated RR
            self.acc += x.factor * rr.acc
            self.touched[:] = True
        else:                                                  # factor * what was injected into RR, where anything was
            t = rr.touched
            add = _cplx(x.factor * rr.S.real, x.factor * rr.S.imag)
            self.acc[t] += add[t]
            self.touched |= t
        return self


class RefInjector(RefSimulator):
    """RefSimulator whose starting planes are the given data."""
    _inj = None

    def _clean(self):
        if self._inj is None:
            return super()._clean()
        d, sigma, cross = self._inj
        S = np.zeros((self.time_bins, self.freq_bins), dtype=np.complex128)
        self.tf_plane = {"RR": _Plane(d[0], sigma, cross, S), "RL": _Plane(d[1], sigma, cross), "LR": _Plane(d[2], sigma, cross),
                         "LL": _Plane(d[3], sigma, cross)}
        self.mask = np.zeros((self.time_bins, self.freq_bins), dtype=bool)
        return self.tf_plane, self.mask

    def inject(self, data, flags=None, scale="iqr", rows="time", cross_hand="injected", baseline_frac=None):
        """One sample: data (4, R, S) complex -> (planes (4, R, S) of data's dtype, mask (R, S) bool); ``noise_scale``,
        ``touched`` (4, R, S), ``ambiguous`` (R, S), ``events`` and ``baseline_frac`` are left on the object."""
        data = np.asarray(data)
        assert data.dtype in (np.complex64, np.complex128) and cross_hand in ("injected", "reference") and rows in ("time", "channel")
        assert not (cross_hand == "reference" and flags is not None)
        T, F = self.time_bins, self.freq_bins
        assert data.shape == ((4, T, F) if rows == "time" else (4, F, T)), data.shape
        fl = np.zeros(data.shape, dtype=bool) if flags is None else np.broadcast_to(np.asarray(flags).astype(bool), data.shape)
        sigma = iqr_sigma(data, flags) if isinstance(scale, str) else float(scale)
        assert scale == "iqr" or not isinstance(scale, str)
        if not (np.isfinite(sigma) and sigma > 0):
            raise ValueError(f"noise scale {sigma!r}")
        d = data if rows == "time" else data.transpose(0, 2, 1)
        fl = fl if rows == "time" else fl.transpose(0, 2, 1)
        self._inj = (d, sigma, cross_hand)
        try:
            self.generate_rfi(baseline_frac)
        finally:
            self._inj = None
        acc = np.stack([self.tf_plane[p].acc for p in POLS])
        touched = np.stack([self.tf_plane[p].touched for p in POLS])
        out = acc.astype(data.dtype)                           # the fp64 value rounded once
        keep = fl | ~touched
        out[keep] = d[keep]                                    # as loaded, bit for bit
        mask, amb = self.mask, self.ambiguous
        if rows == "channel":
            out, touched, mask, amb = out.transpose(0, 2, 1), touched.transpose(0, 2, 1), mask.T, amb.T
        out = np.ascontiguousarray(out)
        self.tf_plane = {p: out[i] for i, p in enumerate(POLS)}
        self.mask, self.ambiguous = np.ascontiguousarray(mask), np.ascontiguousarray(amb)
        self.touched, self.noise_scale = np.ascontiguousarray(touched), sigma
        return out, self.mask


def background(n, R, S, seed, dtype=np.complex128, scale=1.0):
    """(n, 4, R, S) planes that are not noise alone: a smooth bandpass along the last axis times a fringe, plus noise."""
    rng = np.random.default_rng(seed)
    r, s = np.arange(R)[:, None], np.arange(S)[None, :]
    band = 1.0 + 0.4 * np.cos(2 * np.pi * s / max(S, 2)) + 0.1 * np.sin(2 * np.pi * 3 * s / max(S, 2))
    out = np.empty((n, 4, R, S), dtype=np.complex128)
    for i in range(n):
        for p in range(4):
            fringe = np.exp(1j * (2 * np.pi * (0.013 * (p + 1) * r + 0.007 * (i + 1) * s) + 0.3 * p))
            noise = rng.standard_normal((R, S)) + 1j * rng.standard_normal((R, S))
            out[i, p] = scale * ((0.5 if p in (1, 2) else 2.0) * band * fringe + noise)
    return out.astype(dtype)
