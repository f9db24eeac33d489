"""TEST INFRASTRUCTURE ONLY -- NumPy restatement of the on-device RFISimulator (rfi_toolbox_amd/csrc/rfi_sim.hip).

It follows the reference's rfi_toolbox/core/simulator.py line by line (the same np.exp, np.convolve, np.outer and
+= order, complex128 throughout), with every np.random draw replaced by the Philox4x32-10 word the device uses
(oracle.synth_ref.philox4x32_10; the mappings are the ones written in include/rfi_hip.h).  Against the reference
itself the parity is distribution-level (tests/golden/simulator_expected.json); against the device it is to
libm rounding (fp64 sin/cos/log of the device library versus the host's).
"""
import numpy as np

from oracle.synth_ref import philox4x32_10

S_HEADER, S_BROAD, S_NARROW, S_BURST, S_LINEAR, S_QUAD = 0, 1, 2, 3, 4, 5
S_NOISE, S_BROAD_PX, S_NARROW_PT, S_BURST_PT, S_LINEAR_PT, S_QUAD_PT, S_CROSS = 8, 9, 10, 11, 12, 13, 14
EVENT_DTYPE = np.dtype([("i0", "<i4"), ("i1", "<i4"), ("i2", "<i4"), ("i3", "<i4"), ("s0", "<f8"), ("sdot", "<f8"),
                        ("r0", "<f8"), ("phi0", "<f8"), ("v0", "<f8"), ("v1", "<f8")])
AMBIGUOUS = 1e-12          # |field| this close to detect_floor may fall either way under a different libm


def u53(a, b):
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64)) \
        / 9007199254740992.0


def uniform(lo, hi, a, b):
    return lo + (hi - lo) * u53(a, b)


def randint(lo, hi, w):
    return lo + ((int(w) * (hi - lo)) >> 32)


def sign(w):
    return -1.0 if int(w) >> 31 else 1.0


def power_index(w, n):
    return (np.asarray(w, dtype=np.uint64) * np.uint64(n)) >> np.uint64(32)


def normals(a, b):
    r = np.sqrt(-2.0 * np.log((a.astype(np.float64) + 1.0) * (1.0 / 4294967296.0)))
    th = 6.283185307179586 * (b.astype(np.float64) * (1.0 / 4294967296.0))
    return r * np.cos(th), r * np.sin(th)


def _cplx(re, im):
    z = np.empty(re.shape, dtype=np.complex128)
    z.real, z.imag = re, im
    return z


class RefSimulator:
    """The reference class with Philox draws.  ``sample_counter`` counts samples as the device simulator does."""

    def __init__(self, time_bins=1024, freq_bins=1024, seed=0):
        self.time_bins = time_bins
        self.freq_bins = freq_bins
        self.power_range = np.logspace(-6, 4, num=100)
        self.detect_floor = 1.0
        self.drift_prob = 0.3
        self.max_time_fringes = 30.0
        self.max_freq_fringes = 8.0
        self.gibbs_ringing = False
        self._gibbs_kernel = self._make_gibbs_kernel(n_side=8, stretch=2.0)
        self.baseline_frac = 0.5
        self.tf_plane = {pol: np.empty((time_bins, freq_bins), dtype=complex) for pol in ("RR", "RL", "LR", "LL")}
        self.mask = np.zeros((self.time_bins, self.freq_bins), dtype=bool)
        self.seed = int(seed) & (2 ** 64 - 1)
        self.sample_counter = 0

    # ------------------------------------------------------------------ draws
    def _words(self, pos, event, stream):
        k0, k1 = self.seed & 0xFFFFFFFF, self.seed >> 32
        return philox4x32_10(pos, event, stream, self._sample, k0, k1)

    def _event_words(self, stream, k):
        w = []
        for j in range(5):
            w += [int(v[0]) for v in self._words([j], k, stream)]
        return w

    def _pixels(self, rows, cols):
        return (np.asarray(rows, dtype=np.uint64) * np.uint64(self.freq_bins) + np.asarray(cols, dtype=np.uint64))

    def _power(self, w):
        return np.asarray(self.power_range, dtype=np.float64).ravel()[power_index(w, np.size(self.power_range))]

    # ------------------------------------------------------------------ phase
    def _draw_event_phase(self, w, width_channels, n_times, drifting=False):
        wd = max(int(width_channels), 1)
        nt = max(int(n_times), 1)
        bl = self.baseline_frac
        n_ft = float(uniform(0.5, 1.0 + bl * self.max_time_fringes, w[8], w[9]))
        r0 = (n_ft / nt) * sign(w[10])
        n_ff = float(uniform(0.5, 1.0 + bl * self.max_freq_fringes, w[12], w[13]))
        s0 = (n_ff / wd) * sign(w[11])
        phi0 = float(uniform(0, 2 * np.pi, w[14], w[15]))
        if drifting:
            s_end = (float(uniform(0.5, 1.0 + bl * self.max_freq_fringes, w[6], w[7])) / wd) * sign(w[3])
            sdot = (s_end - s0) / nt
        else:
            sdot = 0.0
        return s0, sdot, r0, phi0

    @staticmethod
    def _phase_grid(t_idx, n_idx, params):
        s0, sdot, r0, phi0 = params
        return 2 * np.pi * ((s0 + sdot * t_idx) * n_idx + r0 * t_idx) + phi0

    # ------------------------------------------------------------------ gibbs
    @staticmethod
    def _make_gibbs_kernel(n_side=8, stretch=2.0):
        x = np.arange(-n_side, n_side + 1) / float(stretch)
        k = np.sinc(x)
        return k / k.sum()

    def _spread_block(self, pols, fslice, core):
        if self.gibbs_ringing:
            k = self._gibbs_kernel
            core = np.apply_along_axis(lambda m: np.convolve(m, k, mode="same"), 1, core)
        for pol in pols:
            self.tf_plane[pol][:, fslice] += core

    def _spread_line(self, pols, line, center, axis):
        if not self.gibbs_ringing:
            for pol in pols:
                if axis == 1:
                    self.tf_plane[pol][:, center] += line
                else:
                    self.tf_plane[pol][center, :] += line
            return
        k = self._gibbs_kernel
        n_side = (len(k) - 1) // 2
        size = self.freq_bins if axis == 1 else self.time_bins
        lo, hi = max(0, center - n_side), min(size, center + n_side + 1)
        kslice = k[(lo - center + n_side):(hi - center + n_side)]
        for pol in pols:
            if axis == 1:
                self.tf_plane[pol][:, lo:hi] += np.outer(line, kslice)
            else:
                self.tf_plane[pol][lo:hi, :] += np.outer(kslice, line)

    def _record(self, slot, i0=0, i1=0, i2=0, params=(0.0, 0.0, 0.0, 0.0), v0=0.0):
        self.events[slot] = (i0, i1, i2, 0, *params, v0, 0.0)

    # ------------------------------------------------------------------- data
    def _noise(self):
        T, F = self.time_bins, self.freq_bins
        pix = self._pixels(np.arange(T)[:, None], np.arange(F)[None, :]).ravel()
        a, b = self._words(pix, 0, S_NOISE), self._words(pix, 1, S_NOISE)
        planes = {}
        for pol, (x, y) in zip(("RR", "RL", "LR", "LL"), ((a[0], a[1]), (a[2], a[3]), (b[0], b[1]), (b[2], b[3]))):
            re, im = normals(x, y)
            planes[pol] = _cplx(re.reshape(T, F), im.reshape(T, F))
        return planes

    def generate_clean_data(self):
        self._sample = self.sample_counter
        self.sample_counter += 1
        return self._clean()

    def _clean(self):
        self.tf_plane = self._noise()
        self.mask = np.zeros((self.time_bins, self.freq_bins), dtype=bool)
        return self.tf_plane, self.mask

    def generate_rfi(self, baseline_frac=None):
        self._sample = self.sample_counter
        self.sample_counter += 1
        T, F = self.time_bins, self.freq_bins
        NN, NB = int(F * 0.05), int(T * 0.1)
        self.events = np.zeros(14 + NN + NB, dtype=EVENT_DTYPE)
        h = self._event_words(S_HEADER, 0)
        self.baseline_frac = float(u53(h[0], h[1])) if baseline_frac is None else float(baseline_frac)
        n_broad = 2 + randint(0, 2, h[2])
        self._record(0, i0=n_broad, v0=self.baseline_frac)
        self._clean()
        t_col = np.arange(T)[:, None]
        floor = self.detect_floor
        self.ambiguous = np.zeros((T, F), dtype=bool)

        # Broadband RFI: 2-3 separated frequency chunks (all three slots of the table are drawn).
        for b in range(3):
            w = self._event_words(S_BROAD, b)
            max_width = F - 1
            freq_start = randint(0, max(1, max_width - 100), w[0])
            freq_width = randint(50, min(150, max_width - freq_start), w[1])
            drifting = bool(u53(w[4], w[5]) < self.drift_prob)
            params = self._draw_event_phase(w, freq_width, T, drifting)
            self._record(1 + b, freq_start, freq_width, int(drifting), params)
            if b >= n_broad:
                continue
            n_row = np.arange(freq_start, freq_start + freq_width)[None, :]
            r = self._words(self._pixels(t_col, n_row), b, S_BROAD_PX)
            modulation = uniform(0.5, 2.0, r[0], r[1])
            power = self._power(r[2])
            field = (modulation * power) * np.exp(1j * self._phase_grid(t_col, n_row, params))
            fslice = slice(freq_start, freq_start + freq_width)
            self.mask[:, fslice] |= np.abs(field) > floor
            self.ambiguous[:, fslice] |= np.abs(np.abs(field) - floor) <= AMBIGUOUS
            self._spread_block(("RR", "LL"), fslice, field)

        # Narrowband RFI: single channels, ~5% of the band.
        t_lin = np.arange(T)
        for k in range(NN):
            w = self._event_words(S_NARROW, k)
            freq_idx = randint(0, F, w[0])
            rfi_val = self._power(w[1])
            drifting = bool(u53(w[4], w[5]) < self.drift_prob)
            params = self._draw_event_phase(w, 1, T, drifting)
            self._record(4 + k, freq_idx, int(drifting), int(power_index(w[1], np.size(self.power_range))), params,
                         rfi_val)
            r = self._words(t_lin, k, S_NARROW_PT)
            modulation = uniform(0.5, 2.0, r[0], r[1])
            field = (modulation * rfi_val) * np.exp(1j * self._phase_grid(t_lin, freq_idx, params))
            self.mask[np.abs(field) > floor, freq_idx] = True
            self.ambiguous[np.abs(np.abs(field) - floor) <= AMBIGUOUS, freq_idx] = True
            self._spread_line(("RR", "LL"), field, freq_idx, axis=1)

        # Time-bursty RFI: single time rows, ~10% of the scan.
        f_lin = np.arange(F)
        for k in range(NB):
            w = self._event_words(S_BURST, k)
            time_idx = randint(0, T, w[0])
            rfi_val = self._power(w[1])
            params = self._draw_event_phase(w, F, 1, drifting=False)
            self._record(4 + NN + k, time_idx, 0, int(power_index(w[1], np.size(self.power_range))), params, rfi_val)
            r = self._words(f_lin, k, S_BURST_PT)
            modulation = uniform(0.5, 2.0, r[0], r[1])
            field = (modulation * rfi_val) * np.exp(1j * self._phase_grid(time_idx, f_lin, params))
            self.mask[time_idx, np.abs(field) > floor] = True
            self.ambiguous[time_idx, np.abs(np.abs(field) - floor) <= AMBIGUOUS] = True
            self._spread_line(("RR", "LL"), field, time_idx, axis=0)

        # Linear sweeps.
        for k in range(5):
            w = self._event_words(S_LINEAR, k)
            start_t = randint(0, T // 2, w[0])
            start_f = randint(0, F // 2, w[1])
            slope = float(uniform(-2, 2, w[16], w[17]))
            drifting = bool(u53(w[4], w[5]) < self.drift_prob)
            params = self._draw_event_phase(w, 1, T // 2, drifting)
            self._record(4 + NN + NB + k, start_t, start_f, int(drifting), params, slope)
            amps = self._power(self._words(np.arange(T // 2), k, S_LINEAR_PT)[0])
            for i in range(T // 2):
                f_idx = int(start_f + slope * i) % F
                t_idx = (start_t + i) % T
                amp = amps[i]
                val = amp * np.exp(1j * self._phase_grid(t_idx, f_idx, params))
                for pol in ("RR", "LL"):
                    self.tf_plane[pol][t_idx, f_idx] += val
                if amp > floor:
                    self.mask[t_idx, f_idx] = True

        # Quadratic (time^2) sweeps.
        for k in range(5):
            w = self._event_words(S_QUAD, k)
            start_t = randint(0, T // 4, w[0])
            start_f = randint(0, F // 4, w[1])
            direction = int(sign(w[2]))
            params = self._draw_event_phase(w, 1, T // 4, drifting=True)
            self._record(9 + NN + NB + k, start_t, start_f, direction, params)
            amps = self._power(self._words(np.arange(T // 4), k, S_QUAD_PT)[0])
            for t in range(T // 4):
                f_idx = int(start_f + direction * (t**2) // 100) % F
                t_idx = (start_t + t) % T
                amp = amps[t]
                val = amp * np.exp(1j * self._phase_grid(t_idx, f_idx, params))
                self.tf_plane["RR"][t_idx, f_idx] += val
                if amp > floor:
                    self.mask[t_idx, f_idx] = True

        # Cross-hand RFI inherits the (coherent) parallel-hand structure.
        x = self._words(self._pixels(t_col, np.arange(F)[None, :]), 0, S_CROSS)
        for pol, (a, b) in (("RL", (x[0], x[1])), ("LR", (x[2], x[3]))):
            polarization_factor = uniform(0.0, 1.0, a, b)
            self.tf_plane[pol] += polarization_factor * self.tf_plane["RR"]

        return self.tf_plane, self.mask

    def planes(self):
        return np.stack([self.tf_plane[p] for p in ("RR", "RL", "LR", "LL")])


# ---------------------------------------------------------------------------------------------- statistics
# Distribution statistics of one sample, shared by tests/golden/make_simulator_golden.py (on the reference) and the
# tests (on this restatement and on the device).  planes: (4, T, F) complex in the order RR, RL, LR, LL.
STAT_DECILES = tuple(range(10, 100, 10))
LARGE_DIFF = 10.0          # |RR - LL| above this is RFI, not noise (the noise difference has sigma 2 per component)


def sample_stats(planes, mask):
    rr, rl, lr, ll = (np.asarray(p, dtype=np.complex128) for p in planes)
    mask = np.asarray(mask, dtype=bool)
    out = {"mask_frac": float(mask.mean())}
    a = np.abs(rr[mask])
    a = a[a > 0]
    dec = np.percentile(np.log10(a), STAT_DECILES) if a.size else np.full(len(STAT_DECILES), np.nan)
    for q, v in zip(STAT_DECILES, dec):
        out[f"log10_rr_masked_p{q}"] = float(v)
    e = float(np.sum(np.abs(rr) ** 2))
    out["xhand_rl"] = float(np.sum((rl * np.conj(rr)).real) / e)
    out["xhand_lr"] = float(np.sum((lr * np.conj(rr)).real) / e)
    out["rr_ll_large_frac"] = float(np.mean(np.abs(rr - ll)[mask] > LARGE_DIFF)) if mask.any() else 0.0
    pair = mask[:, 1:] & mask[:, :-1]
    z = rr[:, 1:][pair] * np.conj(rr[:, :-1][pair])
    out["coherence_f"] = float(np.mean(z.real / np.maximum(np.abs(z), 1e-300))) if z.size else 0.0
    return out


def clean_stats(planes):
    out = {}
    for name, p in zip(("RR", "RL", "LR", "LL"), planes):
        p = np.asarray(p, dtype=np.complex128)
        out[f"{name}_re_mean"] = float(p.real.mean())
        out[f"{name}_im_mean"] = float(p.imag.mean())
        out[f"{name}_re_var"] = float(p.real.var())
        out[f"{name}_im_var"] = float(p.imag.var())
        out[f"{name}_reim_corr"] = float(np.mean(p.real * p.imag))
    return out


def aggregate(per_seed):
    """[{stat: value}] over seeds -> {stat: {"mean", "std", "n"}}"""
    keys = per_seed[0].keys()
    out = {}
    for k in keys:
        v = np.array([s[k] for s in per_seed], dtype=np.float64)
        out[k] = {"mean": float(np.mean(v)), "std": float(np.std(v, ddof=1)), "n": int(v.size)}
    return out


def within_spread(got, ref, k=4.0, slack=0.0):
    """-> [failures]: |mean_got - mean_ref| must stay within k standard errors of the difference (+ slack)."""
    bad = []
    for name, r in ref.items():
        g = got[name]
        se = np.sqrt(r["std"] ** 2 / r["n"] + r["std"] ** 2 / g["n"])
        if not abs(g["mean"] - r["mean"]) <= k * se + slack:
            bad.append(f"{name}: got {g['mean']:.6g} vs reference {r['mean']:.6g} +- {se:.3g} (k={k})")
    return bad
