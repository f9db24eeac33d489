"""NumPy restatement of the CASA-style baseline flaggers (include/rfi_hip.h, "CASA-style baseline flaggers"): the robust
piecewise-polynomial fit and TFCrop built on it, RFlag's windowed-rms and spectral-deviation analyses with exact medians,
and the flag extension, every operation in the order the header pins so that the device result can be compared bit for
bit.  Sums run sequentially along the line (vectorised across lines only), masked samples add +0.0.

The algorithms are the published ones (TFCrop and RFlag: the CASA flagdata documentation and Rau & Pramesh Rao's
description of the AIPS tasks they derive from); nothing here is taken from a program, and the reference toolbox has no
statistical flagger of its own."""
import numpy as np

F64 = np.float64
ITERATIONS = 5


# ---------------------------------------------------------------------------------------------- the robust fit
def piece_bounds(L, n):
    """[(first, last + 1)] of the n pieces of a line of L samples; a piece may be empty."""
    return [((p * L) // n, ((p + 1) * L) // n) for p in range(n)]


def shape_of(shape, j, maxnpieces):
    """-> (pieces, degree) of iteration j."""
    if shape == "line" or j == 0:
        return 1, 1
    return min(2 * j + 1, maxnpieces), 3


def _solve4(A, b):
    """The padded 4 x 4 normal equations of every line: elimination by columns without pivoting, back substitution
    with the known terms subtracted in ascending order.  A (n, 4, 4), b (n, 4) -> c (n, 4)."""
    A, b = A.copy(), b.copy()
    with np.errstate(all="ignore"):
        for p in range(4):
            for i in range(p + 1, 4):
                f = A[:, i, p] / A[:, p, p]
                for j in range(p + 1, 4):
                    A[:, i, j] = A[:, i, j] - f * A[:, p, j]
                b[:, i] = b[:, i] - f * b[:, p]
        c = np.zeros_like(b)
        for i in range(3, -1, -1):
            s = b[:, i].copy()
            for j in range(i + 1, 4):
                s = s - A[:, i, j] * c[:, j]
            c[:, i] = s / A[:, i, i]
    return c


def fit_pieces(y, w, pieces, degree):
    """Least-squares fit of every piece over its w-samples -> fit (n, L) float64."""
    y = np.asarray(y, np.float32)
    w = np.asarray(w).astype(bool)
    n, L = y.shape
    fit = np.zeros((n, L), F64)
    yd = y.astype(F64)
    for a, e in piece_bounds(L, pieces):
        m = e - a
        if m == 0:
            continue
        x = np.zeros(m, F64) if m == 1 else (2 * np.arange(m) - (m - 1)).astype(F64) / F64(m - 1)
        x2 = x * x
        x3 = x2 * x
        x4 = x2 * x2
        x5 = x4 * x
        x6 = x3 * x3
        pw = [np.ones(m, F64), x, x2, x3, x4, x5, x6]
        S, B, k = np.zeros((n, 7), F64), np.zeros((n, 4), F64), np.zeros(n, np.int64)
        with np.errstate(all="ignore"):
            for i in range(m):
                wi = w[:, a + i]
                k += wi
                for q in range(7):
                    S[:, q] = S[:, q] + np.where(wi, pw[q][i], F64(0.0))
                for q in range(4):
                    B[:, q] = B[:, q] + np.where(wi, pw[q][i] * yd[:, a + i], F64(0.0))
        d = np.minimum(degree, k - 1)                       # -1 for a piece without a valid sample
        A = np.empty((n, 4, 4), F64)
        for i in range(4):
            for j in range(4):
                inside = (i <= d) & (j <= d)
                A[:, i, j] = np.where(inside, S[:, i + j], F64(1.0) if i == j else F64(0.0))
        rhs = np.where(np.arange(4)[None, :] <= d[:, None], B, F64(0.0))
        c = _solve4(A, rhs)
        with np.errstate(all="ignore"):
            for i in range(m):
                fit[:, a + i] = ((c[:, 3] * x[i] + c[:, 2]) * x[i] + c[:, 1]) * x[i] + c[:, 0]
    return fit


def robust_fit(y, u, shape="line", cutoff=4.0, maxnpieces=7, details=False):
    """The robust fit of the lines y (n, L) float32 with masks u (n, L) -> new flags u & ~w (n, L) bool; with
    ``details`` also the fit of the last iteration that ran, the residuals of it and sigma per iteration."""
    y = np.atleast_2d(np.asarray(y, np.float32))
    u = np.atleast_2d(np.asarray(u).astype(bool))
    n, L = y.shape
    w = u.copy()
    live = np.ones(n, bool)                                 # lines whose iteration goes on
    fit, res = np.zeros((n, L), F64), np.zeros((n, L), F64)
    sigmas = np.full((ITERATIONS, n), np.nan)
    yd = y.astype(F64)
    for j in range(ITERATIONS):
        pieces, degree = shape_of(shape, j, maxnpieces)
        f = fit_pieces(y, w, pieces, degree)
        with np.errstate(all="ignore"):
            r = yd - f
            cnt, s1, s2 = np.zeros(n, np.int64), np.zeros(n, F64), np.zeros(n, F64)
            for i in range(L):
                wi = w[:, i]
                cnt += wi
                s1 = s1 + np.where(wi, r[:, i], F64(0.0))
                s2 = s2 + np.where(wi, r[:, i] * r[:, i], F64(0.0))
            nn = cnt.astype(F64)
            mean = s1 / nn
            var = s2 / nn - mean * mean
            sigma = np.sqrt(np.where(var > 0, var, F64(0.0)))
            sigma = np.where(cnt > 0, sigma, F64(0.0))
            fit[live], res[live] = f[live], r[live]
            live = live & (sigma > 0)
            sigmas[j] = sigma
            keep = np.abs(r) <= F64(cutoff) * sigma[:, None]
        w = np.where(live[:, None], w & keep, w)
    new = u & ~w
    return (new, fit, res, sigmas) if details else new


# ---------------------------------------------------------------------------------------------- TFCrop
def to_plane_values(data):
    a = np.asarray(data)
    if np.iscomplexobj(a):
        with np.errstate(all="ignore"):
            a = np.abs(a)
    with np.errstate(over="ignore"):
        return a.astype(np.float32)


def _chunks(T, ntime):
    ntime = T if ntime is None else int(ntime)
    return [(t0, min(T, t0 + ntime)) for t0 in range(0, T, ntime)]


def tfcrop_chunk(X, F, timecutoff=4.0, freqcutoff=3.0, timefit="line", freqfit="poly", maxnpieces=7,
                 flagdimension="freqtime", divide=True):
    """One chunk: X (C, L) float32 finite, F (C, L) bool -> bool.  ``divide=False`` drops the bandpass division (for the
    test that every stage matters)."""
    C, L = X.shape
    Y = X
    if divide:
        u = ~F
        m, cnt = np.zeros(C, F64), np.zeros(C, np.int64)
        for t in range(L):
            m = m + np.where(u[:, t], X[:, t].astype(F64), F64(0.0))
            cnt += u[:, t]
        with np.errstate(all="ignore"):
            mf = np.where(cnt > 0, m / cnt.astype(F64), F64(0.0)).astype(np.float32)
        _, b, _, _ = robust_fit(mf[None, :], (cnt > 0)[None, :], freqfit, freqcutoff, maxnpieces, details=True)
        b = b[0]
        ok = np.isfinite(b) & (b > 0)
        with np.errstate(all="ignore"):
            Y = np.where(ok[:, None], (X.astype(F64) / b[:, None]).astype(np.float32), X)
    stages = {"freqtime": "tf", "timefreq": "ft", "time": "t", "freq": "f"}[flagdimension]
    for s in stages:
        if s == "t":
            F = F | robust_fit(Y, ~F, timefit, timecutoff, maxnpieces)
        else:
            F = F | robust_fit(Y.T, ~F.T, freqfit, freqcutoff, maxnpieces).T
    return F


def tfcrop_plane(data, prior=None, ntime=None, **kw):
    X = to_plane_values(data)
    F = ~np.isfinite(X)
    if prior is not None:
        F = F | (np.asarray(prior) != 0)
    X = np.where(np.isfinite(X), X, np.float32(0.0)).astype(np.float32)
    out = np.empty(X.shape, bool)
    for t0, t1 in _chunks(X.shape[1], ntime):
        out[:, t0:t1] = tfcrop_chunk(X[:, t0:t1], F[:, t0:t1], **kw)
    return out


def _per_plane(fn, data, prior, per_plane_kw=(), **kw):
    a = np.asarray(data)
    planes = a.reshape((-1,) + a.shape[-2:])
    pr = None if prior is None else np.asarray(prior).reshape(planes.shape)
    out = np.empty(planes.shape, bool)
    for i in range(len(planes)):
        extra = {k: v[i] for k, v in per_plane_kw}
        out[i] = fn(planes[i], None if pr is None else pr[i], **kw, **extra)
    return out.reshape(a.shape)


def tfcrop(data, prior=None, **kw):
    """(..., C, T) -> bool flags of the same shape, plane by plane."""
    return _per_plane(tfcrop_plane, data, prior, **kw)


# ---------------------------------------------------------------------------------------------- RFlag
def window_rms(z, u, winsize):
    """rms_t of the lines z (n, L) complex128 with masks u -> (rms (n, L) float64, has (n, L) bool)."""
    n, L = z.shape
    h = int(winsize) // 2
    re, im = z.real.astype(F64), z.imag.astype(F64)
    rms, has = np.zeros((n, L), F64), np.zeros((n, L), bool)
    with np.errstate(all="ignore"):
        for t in range(L):
            lo, hi = max(0, t - h), min(L - 1, t + h)
            cnt, sr, si = np.zeros(n, np.int64), np.zeros(n, F64), np.zeros(n, F64)
            for k in range(lo, hi + 1):
                cnt += u[:, k]
                sr = sr + np.where(u[:, k], re[:, k], F64(0.0))
                si = si + np.where(u[:, k], im[:, k], F64(0.0))
            nn = cnt.astype(F64)
            mr, mi = sr / nn, si / nn
            vr, vi = np.zeros(n, F64), np.zeros(n, F64)
            for k in range(lo, hi + 1):
                dr, di = re[:, k] - mr, im[:, k] - mi
                vr = vr + np.where(u[:, k], dr * dr, F64(0.0))
                vi = vi + np.where(u[:, k], di * di, F64(0.0))
            v = vr / nn + vi / nn
            has[:, t] = cnt >= 2
            rms[:, t] = np.where(has[:, t], np.sqrt(np.where(v > 0, v, F64(0.0))), F64(0.0))
    return rms, has


def spectral_dev(z, u):
    """Per time sample of z (C, L): (a_re, a_im, d, has)."""
    C, L = z.shape
    re, im = z.real.astype(F64), z.imag.astype(F64)
    with np.errstate(all="ignore"):
        cnt, sr, si = np.zeros(L, np.int64), np.zeros(L, F64), np.zeros(L, F64)
        for c in range(C):
            cnt += u[c]
            sr = sr + np.where(u[c], re[c], F64(0.0))
            si = si + np.where(u[c], im[c], F64(0.0))
        nn = cnt.astype(F64)
        ar, ai = sr / nn, si / nn
        vr, vi = np.zeros(L, F64), np.zeros(L, F64)
        for c in range(C):
            dr, di = re[c] - ar, im[c] - ai
            vr = vr + np.where(u[c], dr * dr, F64(0.0))
            vi = vi + np.where(u[c], di * di, F64(0.0))
        v = vr / nn + vi / nn
        has = cnt >= 2
        d = np.where(has, np.sqrt(np.where(v > 0, v, F64(0.0))), F64(0.0))
    return ar, ai, d, has


def med_plus_mad(v):
    """median + median |v - median| of the float64 values v; inf (nothing can exceed it) for none."""
    if v.size == 0:
        return F64(np.inf)
    med = np.median(v)
    return med + np.median(np.abs(v - med))


def rflag_chunk(z, F, winsize=3, timedevscale=5.0, freqdevscale=5.0, timedev=None, freqdev=None, details=False):
    """One chunk: z (C, L) complex128 (flagged samples may hold anything finite), F (C, L) bool -> bool.
    ``timedev``: None or (C,) values; ``freqdev``: None or one value."""
    C, L = z.shape
    u = ~F
    rms, has = window_rms(z, u, winsize)
    base_t = np.array([med_plus_mad(rms[c][has[c]]) for c in range(C)]) if timedev is None else \
        np.broadcast_to(np.asarray(timedev, F64), (C,))
    thr_t = F64(timedevscale) * base_t
    hit_t = has & (rms > thr_t[:, None])
    ar, ai, d, hasd = spectral_dev(z, u)
    base_f = med_plus_mad(d[hasd]) if freqdev is None else F64(freqdev)
    thr_f = F64(freqdevscale) * base_f
    with np.errstate(all="ignore"):
        dr, di = z.real - ar[None, :], z.imag - ai[None, :]
        dist = np.sqrt(dr * dr + di * di)
    hit_f = u & hasd[None, :] & (dist > thr_f)
    out = F | hit_t | hit_f
    return (out, rms, has, base_t, base_f) if details else out


def rflag_plane(data, prior=None, ntime=None, timedev=None, freqdev=None, **kw):
    z = np.asarray(data).astype(np.complex128)
    F = ~(np.isfinite(z.real) & np.isfinite(z.imag))
    if prior is not None:
        F = F | (np.asarray(prior) != 0)
    z = np.where(F, 0.0, z)
    out = np.empty(z.shape, bool)
    for t0, t1 in _chunks(z.shape[1], ntime):
        out[:, t0:t1] = rflag_chunk(z[:, t0:t1], F[:, t0:t1], timedev=timedev, freqdev=freqdev, **kw)
    return out


def rflag(data, prior=None, timedev=None, freqdev=None, **kw):
    """(..., C, T) -> bool.  ``timedev``: None, a scalar, one value per plane or (planes, C); ``freqdev``: None, a scalar
    or one value per plane."""
    a = np.asarray(data)
    planes, C = int(np.prod(a.shape[:-2], dtype=np.int64)), a.shape[-2]
    per = []
    if timedev is not None:
        td = np.asarray(timedev, F64)
        td = td.reshape(-1, 1) if td.size in (1, planes) and td.size != planes * C else td.reshape(planes, C)
        per.append(("timedev", np.broadcast_to(td, (planes, C))))
    if freqdev is not None:
        per.append(("freqdev", np.broadcast_to(np.asarray(freqdev, F64).reshape(-1), (planes,))))
    return _per_plane(rflag_plane, a, prior, per_plane_kw=per, **kw)


# ---------------------------------------------------------------------------------------------- extend
def extend_chunk(F, growtime=50.0, growfreq=50.0, growaround=False, flagneartime=False, flagnearfreq=False):
    F = np.asarray(F).astype(bool)
    C, L = F.shape
    if growaround:
        p = np.zeros((C + 2, L + 2), np.int64)
        p[1:-1, 1:-1] = F
        nb = sum(p[1 + dc:1 + dc + C, 1 + dt:1 + dt + L] for dc in (-1, 0, 1) for dt in (-1, 0, 1) if (dc, dt) != (0, 0))
        F = F | (nb > 4)
    if growtime < 100.0:
        cnt = F.sum(axis=1)
        F = F | ((100 * cnt).astype(F64) > F64(growtime) * F64(L))[:, None]
    if growfreq < 100.0:
        cnt = F.sum(axis=0)
        F = F | ((100 * cnt).astype(F64) > F64(growfreq) * F64(C))[None, :]
    if flagneartime:
        G = F.copy()
        G[:, 1:] |= F[:, :-1]
        G[:, :-1] |= F[:, 1:]
        F = G
    if flagnearfreq:
        G = F.copy()
        G[1:] |= F[:-1]
        G[:-1] |= F[1:]
        F = G
    return F


def extend_plane(F, prior=None, ntime=None, **kw):
    F = np.asarray(F) != 0
    out = np.empty(F.shape, bool)
    for t0, t1 in _chunks(F.shape[1], ntime):
        out[:, t0:t1] = extend_chunk(F[:, t0:t1], **kw)
    return out


def extend(flags, **kw):
    return _per_plane(extend_plane, np.asarray(flags) != 0, None, **kw)
