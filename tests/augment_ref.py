"""NumPy float64 restatement of the training augmentation (include/rfi_hip.h, "training augmentation"): the parameter
draw, the composed inverse map, the bilinear / nearest warp with reflect-101 borders, and the pixels at which the
nearest-neighbour choice is a tie (so that a test can leave them out of a byte comparison)."""
import numpy as np

from oracle.synth_ref import philox4x32_10

DEFAULTS = dict(p_hflip=0.5, p_vflip=0.5, p_rotate=0.5, rotate_limit=15, p_ssr=0.5, shift_limit=0.05, scale_limit=0.05,
                ssr_rotate_limit=10)
RAD = 0.017453292519943295


def uniforms(seed, call, n):
    """u (n, 12): three Philox blocks per sample, counter (i, call_lo, call_hi, k), key (seed_lo, seed_hi)."""
    i = np.arange(n, dtype=np.uint64)
    lo, hi = call & 0xFFFFFFFF, (call >> 32) & 0xFFFFFFFF
    words = []
    for k in range(3):
        words += philox4x32_10(i, np.full(n, lo, np.uint64), np.full(n, hi, np.uint64), np.full(n, k, np.uint64),
                               seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return (np.stack(words, axis=1).astype(np.float64) + 0.5) * 2.0 ** -32


def draw(n, h, w, seed=0, call=0, **cfg):
    """dict of per-sample arrays: gates (n, 4) int32, theta1, theta2 (degrees), s, dx, dy, inv (n, 6).  The
    probabilities and limits are rounded to float32 first, as the C structure holds them."""
    c = {k: np.float64(np.float32(v)) for k, v in {**DEFAULTS, **cfg}.items()}
    u = uniforms(seed, call, n)
    gh, gv, gr, gs = u[:, 0] < c["p_hflip"], u[:, 1] < c["p_vflip"], u[:, 2] < c["p_rotate"], u[:, 3] < c["p_ssr"]
    th1 = np.where(gr, (2.0 * u[:, 4] - 1.0) * c["rotate_limit"], 0.0)
    th2 = np.where(gs, (2.0 * u[:, 5] - 1.0) * c["ssr_rotate_limit"], 0.0)
    s = np.where(gs, 1.0 + (2.0 * u[:, 6] - 1.0) * c["scale_limit"], 1.0)
    dx = np.where(gs, (2.0 * u[:, 7] - 1.0) * c["shift_limit"] * float(w), 0.0)
    dy = np.where(gs, (2.0 * u[:, 8] - 1.0) * c["shift_limit"] * float(h), 0.0)
    a1, a2 = th1 * RAD, th2 * RAD
    c1, s1 = np.where(gr, np.cos(a1), 1.0), np.where(gr, np.sin(a1), 0.0)
    c2, s2 = np.where(gs, np.cos(a2), 1.0), np.where(gs, np.sin(a2), 0.0)
    pc, ps = c1 * c2 - s1 * s2, c1 * s2 + s1 * c2                      # R(-a1) R(-a2) = [pc ps; -ps pc]
    fh, fv = np.where(gh, -1.0, 1.0), np.where(gv, -1.0, 1.0)
    cx, cy = (float(w) - 1.0) * 0.5, (float(h) - 1.0) * 0.5
    inv = np.empty((n, 6))
    inv[:, 0], inv[:, 1] = fh * pc / s, fh * ps / s
    inv[:, 3], inv[:, 4] = fv * -ps / s, fv * pc / s
    inv[:, 2] = cx - (inv[:, 0] * (cx + dx) + inv[:, 1] * (cy + dy))
    inv[:, 5] = cy - (inv[:, 3] * (cx + dx) + inv[:, 4] * (cy + dy))
    return dict(gates=np.stack([gh, gv, gr, gs], axis=1).astype(np.int32), theta1=th1, theta2=th2, s=s, dx=dx, dy=dy, inv=inv)


def forward_inverse(p, h, w):
    """inv (n, 6) the long way round: build M = SSR R(theta1) Fv Fh as 3 x 3 matrices and invert it (a check of `draw`)."""
    n = len(p["s"])
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    out = np.empty((n, 6))
    for i in range(n):
        gh, gv, _, _ = p["gates"][i]
        a1, a2, s = p["theta1"][i] * RAD, p["theta2"][i] * RAD, p["s"][i]
        ssr = np.array([[s * np.cos(a2), -s * np.sin(a2), p["dx"][i]], [s * np.sin(a2), s * np.cos(a2), p["dy"][i]], [0, 0, 1.0]])
        rot = np.array([[np.cos(a1), -np.sin(a1), 0], [np.sin(a1), np.cos(a1), 0], [0, 0, 1.0]])
        flip = np.diag([-1.0 if gh else 1.0, -1.0 if gv else 1.0, 1.0])
        to_c = np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1.0]])
        from_c = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1.0]])
        out[i] = (from_c @ np.linalg.inv(ssr @ rot @ flip) @ to_c)[:2].ravel()
    return out


def reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.abs(i) % p
    return np.where(i >= n, p - i, i)


def source_positions(inv, h, w):
    """(sx, sy), each (h, w) float64, of one sample's output pixels"""
    yo, xo = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return inv[0] * xo + inv[1] * yo + inv[2], inv[3] * xo + inv[4] * yo + inv[5]


def warp(x, y, p):
    """(x_out float32, y_out uint8, ties bool (n, h, w)) of x (n, h, w, c) float32 and y (n, h, w) uint8 under the
    parameters `p` of draw().  ties: sx + 0.5 or sy + 0.5 within 1e-9 of an integer (never in a flip-only sample)."""
    n, h, w, _ = x.shape
    xo, yo, ties = np.empty_like(x), np.empty_like(y), np.zeros(y.shape, bool)
    for i in range(n):
        gh, gv, gr, gs = p["gates"][i]
        if not gr and not gs:
            xo[i] = x[i][::-1 if gv else 1, ::-1 if gh else 1]
            yo[i] = y[i][::-1 if gv else 1, ::-1 if gh else 1]
            continue
        sx, sy = source_positions(p["inv"][i], h, w)
        x0, y0 = np.floor(sx), np.floor(sy)
        tx, ty = (sx - x0)[..., None], (sy - y0)[..., None]
        xa, xb = reflect101(x0.astype(np.int64), w), reflect101(x0.astype(np.int64) + 1, w)
        ya, yb = reflect101(y0.astype(np.int64), h), reflect101(y0.astype(np.int64) + 1, h)
        v = x[i].astype(np.float64)
        acc = ((1.0 - tx) * (1.0 - ty) * v[ya, xa] + tx * (1.0 - ty) * v[ya, xb]) + (1.0 - tx) * ty * v[yb, xa]
        xo[i] = (acc + tx * ty * v[yb, xb]).astype(np.float32)
        mx, my = np.floor(sx + 0.5), np.floor(sy + 0.5)
        yo[i] = y[i][reflect101(my.astype(np.int64), h), reflect101(mx.astype(np.int64), w)]
        ties[i] = (np.abs(sx + 0.5 - np.round(sx + 0.5)) < 1e-9) | (np.abs(sy + 0.5 - np.round(sy + 0.5)) < 1e-9)
    return xo, yo, ties


def inputs(shape, seed=1):
    """the test data: x normal x 2 float32; y Bernoulli(0.3) with a few bytes set to 2 and 255"""
    n, h, w, c = shape
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 2.0).astype(np.float32)
    y = (rng.random((n, h, w)) < 0.3).astype(np.uint8)
    flat = y.reshape(-1)
    idx = rng.choice(flat.size, size=min(6, flat.size), replace=False)
    flat[idx[::2]], flat[idx[1::2]] = 2, 255
    return x, y
