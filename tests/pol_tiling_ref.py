"""NumPy restatement of the 8-channel tiling (include/rfi_hip.h, rfi_norm_gather), written from the rules:

* a sample is 4 complex planes RR, RL, LR, LL of C x T; its 8 channels are RR.re, RR.im, RL.re, ... LL.im;
* every channel value is float32((float64(x) - centre) / scale), or 0 when scale is 0 (normalize_ref.apply), with the
  sample's own (centre, scale) pair;
* the tiles are stitch_ref's: patch_table order, view_of views, and a pixel past a view's edge is the visibility
  0 + 0j normalised like every other, i.e. float32((0 - centre) / scale), or 0 when scale is 0;
* output (N, ps, ps, 8) float32, channels last.
"""
import numpy as np

import normalize_ref as nref
import stitch_ref as sref


def pad_value(pair):
    """What a pixel past the view's edge holds under `pair` = (centre, scale) or None (the all-zeros transform)."""
    if pair is None or pair[1] == 0:
        return np.float32(0.0)
    return np.float32((0.0 - pair[0]) / pair[1])


def as_samples(data):
    data = np.asarray(data)
    return data if data.ndim == 4 else data[None]


def cut_channels(norm_nchw, pairs, ps, stride=None, views=1, edge="pad"):
    """The tiles of already normalised planes: (n, 8, C, T) float32 -> (N, ps, ps, 8), padding from the sample's pair."""
    norm_nchw = np.asarray(norm_nchw)
    n, k, C, T = norm_nchw.shape
    assert k == 8 and len(pairs) == n
    table = sref.patch_table(n, C, T, ps, stride, views, edge)
    out = np.empty((len(table), ps, ps, 8), dtype=np.float32)
    for e, (p, v, r0, c0) in enumerate(table):
        out[e] = pad_value(pairs[p])
        blk = sref.view_of(norm_nchw[p], v)[:, r0:r0 + ps, c0:c0 + ps]
        out[e, :blk.shape[1], :blk.shape[2], :] = blk.transpose(1, 2, 0)
    return out


def normalise(data, pairs):
    """(n, 8, C, T) float32 of complex (n, 4, C, T) `data`, sample i by pairs[i]."""
    x = nref.to_nchw(as_samples(data))
    return np.stack([nref.apply(s, p) for s, p in zip(x, pairs)])


def tile(data, pairs, ps, stride=None, views=1, edge="pad"):
    """The network input of every tile of complex (n, 4, C, T) or (4, C, T) `data`."""
    return cut_channels(normalise(data, pairs), pairs, ps, stride, views, edge)


def pairs_of(data, method, scope):
    """One (centre, scale) pair or None (all zeros) per sample, as a Normalizer(method, scope) fitted on `data` has it."""
    x = nref.to_nchw(as_samples(data))
    if method is None:
        return [(0.0, 1.0)] * len(x)
    if scope == "dataset":
        return [nref.dataset_params([x], method)[1]] * len(x)
    return [nref.sample_params(s, method) for s in x]


def broadcast(flags, n_pol=4):
    """(B, C, T) or (C, T) baseline flags -> (B, 4, C, T) or (4, C, T)."""
    flags = np.asarray(flags)
    return np.repeat(np.expand_dims(flags, -3), n_pol, axis=-3)
