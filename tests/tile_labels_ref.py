"""NumPy restatement of the label tiling (include/rfi_hip.h, rfi_label_gather), written from the rules on top of
stitch_ref.patch_table / cut:

* labels (n, C, T) bytes; a pixel is invalid where the (n, C, T) map is non-zero, or where any / all of the four
  polarisations of the (n, 4, C, T) map are; an invalid pixel's byte gets bit 7;
* the tiles are stitch_ref's (patch_table order, view_of views), and a pixel past a view's edge holds `pad_value`.
"""
import numpy as np

import stitch_ref as sref


def merge(labels, invalid=None, rule="any"):
    """(n, C, T) uint8: labels | 0x80 where invalid"""
    lab = np.asarray(labels).astype(np.uint8)
    if invalid is None:
        return lab
    inv = np.asarray(invalid) != 0
    if inv.ndim == lab.ndim + 1:
        inv = inv.any(axis=1) if rule == "any" else inv.all(axis=1)
    assert inv.shape == lab.shape
    return lab | (inv.astype(np.uint8) << 7).astype(np.uint8)


def tile(labels, ps, stride=None, views=1, edge="pad", invalid=None, rule="any", pad_value=0x80):
    """(N, ps, ps) uint8 in patch_table order"""
    lab = merge(labels, invalid, rule)
    n, C, T = lab.shape
    table = sref.patch_table(n, C, T, ps, stride, views, edge)
    # cut() pads with zeros: cut the bytes and a plane of ones, and put pad_value where the ones did not reach
    out = sref.cut(lab, table, ps)
    inside = sref.cut(np.ones_like(lab), table, ps) != 0
    return np.where(inside, out, np.uint8(pad_value)).astype(np.uint8)
