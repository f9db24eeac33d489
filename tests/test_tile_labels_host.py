"""No GPU: the NumPy restatement of rfi_label_gather (tests/tile_labels_ref.py) on hand-made planes, the ignore-bit helpers
of rfi_toolbox_amd.class_labels, and tile_labels' argument checks that touch no device."""
import numpy as np
import pytest

import stitch_ref as sref
import tile_labels_ref as T
from rfi_toolbox_amd.class_labels import IGNORE, pack_class_masks, split_ignore, with_ignore


def test_hand_made_plane():
    lab = np.arange(1, 13, dtype=np.uint8).reshape(1, 3, 4)          # C = 3, T = 4
    out = T.tile(lab, 2)                                               # origins rows 0, 2 and columns 0, 2
    assert out.shape == (4, 2, 2)
    assert out[0].tolist() == [[1, 2], [5, 6]] and out[1].tolist() == [[3, 4], [7, 8]]
    assert out[2].tolist() == [[9, 10], [0x80, 0x80]] and out[3].tolist() == [[11, 12], [0x80, 0x80]]
    assert T.tile(lab, 2, pad_value=0)[3].tolist() == [[11, 12], [0, 0]]
    assert T.tile(lab, 2, edge="shift")[2].tolist() == [[5, 6], [9, 10]]          # the last origin moves: no padding
    assert not (T.tile(lab, 2, edge="shift") & 0x80).any()
    v = T.tile(lab, 4, views=4)                                        # one tile per view, the plane padded to 4 x 4
    assert v.shape == (4, 4, 4)
    assert v[0, :3].tolist() == lab[0].tolist() and (v[0, 3] == 0x80).all()
    assert v[1, :3].tolist() == lab[0, ::-1].tolist()
    assert v[2].tolist() == [[1, 5, 9, 0x80], [2, 6, 10, 0x80], [3, 7, 11, 0x80], [4, 8, 12, 0x80]]
    assert v[3, :, :3].tolist() == lab[0].T[::-1].tolist()


def test_invalid_rules():
    lab = np.zeros((2, 3, 4), np.uint8)
    lab[1, 1, 2] = 5
    pol = np.zeros((2, 4, 3, 4), np.uint8)
    pol[0, 1, 0, 0] = 1                      # one polarisation: any, not all
    pol[1, :, 1, 2] = 7                      # all four (non-zero is invalid, whatever the value)
    any_, all_ = T.merge(lab, pol, "any"), T.merge(lab, pol, "all")
    assert any_[0, 0, 0] == 0x80 and all_[0, 0, 0] == 0
    assert any_[1, 1, 2] == all_[1, 1, 2] == 0x85
    assert int(((any_ & 0x80) != 0).sum()) == 2 and int(((all_ & 0x80) != 0).sum()) == 1
    base = pol.any(axis=1)
    assert np.array_equal(T.merge(lab, base), any_)
    assert np.array_equal(T.tile(lab, 2, invalid=pol, rule="any", pad_value=0) & 0x7F, T.tile(lab, 2, pad_value=0))
    # the order is patch_table's: plane, view, tile row, tile column
    table = sref.patch_table(2, 3, 4, 2, None, 2)
    assert len(T.tile(lab, 2, views=2)) == len(table) == 2 * 2 * 2 * 2


def test_with_ignore_round_trip():
    rng = np.random.default_rng(0)
    masks = rng.random((2, 7, 9, 11)) < 0.3
    bits = pack_class_masks(masks)
    ign = rng.random((2, 9, 11)) < 0.25
    y = with_ignore(bits, ign)
    assert y.dtype == np.uint8 and IGNORE == 0x80
    low, got = split_ignore(y)
    assert np.array_equal(low, bits) and np.array_equal(got, ign)
    assert np.array_equal(with_ignore(bits != 0, ign) & 0x7F, (bits != 0).astype(np.uint8))      # a bool map
    assert np.array_equal(with_ignore(bits, True), bits | 0x80) and np.array_equal(with_ignore(bits, 0), bits)
    with pytest.raises(ValueError):
        with_ignore(pack_class_masks(rng.random((8, 4, 4)) < 2), False)       # 8 classes use bit 7
    with pytest.raises(ValueError):
        with_ignore(bits.astype(np.int32), ign)
    with pytest.raises(ValueError):
        split_ignore(bits.astype(np.int16))
    # the restatement's bit 7 is with_ignore's
    assert np.array_equal(T.merge(bits, ign), y)


def test_tile_labels_argument_checks():
    from rfi_toolbox_amd.inference import tile_labels
    lab = np.zeros((2, 6, 8), np.uint8)
    with pytest.raises(ValueError, match="invalid_rule"):
        tile_labels(lab, 4, invalid_rule="some")
    with pytest.raises(ValueError, match="pad must be"):
        tile_labels(lab, 4, pad="one")
    with pytest.raises(TypeError, match="labels must be uint8 or bool"):
        tile_labels(lab.astype(np.float32), 4)
    with pytest.raises(ValueError, match="labels must be"):
        tile_labels(np.zeros(8, np.uint8), 4)
    with pytest.raises(ValueError, match="per polarisation"):
        tile_labels(lab, 4, invalid=np.zeros((2, 3, 6, 8), np.uint8))
    with pytest.raises(TypeError, match="invalid must be"):
        tile_labels(lab, 4, invalid=np.zeros((2, 6, 8), np.float32))
    with pytest.raises(ValueError, match="stride"):
        tile_labels(lab, 4, stride=5)
