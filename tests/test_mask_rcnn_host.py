"""Host-side bookkeeping of the detector (rfi_toolbox_amd/models/mask_rcnn.py) that needs no GPU."""
import numpy as np


def test_topk_selection_equals_the_stable_descending_sort():
    from rfi_toolbox_amd.models.mask_rcnn import _topk_desc_stable
    rng = np.random.default_rng(0)
    for m, k in ((4096, 200), (16, 200), (256, 200), (1024, 7), (1, 1)):
        sc = rng.standard_normal((5, m)).astype(np.float32)
        sc[:, ::7] = 0.5                       # ties
        sc[0, :] = 0
        if m > 8:
            sc[1, 3], sc[1, 4], sc[2, 5], sc[2, 6] = -0.0, 0.0, np.inf, -np.inf
        assert np.array_equal(_topk_desc_stable(sc, k), np.argsort(-sc, axis=1, kind="stable")[:, :k]), (m, k)


def test_anchor_grid_matches_the_oracle_grid():
    from oracle.mask_rcnn_ref import level_anchors
    from rfi_toolbox_amd.models.mask_rcnn import _level_anchors
    for h, w, s in ((2, 3, 8), (4, 4, 32), (1, 1, 64)):
        np.testing.assert_allclose(_level_anchors(h, w, s, 2.0 * s), level_anchors(h, w, s, 2.0 * s), rtol=1e-6, atol=1e-5)


def _bare_detector():
    """A MaskRCNN without models, context or buffers: the size checks must fire before any of them is touched."""
    from rfi_toolbox_amd.models.mask_rcnn import MaskRCNN
    return MaskRCNN.__new__(MaskRCNN)


def test_sizes_off_the_64_pixel_grid_raise_value_error():
    import pytest
    det = _bare_detector()
    for h, w in ((100, 128), (128, 96), (0, 128), (192, 200)):
        with pytest.raises(ValueError, match="multiples of 64"):
            det._buffers(2, h, w, 2)
        with pytest.raises(ValueError, match="multiples of 64"):
            det.predict(np.zeros((1, h, w, 3), np.float32))


def test_more_than_65536_anchors_per_image_raise_value_error():
    import pytest
    from rfi_toolbox_amd.models.mask_rcnn import MaskRCNN
    det = _bare_detector()
    for h, w, a in ((448, 448, 66836), (448, 512, 76384), (64, 4096, 87296)):
        with pytest.raises(ValueError, match=f"at most 65536 anchors per image, {h} x {w} has {a}"):
            det._buffers(2, h, w, 2)
    # inside the limit: 384 x 384 (49,104 anchors, the largest square), 512 x 384 (65,472), 64 x 2048 (43,648)
    for h, w in ((384, 384), (512, 384), (64, 2048), (128, 128)):
        MaskRCNN._check_size(h, w, True)
    MaskRCNN._check_size(448, 448, False)       # predict: the host top-k has no anchor limit
