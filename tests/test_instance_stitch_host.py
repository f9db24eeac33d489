"""CPU-only: the rules of the instance stitch give the truth events of the 96 x 80 scene at every tiling (shown with the NumPy
restatement alone), the case table reaches what it claims, and every argument check of ``stitch_instances`` and
``detect_observation`` raises before a device call."""
import itertools

import numpy as np
import pytest

import instance_stitch_cases as cases


@pytest.mark.parametrize("ps,s", cases.SCENE_TILINGS)
def test_scene_gives_the_truth_events(ps, s):
    truth = cases.scene()
    for views, edge, conn in itertools.product((1, 2, 4), ("pad", "shift"), (4, 8)):
        out = cases.run_ref(cases.scene_case(ps, s, views, edge, conn))
        what = (ps, s, views, edge, conn)
        assert out["counts"][0] == len(truth), what
        for k, (label, score, mask) in enumerate(truth):             # (the scene lists its events by descending score)
            assert out["labels"][0, k] == label and out["scores"][0, k] == np.float32(score), what
            assert np.array_equal(out["masks"][0, k].astype(bool), mask), what
            ys, xs = np.nonzero(mask)
            assert out["boxes"][0, k].tolist() == [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1], what
        assert np.array_equal(out["rfi_mask"][0].astype(bool), np.any([m for _, _, m in truth], axis=0)), what


@pytest.fixture(scope="module")
def table():
    t = cases.table()
    stats = {}
    for name, c in t.items():
        stats[name] = {}
        c["want"] = cases.run_ref(c, stats[name])
    return t, stats


def test_table_holds_what_it_claims(table):
    t, st = table
    # both link branches
    assert st["scene_s32"]["adjacent"] > 0 and st["scene_s32"]["shared"] == 0
    assert st["scene_s16_v2"]["shared"] > 0 and st["aligned_d256"]["shared"] > 0 and st["aligned_d256"]["adjacent"] == 0
    # a chain of at least four tiles whose ends are joined only through the tiles between them
    assert any(len(e["tiles"]) >= 4 and not e["complete"] for e in st["scene_s24_pad"]["events"])
    # a detection that lies only in padding, a low score, a small area
    e = st["edges_d130"]
    assert e["padding_only"] == 1 and e["drop_score"] == 129 and e["drop_area"] == 3
    # a score tie between two events: the smaller id first
    w = t["edges_d130"]["want"]
    assert w["scores"][0, 0] == w["scores"][0, 1] == np.float32(0.8) and w["labels"][0, :2].tolist() == [2, 3]
    # a capped plane whose flags hold the cut events too, and a plane without detections
    assert e["n_events"] == [5, 0] and w["counts"].tolist() == [3, 0]
    assert (w["rfi_mask"][0] > w["masks"][0].any(0)).any() and not w["rfi_mask"][1].any()
    # slot 129 of the full tile is half of an event that crosses the seam
    assert w["scores"][0, 2] == np.float32(0.6) and w["masks"][0, 2, 29, 31] and w["masks"][0, 2, 29, 32]
    # class_aware both ways: without it the crossing lines of the scene merge
    assert t["scene_s24_v4_shift_c4_any"]["class_aware"] is False and t["scene_s24_v4_shift_c4_any"]["want"]["counts"][0] < 7
    # the connectivities where they differ
    assert t["seam_c8"]["want"]["counts"][0] == 1 and t["seam_c4"]["want"]["counts"][0] == 2
    assert st["seam_c8"]["adjacent"] == 1 and st["seam_c4"]["adjacent"] == 0
    # views, edges, D
    assert {c["views"] for c in t.values()} == {1, 2, 4} and {c["edge"] for c in t.values()} == {"pad", "shift"}
    assert {1, 64, 65, 130, 256} <= {c["det"]["scores"].shape[1] for c in t.values()}
    assert {c["connectivity"] for c in t.values()} == {4, 8}
    # planes of at most 96 x 80 in 32-tiles, and the one 64 x 64 plane in a 64-tile
    assert all((c["ps"] == 32 and c["C"] <= 96 and c["T"] <= 80) or (c["ps"], c["C"], c["T"]) == (64, 64, 64) for c in t.values())


def test_random_cases_are_not_trivial():
    for seed, D, planes in cases.RANDOM_CASES:
        c = cases.random_case(seed, D, planes)
        stats = {}
        out = cases.run_ref(c, stats)
        assert c["det"]["scores"].shape[1] == D and len(out["counts"]) == planes
        assert stats["shared"] + stats["adjacent"] > 0 and out["rfi_mask"].any()


def _tiles(n=6, D=2, ps=32):
    return {"boxes": np.zeros((n, D, 4), np.float32), "scores": np.zeros((n, D), np.float32), "labels": np.zeros((n, D), np.int32),
            "counts": np.zeros((n,), np.int32), "masks": np.zeros((n, D, ps, ps), np.uint8)}


@pytest.mark.parametrize("kw", [dict(patch_size=0), dict(stride=33), dict(views=3), dict(edge="wrap"), dict(max_events=0),
                                dict(max_events=257), dict(min_area=0), dict(min_score=float("nan")), dict(connectivity=6),
                                dict(out="gpu"), dict(channels=0), dict(times=-1), dict(channels=97),        # 12 tiles a plane: not 6
                                dict(patch_size=16)])                                                        # tiles of 32 x 32
def test_stitch_instances_argument_checks(kw):
    from rfi_toolbox_amd.inference import stitch_instances
    args = dict(channels=96, times=64, patch_size=32)
    args.update(kw)
    with pytest.raises(ValueError):
        stitch_instances(_tiles(), **args)


def test_stitch_instances_detection_checks():
    from rfi_toolbox_amd.inference import stitch_instances
    d = _tiles()
    del d["masks"]
    with pytest.raises(ValueError):
        stitch_instances(d, 96, 64, 32)
    d = _tiles()
    d["scores"] = d["scores"][:, :1]
    with pytest.raises(ValueError):
        stitch_instances(d, 96, 64, 32)
    with pytest.raises(ValueError):
        stitch_instances([{"boxes": np.zeros((1, 4)), "labels": [1], "scores": [0.5]}] * 6, 96, 64, 32)      # no masks
    with pytest.raises(ValueError):
        stitch_instances("tiles", 96, 64, 32)
    with pytest.raises(ValueError, match="65536"):
        stitch_instances(_tiles(1, 256), 2048, 2048, 32)                 # 4096 tiles a plane x 256 slots


@pytest.mark.parametrize("kw", [dict(patch_size=-1), dict(stride=200), dict(views=0), dict(edge=None), dict(max_events=1000),
                                dict(min_area=0), dict(connectivity=0), dict(out="torch"), dict(batch_size=0),
                                dict(min_score=float("inf"))])
def test_detect_observation_argument_checks(kw):
    from rfi_toolbox_amd.inference import detect_observation
    with pytest.raises(ValueError):
        detect_observation(None, np.zeros((4, 128, 128), np.complex64), **kw)


def test_public_names():
    import rfi_toolbox_amd
    from rfi_toolbox_amd import inference
    assert rfi_toolbox_amd.stitch_instances is inference.stitch_instances
    assert rfi_toolbox_amd.detect_observation is inference.detect_observation
    assert {"stitch_instances", "detect_observation"} <= set(inference.__all__)
