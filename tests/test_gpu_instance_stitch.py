"""-m gpu: the instance stitch on the GPU (csrc/instance_stitch.hip, rfi_toolbox_amd/inference.py stitch_instances and
detect_observation) against the NumPy restatement tests/instance_stitch_ref.py.  Minima, maxima, ORs and a sort on a total
order: every comparison is exact."""
import numpy as np
import pytest

import instance_stitch_cases as cases
import instance_stitch_ref as ref

pytestmark = pytest.mark.gpu

KEYS = ("boxes", "scores", "labels", "counts", "rfi_mask", "masks")
DETECTOR_SEED = 1        # untrained mask logits lie near 0: under this seed every end-to-end case has events (seeds 0, 2, 3: none at all
                         # with the dataset-scope normalizer), [32, 32], [32, 23] and [32, 32] per plane at max_events = 32


def _ctx():
    from rfi_toolbox_amd.runtime import Context
    return Context.get(0)


def _stitch(case, det=None, **over):
    from rfi_toolbox_amd.inference import stitch_instances
    kw = {k: case[k] for k in cases.DEFAULTS}
    kw.update(over)
    return stitch_instances(case["det"] if det is None else det, case["C"], case["T"], case["ps"], **kw)


def _host(res):
    return {k: v.numpy() for k, v in res.items()}


def _same(got, want, what, keys=KEYS):
    for k in keys:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert g.tobytes() == w.tobytes(), (what, k, np.argwhere(g != w)[:5].tolist())


@pytest.fixture(scope="module")
def table():
    t = cases.table()
    for c in t.values():
        c["want"] = cases.run_ref(c)
    return t


@pytest.mark.parametrize("name", sorted(cases.table()))
def test_table_equals_the_restatement(table, name):
    c = table[name]
    ctx = _ctx()
    dev = {k: ctx.to_device(v) for k, v in c["det"].items()}          # the device dict, used in place
    got = _host(_stitch(c, dev))
    _same(got, c["want"], name)
    again = _host(_stitch(c, dev))                                    # two calls: identical bytes
    _same(again, got, name)
    lean = _stitch(c, dev, instance_masks=False)                      # no instance masks: the rest unchanged, none written
    assert "masks" not in lean
    _same(_host(lean), got, name, KEYS[:5])
    from_host = _host(_stitch(c))                                     # NumPy arrays are uploaded
    _same(from_host, got, name)
    E = c["max_events"]
    for p in range(len(got["counts"])):                               # everything is zero behind the counts
        k = int(got["counts"][p])
        assert not got["boxes"][p, k:].any() and not got["scores"][p, k:].any() and not got["labels"][p, k:].any()
        assert not got["masks"][p, k:].any() and set(np.unique(got["masks"][p])) <= {0, 1}
        if k < E:                                                     # an uncapped plane: the masks add up to the flags
            assert np.array_equal(got["masks"][p].any(0), got["rfi_mask"][p].astype(bool)), (name, p)


@pytest.mark.parametrize("seed,D,planes", cases.RANDOM_CASES)
def test_random_cases_equal_the_restatement(seed, D, planes):
    c = cases.random_case(seed, D, planes)
    _same(_host(_stitch(c)), cases.run_ref(c), (seed, D, planes))


def test_flags_do_not_depend_on_the_cap(table):
    c = table["scene_s24_pad"]
    full, capped = _host(_stitch(c)), _host(_stitch(c, max_events=2))
    assert full["counts"][0] == 7 and capped["counts"][0] == 2
    assert np.array_equal(full["rfi_mask"], capped["rfi_mask"])
    _same({k: v[:, :2] for k, v in full.items() if k not in ("counts", "rfi_mask")},
          {k: v for k, v in capped.items() if k not in ("counts", "rfi_mask")}, "cap", ("boxes", "scores", "labels", "masks"))


def test_one_tile_is_the_identity():
    """One tile that is the whole plane: the arrays of detect(out="device") come back unchanged."""
    rng = np.random.default_rng(3)
    n, D, ps = 3, 9, 64
    det = {"boxes": np.zeros((n, D, 4), np.float32), "scores": np.zeros((n, D), np.float32), "labels": np.zeros((n, D), np.int32),
           "counts": np.array([9, 0, 4], np.int32), "masks": np.zeros((n, D, ps, ps), np.uint8)}
    for i in range(n):
        k = int(det["counts"][i])
        det["scores"][i, :k] = np.sort(rng.random(k).astype(np.float32))[::-1]
        det["labels"][i, :k] = rng.integers(1, 6, k)
        for j in range(k):
            x1, y1 = rng.uniform(0, 40, 2)
            det["boxes"][i, j] = (x1, y1, x1 + rng.uniform(1, 24), y1 + rng.uniform(1, 24))
            det["masks"][i, j, int(y1):int(y1) + 5, int(x1):int(x1) + 7] = 1       # overlapping masks of one tile stay apart
    from rfi_toolbox_amd.inference import stitch_instances
    got = _host(stitch_instances(det, ps, ps, ps, max_events=D))
    _same(got, det, "identity", ("boxes", "scores", "labels", "counts", "masks"))
    assert np.array_equal(got["rfi_mask"], det["masks"].any(1).astype(np.uint8))


def _scene_targets():
    out = {"boxes": [], "labels": [], "masks": []}
    for label, _, mask in cases.scene():
        ys, xs = np.nonzero(mask)
        out["boxes"].append((xs.min(), ys.min(), xs.max() + 1, ys.max() + 1))
        out["labels"].append(label)
        out["masks"].append(mask)
    return [{"boxes": np.asarray(out["boxes"], np.float32), "labels": np.asarray(out["labels"]), "masks": np.stack(out["masks"])}]


def test_stitched_detections_score_as_the_emitters(table):
    """Perfect per-tile detections of the scene: stitched they are the emitters (AP = AR = 1); tile by tile they are pieces."""
    from rfi_toolbox_amd.evaluation.detection import score_detections
    c = table["scene_s24_pad"]
    targets = _scene_targets()
    s = score_detections(_stitch(c), targets, num_classes=6)
    assert s["AP"] == 1.0 and s["AR"] == 1.0
    host = _stitch(c, out="host")                                     # the list form scores the same
    assert len(host) == 1 and host[0]["masks"].dtype == bool and host[0]["labels"].dtype == np.int64
    s = score_detections(host, targets, num_classes=6)
    assert s["AP"] == 1.0 and s["AR"] == 1.0
    # the same detections unstitched: every tile's pieces pasted into the plane and scored against it
    C, T, ps, d = c["C"], c["T"], c["ps"], c["det"]
    tiles = ref.tile_table(C, T, ps, c["stride"], c["views"], c["edge"])
    pieces = {"boxes": [], "scores": [], "labels": [], "masks": []}
    for i, (v, r0, c0) in enumerate(tiles):
        for j in range(int(d["counts"][i])):
            pieces["boxes"].append(ref.map_box(d["boxes"][i, j], v, r0, c0, C, T))
            pieces["scores"].append(d["scores"][i, j])
            pieces["labels"].append(d["labels"][i, j])
            pieces["masks"].append(ref.to_plane(d["masks"][i, j], v, r0, c0, C, T))
    s = score_detections([{k: np.asarray(v) for k, v in pieces.items()}], targets, num_classes=6)
    assert s["AP"] < 0.5 and s["AR"] < 0.5


# ---------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def detector():
    import torch
    from rfi_toolbox_amd.models import MaskRCNN
    torch.manual_seed(DETECTOR_SEED)     # the weights are drawn from torch's generator; `seed` is the samplers'
    det = MaskRCNN(6, 8, 16, 64, 128, seed=7)
    det.score_thresh = 0.0           # untrained: keep every box, so that detections exist
    det.max_det = 6                  # (keeps the restatement's loop over pairs of members short)
    return det


@pytest.fixture(scope="module")
def observation():
    from rfi_toolbox_amd.core import RFISimulator
    data = RFISimulator(128, 192, seed=4, device="cuda:0").generate_batch(2, out="complex64").data
    return data.numpy() if hasattr(data, "ptr") else data.cpu().numpy()


def _normalizer(form, data):
    from rfi_toolbox_amd.preprocessing import Normalizer
    if form == "dataset":
        return Normalizer("standardize", "dataset").fit(data)
    return Normalizer("robust_scale", "sample")


@pytest.mark.parametrize("stride,form,bs", [(64, "sample", 4), (48, "dataset", 4), (48, "sample", 5)])
def test_detect_observation_end_to_end(detector, observation, stride, form, bs):
    """detect_observation = tile_observation -> detect per batch -> stitch_instances, and = the restatement on the downloaded
    per-tile detections; both output forms agree.  12 and 24 tiles: batches of 4 come out even, batches of 5 end in a padded one."""
    from rfi_toolbox_amd.inference import detect_observation, stitch_instances, tile_observation, tiling_count
    from rfi_toolbox_amd.runtime import DeviceArray
    data, ps = observation, 64
    assert data.shape == (2, 4, 128, 192)
    nz = _normalizer(form, data)
    kw = dict(max_events=32, min_area=2, min_score=0.0, class_aware=True, connectivity=8)
    got = detect_observation(detector, data, ps, stride, views=1, normalizer=nz, batch_size=bs, instance_masks=True, out="device", **kw)
    got = _host(got)
    # by hand
    x = tile_observation(data, ps, stride, 1, normalizer=nz)
    N = x.shape[0]
    assert N == 2 * tiling_count(128, 192, ps, stride) and (N % bs != 0) == (bs == 5)
    xh = x.numpy()
    D = detector.max_det
    tiles = {"boxes": np.zeros((N, D, 4), np.float32), "scores": np.zeros((N, D), np.float32), "labels": np.zeros((N, D), np.int32),
             "counts": np.zeros((N,), np.int32), "masks": np.zeros((N, D, ps, ps), np.uint8)}
    ctx = detector.backbone.ctx
    for i0 in range(0, N, bs):
        k = min(bs, N - i0)
        batch = np.zeros((bs, ps, ps, 8), np.float32)
        batch[:k] = xh[i0:i0 + k]
        d = detector.detect(ctx.to_device(batch), out="device")
        for key in tiles:
            tiles[key][i0:i0 + k] = d[key].numpy()[:k]
    assert tiles["counts"].sum() > 0
    by_hand = _host(stitch_instances(tiles, 128, 192, ps, stride, **kw))
    _same(got, by_hand, (stride, form))
    want = ref.stitch(tiles["boxes"], tiles["scores"], tiles["labels"], tiles["counts"], tiles["masks"], 128, 192, ps, stride, **kw)
    _same(got, want, (stride, form))
    assert got["counts"].sum() > 0
    # the host form, and the lean one
    host = detect_observation(detector, data, ps, stride, views=1, normalizer=nz, batch_size=bs, instance_masks=True, out="host", **kw)
    assert len(host) == 2
    for p, o in enumerate(host):
        k = int(got["counts"][p])
        assert len(o["boxes"]) == k and np.array_equal(o["boxes"], got["boxes"][p, :k]) and np.array_equal(o["scores"], got["scores"][p, :k])
        assert np.array_equal(o["labels"], got["labels"][p, :k]) and np.array_equal(o["masks"], got["masks"][p, :k].astype(bool))
        assert np.array_equal(o["rfi_mask"], got["rfi_mask"][p].astype(bool))
    lean = detect_observation(detector, data[0], ps, stride, normalizer=nz, batch_size=bs, **kw)        # (4, C, T), no masks
    assert len(lean) == 1 and "masks" not in lean[0]
    if form == "dataset":          # (one pair for every baseline: the first baseline alone gives the same flags)
        assert np.array_equal(lean[0]["rfi_mask"], got["rfi_mask"][0].astype(bool))
    assert isinstance(detect_observation(detector, data, ps, stride, batch_size=bs, out="device", **kw)["rfi_mask"], DeviceArray)


def test_detect_observation_refuses_other_detectors(detector):
    from rfi_toolbox_amd.inference import detect_observation
    from rfi_toolbox_amd.models import MaskRCNN
    with pytest.raises(ValueError, match="stitch_instances"):
        detect_observation(MaskRCNN(2, 3, 16, 64, 128, seed=7), np.zeros((4, 64, 64), np.complex64), 64)
    with pytest.raises(ValueError):
        detect_observation(detector, np.zeros((4, 64, 64), np.float32), 64)                 # real data
    with pytest.raises(ValueError):
        detect_observation(detector, np.zeros((4, 96, 96), np.complex64), 96)               # not a size detect takes
    huge = np.broadcast_to(np.zeros((), np.complex64), (4, 8192, 8192))                     # (no memory behind it: refused by its shape)
    with pytest.raises(ValueError, match="instance_masks=False"):
        detect_observation(detector, huge, 128, instance_masks=True)                        # 64 event planes of 64 MiB: over the bound
