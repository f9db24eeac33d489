"""-m gpu: instance matching on the GPU (csrc/instance_match.hip, rfi_toolbox_amd/evaluation/detection.py) against the NumPy
restatement tests/instance_match_ref.py.  Integers, and float32 in a pinned operation order: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import instance_match_cases as cases
import instance_match_ref as ref

pytestmark = pytest.mark.gpu


def _ctx():
    from rfi_toolbox_amd.runtime import Context
    return Context.get(0)


def _lib():
    from rfi_toolbox_amd._lib import check, lib
    return check, lib


def _p(d, offset=0):
    return C.c_void_p(d.ptr + offset)


def _pack(ctx, masks_dev_ptr, m, h, w):
    """rfi_op_pack_masks on a device pointer -> (bits, area, extent) DeviceArrays."""
    check, lib = _lib()
    wc = (w + 63) // 64
    bits, area, extent = ctx.empty((m, h, wc), np.uint64), ctx.empty((m,), np.int32), ctx.empty((m, 4), np.int32)
    check(lib.rfi_op_pack_masks(ctx.handle, masks_dev_ptr, m, h, w, _p(bits), _p(area), _p(extent)))
    return bits, area, extent


# ---------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("shape", cases.PACK_SHAPES)
def test_pack_masks(shape):
    H, W = shape
    ctx = _ctx()
    c = cases.random_case(100 + H * W, 1, 12, 1, shape)
    masks = c["det_masks"][0].copy()
    masks[0], masks[1] = 0, 255                                     # an empty and a full plane among them
    masks[2] = 0
    masks[2, H - 1, W - 1] = 7                                      # the last pixel alone
    want = ref.pack(masks)
    # the planes start at an odd byte offset of a larger buffer
    buf = np.full(masks.size + 7, 255, np.uint8)
    buf[3:3 + masks.size] = masks.reshape(-1)
    dev, plain = ctx.to_device(buf), ctx.to_device(masks)
    for ptr in (_p(plain), _p(dev, 3)):
        bits, area, extent = (a.numpy() for a in _pack(ctx, ptr, len(masks), H, W))
        assert np.array_equal(bits, want[0]) and np.array_equal(area, want[1]) and np.array_equal(extent, want[2]), shape
        if W % 64:
            assert not (bits[:, :, -1] >> np.uint64(W % 64)).any()   # nothing beyond W, under a full plane too
        assert area[0] == 0 and extent[0].tolist() == [0, 0, 0, 0] and area[1] == H * W
        assert extent[2].tolist() == [H - 1, (W - 1) // 64, H, (W - 1) // 64 + 1]


# ---------------------------------------------------------------------------------------------- the C ABI on the case table and on random sets
def _run_abi(c, thr, class_aware, gt_layout="compact", repeat=2):
    """Mask IoU, box IoU and both matches of a padded case through the C ABI -> dict of host arrays.  gt_layout "compact":
    the planes of InstanceTargets (base = prefix sum of count); "padded": (n, G) planes with the garbage behind the counts
    in place and base = i G."""
    check, lib = _lib()
    ctx = _ctx()
    n, D, H, W = c["det_masks"].shape
    G = c["gt_masks"].shape[1]
    up = ctx.to_device
    d_count, g_count = up(c["det_count"]), up(c["gt_count"])
    d_masks = up(c["det_masks"])
    d_bits = _pack(ctx, _p(d_masks), n * D, H, W)
    d_base = up(np.arange(n, dtype=np.int32) * D)
    if gt_layout == "compact":
        planes = np.concatenate([c["gt_masks"][i, :int(c["gt_count"][i])] for i in range(n)])
        base = np.concatenate([[0], np.cumsum(c["gt_count"])])[:-1].astype(np.int32)
    else:
        planes, base = c["gt_masks"].reshape(n * G, H, W), np.arange(n, dtype=np.int32) * G
    m_gt = len(planes)
    g_masks = up(planes) if m_gt else None
    g_bits = _pack(ctx, _p(g_masks), m_gt, H, W) if m_gt else (ctx.empty((1,), np.uint64), ctx.empty((1,), np.int32), ctx.empty((4,), np.int32))
    g_base = up(base)
    inter, iou, biou = ctx.empty((n, D, G), np.int32), ctx.empty((n, D, G), np.float32), ctx.empty((n, D, G), np.float32)
    T = len(thr)
    dm, gm, bdm, bgm = (ctx.empty((n, T, k), np.int32) for k in (D, G, D, G))
    d_boxes, g_boxes, scores = up(c["det_boxes"]), up(c["gt_boxes"]), up(c["scores"])
    d_labels, g_labels = up(c["det_labels"]), up(c["gt_labels"])
    thr = np.ascontiguousarray(thr, np.float32)
    first = None
    for _ in range(repeat):
        check(lib.rfi_op_mask_iou(ctx.handle, *(_p(a) for a in d_bits), _p(d_count), _p(d_base), n * D, *(_p(a) for a in g_bits),
                                  _p(g_count), _p(g_base), m_gt, n, D, G, H, W, _p(inter), _p(iou)))
        check(lib.rfi_op_box_iou(ctx.handle, _p(d_boxes), _p(d_count), _p(g_boxes), _p(g_count), n, D, G, _p(biou)))
        for src, a, b in ((iou, dm, gm), (biou, bdm, bgm)):
            check(lib.rfi_op_match_instances(ctx.handle, _p(src), _p(scores), _p(d_labels), _p(d_count), _p(g_labels), _p(g_count), n, D, G,
                                             thr.ctypes.data_as(C.c_void_p), T, int(class_aware), _p(a), _p(b)))
        out = {k: v.numpy() for k, v in (("inter", inter), ("iou", iou), ("box_iou", biou), ("det_match", dm), ("gt_match", gm),
                                         ("box_det_match", bdm), ("box_gt_match", bgm))}
        if first is None:
            first = out
        else:
            for k in out:
                assert first[k].tobytes() == out[k].tobytes(), k    # repeated, the same bytes
    return first


def _want(c, thr, class_aware):
    inter, iou = ref.mask_iou(c["det_masks"], c["det_count"], c["gt_masks"], c["gt_count"])
    biou = ref.box_iou(c["det_boxes"], c["det_count"], c["gt_boxes"], c["gt_count"])
    args = (c["scores"], c["det_labels"], c["det_count"], c["gt_labels"], c["gt_count"], thr)
    dm, gm = ref.match(iou, *args, class_aware=class_aware)
    bdm, bgm = ref.match(biou, *args, class_aware=class_aware)
    return {"inter": inter, "iou": iou, "box_iou": biou, "det_match": dm, "gt_match": gm, "box_det_match": bdm, "box_gt_match": bgm}


def _same(got, want, tag):
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (tag, k)


@pytest.mark.parametrize("class_aware", (True, False))
@pytest.mark.parametrize("gt_layout", ("compact", "padded"))
def test_case_table(class_aware, gt_layout):
    c, thr = cases.table(), cases.TABLE_THRESHOLDS
    _same(_run_abi(c, thr, class_aware, gt_layout), _want(c, thr, class_aware), "table")


@pytest.mark.parametrize("n,D,G,T,shape", cases.RANDOM_SETS)
def test_random_sets(n, D, G, T, shape):
    c, thr = cases.random_case(n * 1000 + D * 3 + G, n, D, G, shape), cases.thresholds_of(T)
    want = _want(c, thr, True)
    _same(_run_abi(c, thr, True, "padded" if D % 2 else "compact"), want, (n, D, G, T))
    assert min(D, G) < 5 or (want["iou"].any() and (want["det_match"] >= 0).any())               # the set exercises something


def test_window_beyond_lds_staging():
    """A detection whose extent window holds more than 4096 words is read in place, not staged: full and thin planes of
    2100 x 130 (6300 words)."""
    shape = (2100, 130)
    c = cases.random_case(77, 1, 3, 3, shape)
    c["det_masks"][0, 0], c["gt_masks"][0, 0] = 1, 255            # full against full: the whole plane
    c["det_masks"][0, 1] = 0
    c["det_masks"][0, 1, ::2, 5:129] = 2                           # a window of every word, half of the rows set
    thr = cases.thresholds_of(10)
    got, want = _run_abi(c, thr, False, repeat=1), _want(c, thr, False)
    _same(got, want, "window")
    assert want["inter"][0, 0, 0] == 2100 * 130 and want["iou"][0, 0, 0] == 1


def test_limits_are_refused_by_name():
    from rfi_toolbox_amd._lib import RfiHipError
    check, lib = _lib()
    ctx = _ctx()
    a = ctx.empty((1024,), np.uint8)
    a.zero_()
    p = _p(a)
    thr = np.asarray([0.5], np.float32)
    tp = thr.ctypes.data_as(C.c_void_p)

    def box(n=1, D=1, G=1):
        return lib.rfi_op_box_iou(ctx.handle, p, p, p, p, n, D, G, p)

    def match(T=1, t=tp):
        return lib.rfi_op_match_instances(ctx.handle, p, p, p, p, p, p, 1, 1, 1, t, T, 1, p, p)

    for call, word in ((lambda: box(D=257), "D <= 256"), (lambda: box(G=0), "G <= 256"), (lambda: box(n=0), "n <= 65535"),
                       (lambda: match(T=33), "T <= 32"), (lambda: match(T=0), "T <= 32"),
                       (lambda: match(t=np.asarray([1.5], np.float32).ctypes.data_as(C.c_void_p)), "(0, 1]"),
                       (lambda: match(t=np.asarray([np.nan], np.float32).ctypes.data_as(C.c_void_p)), "(0, 1]"),
                       (lambda: lib.rfi_op_pack_masks(ctx.handle, p, 1, 4097, 4096, p, p, p), "2^24"),
                       (lambda: lib.rfi_op_pack_masks(ctx.handle, p, 1, 0, 4, p, p, p), "H, W >= 1"),
                       (lambda: lib.rfi_op_pack_masks(ctx.handle, p, 1, 4, 4, _p(a, 4), p, p), "aligned"),
                       (lambda: lib.rfi_op_box_iou(ctx.handle, _p(a, 2), p, p, p, 1, 1, 1, p), "aligned")):
        with pytest.raises(RfiHipError, match=None) as e:
            check(call())
        assert word in str(e.value), (word, str(e.value))


# ---------------------------------------------------------------------------------------------- the Python surface
def _device_dict(ctx, c):
    return {"boxes": ctx.to_device(c["det_boxes"]), "scores": ctx.to_device(c["scores"]), "labels": ctx.to_device(c["det_labels"]),
            "counts": ctx.to_device(c["det_count"]), "masks": ctx.to_device(c["det_masks"])}


@pytest.mark.parametrize("kind", ("mask", "box"))
def test_device_dict_and_host_lists_agree(kind):
    from rfi_toolbox_amd.evaluation import DetectionScorer, match_instances
    ctx = _ctx()
    c = cases.random_case(31, 3, 9, 6, (12, 70))
    dets, tgts = cases.lists_of(c)
    thr = ref.default_thresholds()
    a = match_instances(_device_dict(ctx, c), tgts, kind=kind)
    b = match_instances(dets, tgts, kind=kind)
    want = _want(c, thr, True)
    pre = "" if kind == "mask" else "box_"
    D, G = max(len(d["boxes"]) for d in dets), max(len(t["boxes"]) for t in tgts)
    for m in (a, b):
        out = m.numpy()
        assert (m.inter is None) == (kind == "box") and np.array_equal(out["thresholds"], thr)
        # (the device dict is D = 9 wide, the lists as wide as the longest list: equal where both have slots, empty beyond)
        assert np.array_equal(out["iou"][:, :D, :G], want[pre + "iou"][:, :D, :G]) and not out["iou"][:, D:].any()
        assert np.array_equal(out["det_match"][:, :, :D], want[pre + "det_match"][:, :, :D])
        assert np.array_equal(out["gt_match"][:, :, :G], want[pre + "gt_match"][:, :, :G])
        if kind == "mask":
            assert np.array_equal(out["inter"][:, :D, :G], want["inter"][:, :D, :G])
    s1, s2 = DetectionScorer(4, kind=kind), DetectionScorer(4, kind=kind)
    s1.update(_device_dict(ctx, c), tgts)
    s2.update(dets, tgts)
    assert ref.same(s1.summary(), s2.summary()) and ref.same(s1.summary(), ref.score(dets, tgts, 4, kind=kind))
    for x, y in zip(s1.pr_curve(1, 0.5), s2.pr_curve("1", 0.5)):
        assert np.array_equal(x, y)
    agn = DetectionScorer(4, kind=kind, class_aware=False)
    agn.update(dets, tgts)
    assert ref.same(agn.summary(), ref.score(dets, tgts, 4, kind=kind, class_aware=False))


def test_end_to_end_detector_against_simulator_instances():
    """An untrained detector on two simulator samples: equality with the restatement, not quality."""
    from rfi_toolbox_amd.core import EVENT_CLASSES, RFISimulator, event_instances
    from rfi_toolbox_amd.evaluation import match_instances, score_detections
    from rfi_toolbox_amd.models import MaskRCNN
    from rfi_toolbox_amd.preprocessing import Normalizer
    det = MaskRCNN(len(EVENT_CLASSES), 8, 16, 64, 128, seed=0)
    det.score_thresh = 0.0
    batch = RFISimulator(64, 64, seed=1).generate_batch(2, out="nhwc")
    x = Normalizer("robust_scale", scope="sample").fit_transform(batch.data, out="nhwc", layout="nhwc")
    targets = event_instances(batch, max_instances=16)
    dev = det.detect(x, out="device")
    got = score_detections(dev, targets, class_names=EVENT_CLASSES)
    got_box = score_detections(dev, targets, kind="box", class_names=EVENT_CLASSES)
    m = match_instances(dev, targets).numpy()
    host, tl = det.detect(x, out="host"), targets.to_list()
    assert sum(len(h["boxes"]) for h in host) > 0 and targets.total > 0
    assert ref.same(got, ref.score(host, tl, 6, class_names=EVENT_CLASSES))
    assert ref.same(got_box, ref.score(host, tl, 6, kind="box", class_names=EVENT_CLASSES))
    p = ref.pad_lists(host, tl)
    inter, iou = ref.mask_iou(p["det_masks"], p["det_count"], p["gt_masks"], p["gt_count"])
    D, G = inter.shape[1:]
    assert np.array_equal(m["inter"][:, :D, :G], inter) and np.array_equal(m["iou"][:, :D, :G], iou) and not m["iou"][:, D:].any()
    # boxes alone: no instance masks on either side
    boxes_only = event_instances(batch, max_instances=16, instance_masks=False)
    dev = det.detect(x, instance_masks=False, out="device")
    assert "masks" not in dev and boxes_only.masks is None
    assert ref.same(score_detections(dev, boxes_only, kind="box", class_names=EVENT_CLASSES), got_box)
    with pytest.raises(ValueError):
        score_detections(dev, boxes_only, kind="mask")
