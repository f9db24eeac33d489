"""-m gpu: connected components on the GPU (csrc/components.hip, rfi_toolbox_amd/components.py) against scipy.ndimage.label
and the NumPy oracle tests/components_ref.py.  Integer work throughout: every comparison is exact."""
import numpy as np
import pytest

import components_ref as ref

pytestmark = pytest.mark.gpu

CONNECTIVITIES = (4, 8)


def _c():
    from rfi_toolbox_amd import components
    return components


def _check_plane(c, name, m, conn):
    """Labels, count and table of one plane against the oracle."""
    want, k = ref.label(m, conn)
    got, gk = c.label_components(m, conn)
    assert got.dtype == np.int32 and got.shape == m.shape, name
    assert int(gk) == k and np.array_equal(got, want), (name, conn, int(gk), k)
    area, box = ref.table(want, k)
    t = c.component_table(m, conn)
    assert len(t) == 1 and t[0]["area"].dtype == np.int32 and t[0]["box"].dtype == np.int32, name
    assert np.array_equal(t[0]["area"], area) and np.array_equal(t[0]["box"].reshape(-1, 4), box), (name, conn)
    return got


@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_basic_cases(conn):
    c = _c()
    for name, m in ref.basic_cases().items():
        _check_plane(c, name, m, conn)


@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_dispatch_gates(conn):
    """Serpentine, random and the two diagonals at plane sizes just below, at and just above every size at which the code
    takes another path -- TILE_H, TILE_W (one tile: no border merge) and SCAN_BLOCK (one root count: nothing to scan
    across) -- and at shapes that are no multiple of the tile."""
    c = _c()
    TILE_H, TILE_W, SCAN_BLOCK = c.limits()
    shapes = ref.gate_shapes(TILE_H, TILE_W, SCAN_BLOCK)
    assert (130, 67) in shapes and (257, 300) in shapes and (TILE_H + 1, TILE_W) in shapes and (1, SCAN_BLOCK + 1) in shapes
    for shape in shapes:
        for name, m in ref.gate_cases(shape).items():
            first = _check_plane(c, f"{name}_{shape[0]}x{shape[1]}", m, conn)
            again, _ = c.label_components(m, conn)
            assert first.tobytes() == again.tobytes(), (name, shape)          # two runs, the same bytes


@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_batched_call_has_no_leak_across_planes(conn):
    c = _c()
    st = ref.batch_stack()
    want = [ref.label(p, conn) for p in st]
    got, k = c.label_components(st.reshape(2, 3, *st.shape[1:]), conn)      # leading axes are flattened and restored
    assert got.shape == (2, 3) + st.shape[1:] and k.shape == (2, 3)
    assert k.reshape(-1).tolist() == [w[1] for w in want]
    assert np.array_equal(got.reshape(st.shape), np.stack([w[0] for w in want]))
    t = c.component_table(st, conn)
    assert len(t) == len(st)
    for ti, (lab, kk) in zip(t, want):
        area, box = ref.table(lab, kk)
        assert np.array_equal(ti["area"], area) and np.array_equal(ti["box"].reshape(-1, 4), box)


def test_input_kinds_and_device_output():
    import torch
    from rfi_toolbox_amd.runtime import Context, DeviceArray
    c = _c()
    m = ref.random_plane(40, 50, 0.5, 11)
    want, k = ref.label(m, 8)
    for x in (m.astype(bool), m, m.astype(np.float32) * 0.25, m.astype(np.int64) * 170, m.astype(np.float64) * -3.0,
              torch.from_numpy(m), torch.from_numpy(m.astype(bool)), torch.from_numpy(m).cuda(), torch.from_numpy(m).cuda().float()):
        before = x.clone() if isinstance(x, torch.Tensor) else x.copy()
        got, gk = c.label_components(x, 8)
        assert int(gk) == k and np.array_equal(got, want), type(x)
        assert (torch.equal(x, before) if isinstance(x, torch.Tensor) else np.array_equal(x, before))
    ctx = Context.get(0)
    for dev in (ctx.to_device(m), ctx.to_device(m.astype(np.float32))):
        lab, nk = c.label_components(dev, 8, out="device")
        assert isinstance(lab, DeviceArray) and lab.dtype == np.int32 and lab.shape == m.shape
        assert np.array_equal(lab.numpy(), want) and int(nk.numpy()) == k
        assert np.array_equal(dev.numpy() != 0, m != 0)
    with pytest.raises(ValueError, match="device array"):
        c.label_components(ctx.to_device(m.astype(np.int32)), 8)


def test_checkerboard_with_131072_components():
    """More components than one sort segment holds, all of area 1: the selection must find its cut by label alone."""
    c = _c()
    m = ref.checkerboard(512, 512)
    want, k = ref.label(m, 4)
    got, gk = c.label_components(m, 4)
    assert k == 131072 and int(gk) == k and np.array_equal(got, want)
    t = c.instances_from_masks(m, connectivity=4, max_instances=256)
    assert t.count_host.tolist() == [256] and t.n_survivors_host.tolist() == [131072] and t.n_components_host.tolist() == [131072]
    assert t.component.numpy().tolist() == [list(range(1, 257))]          # the first 256 foreground pixels in raster order
    ys, xs = np.nonzero(m)
    boxes = np.stack([xs[:256], ys[:256], xs[:256] + 1, ys[:256] + 1], 1).astype(np.float32)
    assert np.array_equal(t.boxes.numpy()[0], boxes)
    masks = t.masks.numpy()
    assert masks.shape == (256, 512, 512) and masks.sum() == 256 and all(masks[j, ys[j], xs[j]] == 1 for j in range(256))
    one, k8 = c.label_components(m, 8)
    assert int(k8) == 1 and np.array_equal(one, m.astype(np.int32))


@pytest.mark.parametrize("conn", CONNECTIVITIES)
@pytest.mark.parametrize("par", ref.INSTANCE_PARAMS, ids=lambda p: "a{min_area}_s{min_side}_g{max_instances}".format(**p))
def test_instances(conn, par):
    c = _c()
    st = ref.instance_stack()
    per = [ref.instances(p, conn, **par) for p in st]
    t = c.instances_from_masks(st, connectivity=conn, **par)
    G = par["max_instances"]
    count = [r["count"] for r in per]
    assert len(t) == 3 and t.max_count == max(count) and t.shape == st.shape[1:]
    assert t.count_host.tolist() == count and t.count.numpy().tolist() == count
    assert t.n_survivors_host.tolist() == [r["n_survivors"] for r in per] == t.n_survivors.numpy().tolist()
    assert t.n_components_host.tolist() == [r["n_components"] for r in per]
    assert t.base.numpy().tolist() == np.concatenate([[0], np.cumsum(count)[:-1]]).tolist()
    boxes, labels, comp = t.boxes.numpy(), t.labels.numpy(), t.component.numpy()
    assert boxes.shape == (3, G, 4) and boxes.dtype == np.float32 and labels.dtype == np.int32
    for i, r in enumerate(per):
        assert np.array_equal(boxes[i], r["boxes"]) and np.array_equal(labels[i], r["labels"]) and np.array_equal(comp[i], r["component"])
        assert not boxes[i, r["count"]:].any() and not labels[i, r["count"]:].any()          # padding rows are zero
    masks = t.masks.numpy()
    assert masks.dtype == np.uint8 and np.array_equal(masks, np.concatenate([r["masks"] for r in per]))
    lst = t.to_list()
    for i, (d, r) in enumerate(zip(lst, per)):
        k = r["count"]
        assert np.array_equal(d["masks"], r["masks"]) and d["labels"].tolist() == [1] * k
        assert d["masks"].astype(np.int32).sum(0).max(initial=0) <= 1                          # pairwise disjoint
        if r["n_survivors"] == k and par["min_side"] == 1:                                      # nothing cut: the union is the despeckled plane
            assert np.array_equal(d["masks"].any(0), ref.despeckle(st[i], par["min_area"], conn))
    cut = [r["n_survivors"] > r["count"] for r in per]
    if G < 9:
        assert cut[0] and cut[2] and (t.n_survivors_host > t.count_host)[[0, 2]].all()
    if par["min_area"] >= 2:
        assert count[1] == 0 and count[0] > 0 and count[2] > 0                                  # no survivor between two planes with some
    bare = c.instances_from_masks(st, connectivity=conn, instance_masks=False, **par)
    assert bare.masks is None and np.array_equal(bare.boxes.numpy(), boxes) and bare.count_host.tolist() == count


@pytest.mark.parametrize("conn", CONNECTIVITIES)
def test_despeckle(conn):
    import torch
    from rfi_toolbox_amd.runtime import Context, DeviceArray
    c = _c()
    planes = np.stack([ref.random_plane(70, 90, 0.35, 21), np.repeat(np.repeat(ref.tie_plane(), 2, 0), 2, 1)[:70, :90].copy(),
                       ref.random_plane(70, 90, 0.6, 22)])
    ctx = Context.get(0)
    for min_area in (1, 3, 17, 10 ** 6):
        want = np.stack([ref.despeckle(p, min_area, conn) for p in planes])
        src = planes.copy()
        got = c.remove_small_components(src, min_area, conn)
        assert got.dtype == np.uint8 and got.shape == planes.shape and np.array_equal(got, want.astype(np.uint8))
        assert np.array_equal(src, planes)                                                      # the input is unchanged
        gb = c.remove_small_components(planes.astype(bool), min_area, conn)
        assert gb.dtype == np.bool_ and np.array_equal(gb, want)
        dev = ctx.to_device(planes)
        res = c.remove_small_components(dev, min_area, conn, out="device")
        assert isinstance(res, DeviceArray) and res.dtype == np.uint8 and res.shape == planes.shape
        assert res.numpy().tobytes() == got.tobytes() and np.array_equal(dev.numpy(), planes)
    tt = torch.from_numpy(planes.astype(np.float32)).cuda()
    out = c.remove_small_components(tt, 3, conn)
    assert out.dtype == torch.float32 and out.is_cuda and np.array_equal(out.cpu().numpy() != 0,
                                                                          np.stack([ref.despeckle(p, 3, conn) for p in planes]))


def _detector_batch():
    """3 images of 128 x 128: a few separated blobs each, the middle image without any."""
    rng = np.random.default_rng(31)
    x = rng.standard_normal((3, 128, 128, 3)).astype(np.float32) * 0.1
    masks = np.zeros((3, 128, 128), np.uint8)
    for i, rects in ((0, [(8, 10, 30, 40), (70, 60, 25, 50), (100, 8, 20, 22)]), (2, [(20, 30, 45, 28), (80, 75, 36, 40)])):
        for y, x0, h, w in rects:
            masks[i, y:y + h, x0:x0 + w] = 1
            x[i, y:y + h, x0:x0 + w] += 2.0
    return x, masks


def test_detector_takes_instance_targets():
    """train_step on InstanceTargets (ground truth and instance masks used in HBM) equals train_step on their list form bit
    for bit: losses, gradient norms, the sampled RoIs and the RPN labels (after _check_bitwise_reproducible of
    tests/test_gpu_mask_rcnn.py)."""
    import torch
    from rfi_toolbox_amd.models import MaskRCNN
    c = _c()
    torch.manual_seed(3)
    det = MaskRCNN(2, 3, 16, 64, 128, seed=7)
    det.keep_trace = True
    x, masks = _detector_batch()
    targets = c.instances_from_masks(masks)
    assert targets.count_host.tolist() == [3, 0, 2]
    lst = targets.to_list()
    wrong = c.instances_from_masks(masks[:, :64])
    with pytest.raises(ValueError, match="train_step"):
        det.train_step(x, wrong)
    with pytest.raises(ValueError, match="train_step"):
        det.train_step(x[:2], targets)
    with pytest.raises(ValueError, match="train_step"):
        det.train_step(x, c.instances_from_masks(masks, instance_masks=False))
    runs = []
    for tg in (targets, lst, targets):
        det.sample_step = 11
        losses = det.train_step(x, tg, lr=0.0, weight_decay=0.0, max_grad_norm=1e9)
        runs.append((losses, dict(det.last_trace["grad_norms"]), det.last_trace["rois"].copy(), det.last_trace["rpn_labels"].copy(),
                     det.last_trace["num_foreground"]))
    assert runs[0][4] > 0 and runs[0][0]["loss_mask"] > 0                                       # the mask branch trained
    for losses, norms, rois, rpn_labels, nf in runs[1:]:
        assert losses == runs[0][0] and norms == runs[0][1] and nf == runs[0][4]
        assert np.array_equal(rois, runs[0][2]) and np.array_equal(rpn_labels, runs[0][3])
