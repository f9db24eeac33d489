"""CPU-only checks of the connected-component surface (rfi_toolbox_amd/components.py): argument validation without a GPU,
InstanceTargets.to_list on arrays built by the oracle tests/components_ref.py, and properties of the case table that show
each case can catch what it is for."""
import numpy as np
import pytest

import components_ref as ref


def _mod():
    from rfi_toolbox_amd import components
    return components


def test_exported_from_the_package_root():
    import rfi_toolbox_amd as pkg
    c = _mod()
    assert pkg.label_components is c.label_components and pkg.component_table is c.component_table
    assert pkg.remove_small_components is c.remove_small_components and pkg.instances_from_masks is c.instances_from_masks
    assert pkg.InstanceTargets is c.InstanceTargets
    th, tw, sb = c.limits()
    assert th >= 1 and tw >= 1 and sb >= 1


def test_value_errors_are_raised_without_a_gpu():
    c = _mod()
    m = np.zeros((8, 8), np.uint8)
    calls = [lambda **kw: c.label_components(m, **kw), lambda **kw: c.component_table(m, **kw),
             lambda **kw: c.remove_small_components(m, 2, **kw), lambda **kw: c.instances_from_masks(m, **kw)]
    for call in calls:
        for conn in (0, 6, 1, 2, True, "8", None):
            with pytest.raises(ValueError, match="connectivity"):
                call(connectivity=conn)
    for bad in (0, -3, 1.5, True):
        with pytest.raises(ValueError, match="min_area"):
            c.remove_small_components(m, bad)
        with pytest.raises(ValueError, match="min_area"):
            c.instances_from_masks(m, min_area=bad)
        with pytest.raises(ValueError, match="min_side"):
            c.instances_from_masks(m, min_side=bad)
    for bad in (0, 257, -1, 2.0):
        with pytest.raises(ValueError, match="max_instances"):
            c.instances_from_masks(m, max_instances=bad)
    too_big = np.broadcast_to(np.zeros((1, 1), np.uint8), (32769, 32768))          # H W = 2^30 + 2^15, no memory behind it
    for call in (lambda x: c.label_components(x), lambda x: c.component_table(x), lambda x: c.remove_small_components(x, 1),
                 lambda x: c.instances_from_masks(x)):
        with pytest.raises(ValueError, match="ndim >= 2"):
            call(np.zeros(16, np.uint8))
        with pytest.raises(ValueError, match="2\\^30"):
            call(too_big)
    with pytest.raises(ValueError, match="out must be"):
        c.label_components(m, out="gpu")
    with pytest.raises(ValueError, match="out must be"):
        c.remove_small_components(m, 1, out="gpu")


def test_instance_targets_to_list_on_oracle_arrays():
    c = _mod()
    stack = ref.instance_stack()
    par = dict(min_area=2, min_side=2, max_instances=3)
    per = [ref.instances(p, 8, **par) for p in stack]
    count = np.asarray([r["count"] for r in per], np.int32)
    assert count.tolist() == [3, 0, 3]                                   # an image without instances between two with some
    t = c.InstanceTargets(stack.shape[1:], np.stack([r["boxes"] for r in per]), np.stack([r["labels"] for r in per]), count,
                          np.asarray([r["n_survivors"] for r in per], np.int32),
                          np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int32), np.stack([r["component"] for r in per]),
                          np.concatenate([r["masks"] for r in per]), count, [r["n_survivors"] for r in per],
                          [r["n_components"] for r in per])
    assert len(t) == 3 and t.max_count == 3 and t.total == 6 and t.shape == (64, 80)
    lst = t.to_list()
    assert len(lst) == 3
    for d, r in zip(lst, per):
        k = r["count"]
        assert d["boxes"].dtype == np.float32 and d["boxes"].shape == (k, 4) and np.array_equal(d["boxes"], r["boxes"][:k])
        assert d["labels"].dtype == np.int64 and np.array_equal(d["labels"], np.ones(k, np.int64))
        assert d["masks"].dtype == np.uint8 and d["masks"].shape == (k, 64, 80) and np.array_equal(d["masks"], r["masks"])
        for b, m in zip(d["boxes"], d["masks"]):                         # half-open boxes: the mask fills its box's extent exactly
            ys, xs = np.nonzero(m)
            assert (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1) == tuple(b)
    no_masks = c.InstanceTargets((64, 80), t.boxes, t.labels, count, count, t.base, t.component, None, count, count, count)
    with pytest.raises(ValueError, match="instance_masks"):
        no_masks.to_list()


def test_oracle_on_hand_worked_planes():
    m = np.array([[1, 0, 0, 1],
                  [0, 1, 0, 1],
                  [0, 0, 0, 0],
                  [7, 7, 0, 2]])
    lab4, k4 = ref.label(m, 4)
    lab8, k8 = ref.label(m, 8)
    assert k4 == 5 and lab4.tolist() == [[1, 0, 0, 2], [0, 3, 0, 2], [0, 0, 0, 0], [4, 4, 0, 5]]
    assert k8 == 4 and lab8.tolist() == [[1, 0, 0, 2], [0, 1, 0, 2], [0, 0, 0, 0], [3, 3, 0, 4]]
    area, box = ref.table(lab8, k8)
    assert area.tolist() == [2, 2, 2, 1] and box.tolist() == [[0, 0, 1, 1], [3, 0, 3, 1], [0, 3, 1, 3], [3, 3, 3, 3]]
    assert ref.despeckle(m, 2, 8).tolist() == [[True, False, False, True], [False, True, False, True], [False] * 4,
                                               [True, True, False, False]]
    inst = ref.instances(m, 8, min_area=2, max_instances=2)
    assert inst["count"] == 2 and inst["n_survivors"] == 3 and inst["component"].tolist() == [1, 2]      # ties: the smaller label
    assert inst["boxes"].tolist() == [[0, 0, 2, 2], [3, 0, 4, 2]]


def test_case_table_can_catch_what_it_is_for():
    s = ref.serpentine(33, 33)
    n4, n8 = ref.sweeps(s, 4), ref.sweeps(s, 8)
    print("sweeps of the 33 x 33 serpentine:", n4, n8)
    assert n4 > 500 and n8 > 500                  # far more than any fixed number of neighbour sweeps
    assert ref.label(s, 4)[1] == 1 and ref.label(s, 8)[1] == 1
    assert ref.label(ref.checkerboard(16, 18), 4)[1] == 144 and ref.label(ref.checkerboard(16, 18), 8)[1] == 1
    big = ref.checkerboard(512, 512)
    assert ref.label(big, 4)[1] == 131072 > 65536                       # more components than one sort segment holds
    # the cuts at 1 and at 3 instances fall between equal areas
    full = ref.instances(ref.tie_plane(), 8, max_instances=256)
    areas = full["areas"].tolist()
    assert areas[0] == areas[1] == 100 and areas[2] == areas[3] == 25 and full["count"] == full["n_survivors"] == 9
    # min_area and min_side each remove something the other keeps
    by_area = set(ref.instances(ref.tie_plane(), 8, min_area=16, max_instances=256)["component"].tolist()) - {0}
    by_side = set(ref.instances(ref.tie_plane(), 8, min_side=2, max_instances=256)["component"].tolist()) - {0}
    assert by_area - by_side and by_side - by_area
    assert ref.instances(ref.speck_plane(), 8, min_area=2)["count"] == 0 and ref.label(ref.speck_plane(), 8)[1] > 0
    # the diagonals: one component under 8, every pixel its own under 4, and they pass through a tile corner
    from rfi_toolbox_amd.components import limits
    th, tw, _ = limits()
    for shape in ((130, 67), (257, 300)):
        d, a = ref.diagonal(*shape), ref.anti_diagonal(*shape)
        for m in (d, a):
            assert ref.label(m, 8)[1] == 1 and ref.label(m, 4)[1] == int(m.sum()) > 64
        c = max(th, tw)
        assert c % th == 0 and c % tw == 0 and d[c - 1, c - 1] and d[c, c] and a[c - 1, c] and a[c, c - 1]
    # the batched stack: a leak from plane 1's last row into plane 2's first row would merge components
    st = ref.batch_stack()
    assert st[1, -1].all() and st[2, 0].all() and not st[3].any()
