"""CPU-only: the per-emitter instance targets of RFISimulator batches -- the NumPy restatement tests/sim_instances_ref.py
against RefSimulator's own mask, that the case table reaches the situations it is there for, and the host side of the
feature (exports, argument checks, InstanceTargets.num_classes).  No GPU work is started."""
import numpy as np
import pytest

import sim_instances_ref as ref
from sim_instances_cases import CASES, TALL, ODD_PLANE, case_id


@pytest.mark.parametrize("case", CASES + (ODD_PLANE,), ids=case_id)
def test_union_of_event_masks_is_the_mask(case):
    for i, s in enumerate(ref.case_reference(*case)):
        assert s["masks"].shape == (13 + int(case[1] * 0.05) + int(case[0] * 0.1), case[0], case[1])
        assert np.array_equal(s["masks"].any(axis=0), s["mask"]), (case, i)
        assert not s["ambiguous"].any(), (case, i)              # no pixel within AMBIGUOUS of the floor: exact on any libm
        area, box = ref.table(s["masks"])
        assert np.array_equal(area, s["masks"].reshape(len(area), -1).sum(axis=1)) and not box[area == 0].any()


def test_case_table_reaches_what_it_claims():
    samples = [(c, s) for c in CASES for s in ref.case_reference(*c)]
    assert len(samples) == 19
    assert CASES[0][:2] == (4, 52) and int(CASES[0][0] * 0.1) == 0 and CASES[0][0] // 4 == 1
    assert all(int(s["events"][b]["i1"]) == 50 for s in ref.case_reference(*CASES[0]) for b in (1, 2, 3))
    assert (CASES[1][0] * CASES[1][1]) % 16 != 0
    two = [s for _, s in samples if int(s["events"][0]["i0"]) == 2]
    assert two and all(s["area"][2] == 0 and not s["box"][2].any() for s in two)        # the unused third broadband slot
    assert any((s["area"][3:] == 0).any() for _, s in samples)                          # empty events besides it
    unwrapped = [fu for c, s in samples for pts in s["sweeps"].values() for _, fu in pts]
    assert min(unwrapped) < 0
    assert any(fu >= c[1] for c, s in samples for pts in s["sweeps"].values() for _, fu in pts)
    for c, s in samples:
        kept, ns = ref.select(s["area"], s["box"], 1, 1, 256)
        assert ns == int((s["area"] > 0).sum()) == len(kept)
    assert any(len(set(s["area"][s["area"] > 0].tolist())) < int((s["area"] > 0).sum()) for _, s in samples)      # area ties
    for c in TALL:
        for s in ref.case_reference(*c):
            assert int((s["area"] > 0).sum()) >= 13                                   # max_instances = 4 cuts
            kept, ns = ref.select(s["area"], s["box"], 1, 2, 256)
            cls = ref.classes(c[0], c[1])[[l - 1 for l in kept]]
            assert 2 <= ns <= 13 and 2 not in cls and 3 not in cls                      # min_side = 2: no narrowband, no burst


def test_selection_rule():
    area = np.array([5, 9, 0, 9, 1, 5], np.int32)
    box = np.array([[0, 0, 4, 0], [0, 0, 2, 2], [0, 0, 0, 0], [1, 1, 3, 3], [7, 7, 7, 7], [2, 0, 2, 4]], np.int32)
    assert ref.select(area, box, 1, 1, 256) == ([2, 4, 1, 6, 5], 5)                     # descending area, ties ascending slot
    assert ref.select(area, box, 1, 1, 3) == ([2, 4, 1], 5)
    assert ref.select(area, box, 2, 1, 256) == ([2, 4, 1, 6], 4)
    assert ref.select(area, box, 1, 2, 256) == ([2, 4], 2)


def test_library_exports_the_entry_points():
    from rfi_toolbox_amd import _lib
    for name, nargs in (("rfi_sim_event_table", 9), ("rfi_sim_instances", 14)):
        assert name in _lib.EXPORTED
        fn = getattr(_lib.lib, name)
        assert len(fn.argtypes) == nargs and fn.argtypes[4] is not None
    # bad arguments are the library's error code, before anything touches a device (there is no context here)
    p = _lib.SimParams()
    p.time_bins, p.freq_bins, p.n_power = 128, 128, 100
    assert _lib.lib.rfi_sim_event_table(None, 0, 0, 1, None, None, None, None, None) != 0
    assert _lib.lib.rfi_sim_instances(None, 0, 0, 1, None, None, None, None, None, None, 4, 0, None, None) != 0
    assert b"null" in _lib.lib.rfi_last_error()


def test_public_names():
    import rfi_toolbox_amd
    from rfi_toolbox_amd import EVENT_CLASSES, core, event_instances, event_table
    assert EVENT_CLASSES == ("background", "broadband", "narrowband", "burst", "linear_sweep", "quadratic_sweep")
    assert core.event_instances is event_instances and core.event_table is event_table and core.EVENT_CLASSES is EVENT_CLASSES
    assert rfi_toolbox_amd.event_instances is event_instances
    assert [ref.FAMILY[k] for k in sorted(ref.FAMILY)] == [EVENT_CLASSES.index(n) for n in EVENT_CLASSES[1:]]


def test_sim_batch_stays_a_four_tuple():
    from rfi_toolbox_amd.core import SimBatch
    b = SimBatch(1, 2, 3, 4)
    data, mask, bl, events = b
    assert len(b) == 4 and (data, mask, bl, events) == (1, 2, 3, 4) and b == (1, 2, 3, 4)
    assert SimBatch._fields == ("data", "mask", "baseline_frac", "events") and b.events == 4 and b.origin is None
    assert SimBatch(1, 2, 3, 4, origin="o").origin == "o" and len(SimBatch(1, 2, 3, 4, origin="o")) == 4
    assert b._replace(mask=5).mask == 5


def test_event_instances_rejects_bad_arguments_without_a_context():
    from rfi_toolbox_amd.core import SimBatch, event_instances, event_table
    from rfi_toolbox_amd.runtime import Context
    before = dict(Context._cache)
    batch = SimBatch(None, None, None, None)
    for kw in ({"max_instances": 0}, {"max_instances": 257}, {"max_instances": True}, {"max_instances": 4.0}, {"min_area": 0},
               {"min_area": 1.5}, {"min_side": 0}, {"classes": "families"}, {"classes": 1}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            event_instances(batch, **kw)
    for bad in (np.zeros((1, 4, 52), np.uint8), None, (1, 2, 3, 4), batch):             # (the last: a SimBatch without an origin)
        with pytest.raises(ValueError, match="SimBatch"):
            event_instances(bad)
        with pytest.raises(ValueError, match="SimBatch"):
            event_table(bad)
    assert dict(Context._cache) == before


def test_instance_targets_num_classes_defaults_to_two():
    from rfi_toolbox_amd.components import InstanceTargets
    z = np.zeros(0, np.int32)
    args = ((4, 4), np.zeros((0, 1, 4), np.float32), np.zeros((0, 1), np.int32), z, z, z, np.zeros((0, 1), np.int32), None, z, z, z)
    assert InstanceTargets(*args).num_classes == 2
    assert InstanceTargets(*args, num_classes=6).num_classes == 6
