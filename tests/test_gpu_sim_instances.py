"""-m gpu: per-emitter instance targets of RFISimulator batches (rfi_sim_event_table / rfi_sim_instances of csrc/rfi_sim.hip,
rfi_toolbox_amd.core.event_table / event_instances) against the NumPy restatement tests/sim_instances_ref.py.  Integer and
byte results throughout, and no case has a pixel within AMBIGUOUS of the floor: every comparison is exact."""
import numpy as np
import pytest

import sim_instances_ref as ref
from sim_instances_cases import CASES, TALL, ODD_PLANE, case_id

pytestmark = pytest.mark.gpu


def _sim(T, F, seed, **attrs):
    from rfi_toolbox_amd.core import RFISimulator
    sim = RFISimulator(T, F, seed=seed, device="cuda:0")
    for k, v in attrs.items():
        setattr(sim, k, v)
    return sim


def _instances(batch, **kw):
    from rfi_toolbox_amd.core import event_instances
    return event_instances(batch, **kw)


def _host(tg):
    """every array of an InstanceTargets on the host"""
    num = lambda a: None if a is None else (a if isinstance(a, np.ndarray) else a.numpy())  # noqa: E731
    return {k: num(getattr(tg, k)) for k in ("boxes", "labels", "count", "n_survivors", "base", "component", "masks")}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None and b[k] is None) or (a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and
                                                   a[k].tobytes() == b[k].tobytes()), k


def _check(tg, samples, T, F, G, **kw):
    """targets of a whole batch against the restatement's samples"""
    got = _host(tg)
    n = len(samples)
    assert tg.shape == (T, F) and len(tg) == n
    assert got["boxes"].shape == (n, G, 4) and got["boxes"].dtype == np.float32
    assert got["labels"].shape == (n, G) and got["labels"].dtype == np.int32 and got["component"].shape == (n, G)
    want = [ref.targets(s, max_instances=G, **kw) for s in samples]
    counts = [w["count"] for w in want]
    assert got["count"].tolist() == counts == tg.count_host.tolist()
    assert got["n_survivors"].tolist() == [w["n_survivors"] for w in want] == tg.n_survivors_host.tolist()
    assert got["base"].tolist() == np.concatenate([[0], np.cumsum(counts)[:-1]]).tolist()
    assert tg.n_components_host.tolist() == [len(samples[0]["area"])] * n
    for i, w in enumerate(want):
        assert np.array_equal(got["boxes"][i], w["boxes"]), i            # (rows >= count are zero in both)
        assert np.array_equal(got["labels"][i], w["labels"]), (i, got["labels"][i], w["labels"])
        assert np.array_equal(got["component"][i], w["component"]), (i, got["component"][i], w["component"])
    if got["masks"] is not None:
        assert got["masks"].dtype == np.uint8 and got["masks"].shape == (sum(counts), T, F)
        assert np.array_equal(got["masks"], np.concatenate([w["masks"] for w in want])), \
            [j for j, (a, b) in enumerate(zip(got["masks"], np.concatenate([w["masks"] for w in want]))) if not np.array_equal(a, b)]
    return got, want


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_event_table_matches_restatement(case):
    from rfi_toolbox_amd.core import event_table
    T, F, seed, n = case
    batch = _sim(T, F, seed).generate_batch(n)
    area, box = event_table(batch)
    S = batch.events.shape[1] - 1
    assert area.shape == (n, S) and area.dtype == np.int32 and box.shape == (n, S, 4) and box.dtype == np.int32
    area, box = area.numpy(), box.numpy()
    for i, s in enumerate(ref.case_reference(*case)):
        assert np.array_equal(area[i], s["area"]), (i, area[i], s["area"])
        assert np.array_equal(box[i], s["box"]), (i, np.nonzero((box[i] != s["box"]).any(axis=1))[0])


@pytest.mark.parametrize("case", CASES + (ODD_PLANE,), ids=case_id)
def test_every_event_is_an_instance(case):
    T, F, seed, n = case
    batch = _sim(T, F, seed).generate_batch(n)
    samples = ref.case_reference(*case)
    tg = _instances(batch, max_instances=256)
    assert tg.num_classes == 6
    got, want = _check(tg, samples, T, F, 256, family=True)
    mask = batch.mask.numpy()
    b = 0
    for i, s in enumerate(samples):
        k = int(got["count"][i])
        assert k == int((s["area"] > 0).sum()) == got["n_survivors"][i]
        assert np.array_equal(got["masks"][b:b + k].any(axis=0).astype(np.uint8), mask[i]), i     # OR of the instances == the mask
        assert set(np.unique(got["masks"][b:b + k]).tolist()) <= {0, 1}
        assert not got["boxes"][i, k:].any() and not got["labels"][i, k:].any() and not got["component"][i, k:].any()
        b += k
    assert b == tg.total


@pytest.mark.parametrize("classes", ["family", "single"])
@pytest.mark.parametrize("case", TALL, ids=case_id)
def test_selection_grid(case, classes):
    T, F, seed, n = case
    batch = _sim(T, F, seed).generate_batch(n)
    samples = ref.case_reference(*case)
    cut = False
    for min_area in (1, 4):
        for min_side in (1, 2):
            for G in (1, 4, 64):
                tg = _instances(batch, min_area=min_area, min_side=min_side, max_instances=G, classes=classes)
                assert tg.num_classes == (6 if classes == "family" else 2)
                got, want = _check(tg, samples, T, F, G, min_area=min_area, min_side=min_side, family=classes == "family")
                for i, w in enumerate(want):
                    assert (got["n_survivors"][i] > got["count"][i]) == (w["n_survivors"] > G)
                    cut = cut or w["n_survivors"] > G
                if classes == "single":
                    assert set(np.unique(got["labels"]).tolist()) <= {0, 1}
    assert cut


def test_split_invariance():
    """One call of four samples equals two calls of two from a second simulator with the same seed: first_sample counts."""
    T, F, seed, _ = CASES[-1]
    whole = _host(_instances(_sim(T, F, seed).generate_batch(4), max_instances=32))
    sim = _sim(T, F, seed)
    halves = [_host(_instances(sim.generate_batch(2), max_instances=32)) for _ in range(2)]
    assert sim.sample_counter == 4
    for k in ("boxes", "labels", "count", "n_survivors", "component"):
        assert np.array_equal(whole[k], np.concatenate([h[k] for h in halves])), k
    assert np.array_equal(whole["masks"], np.concatenate([h["masks"] for h in halves]))
    _check(_instances(sim.generate_batch(1), max_instances=32), ref.case_reference(T, F, seed, 1, 1.0, 4), T, F, 32)


def test_origin_snapshot():
    """The targets follow the batch as generated, not the simulator's attributes of later."""
    T, F, seed, n = CASES[3]
    sim = _sim(T, F, seed)
    batch = sim.generate_batch(n)
    o = batch.origin
    assert (o.seed, o.first_sample, o.T, o.F) == (seed, 0, T, F) and o.params.detect_floor == 1.0 and len(batch) == 4
    first = _host(_instances(batch))
    sim.detect_floor = 5.0
    sim.power_range = np.logspace(-2, 2, num=37)
    later = sim.generate_batch(n)                       # (uploads the new power table; the first batch keeps its own)
    assert later.origin.first_sample == n and later.origin.power is not o.power and batch.origin.power is o.power
    _same(first, _host(_instances(batch)))
    _check(_instances(batch), ref.case_reference(*CASES[3]), T, F, 64)
    high = _sim(T, F, seed, detect_floor=5.0)
    samples = ref.case_reference(T, F, seed, n, 5.0)
    assert any(not np.array_equal(a["area"], b["area"]) for a, b in zip(samples, ref.case_reference(*CASES[3])))
    hb = high.generate_batch(n)
    _check(_instances(hb), samples, T, F, 64)
    assert np.array_equal(hb.mask.numpy(), np.stack([s["mask"] for s in samples]).astype(np.uint8))


def test_layouts_ringing_masks_off_and_clean():
    T, F, seed, n = CASES[4]
    base = _host(_instances(_sim(T, F, seed).generate_batch(n), max_instances=32))
    for out in ("complex128", "complex64", "nchw", "nhwc"):
        _same(base, _host(_instances(_sim(T, F, seed).generate_batch(n, out=out), max_instances=32)))
    _same(base, _host(_instances(_sim(T, F, seed, gibbs_ringing=True).generate_batch(n), max_instances=32)))
    bare = _instances(_sim(T, F, seed).generate_batch(n), max_instances=32, instance_masks=False)
    assert bare.masks is None
    got = _host(bare)
    for k in ("boxes", "labels", "count", "n_survivors", "base", "component"):
        assert np.array_equal(got[k], base[k]), k
    clean = _instances(_sim(T, F, seed).generate_batch(n, clean=True), max_instances=32)
    assert len(clean) == n and clean.count_host.tolist() == [0] * n and clean.total == 0 and clean.max_count == 0
    got = _host(clean)
    assert not got["count"].any() and not got["labels"].any() and not got["boxes"].any() and got["masks"].shape == (0, T, F)


@pytest.mark.parametrize("case", [CASES[1], CASES[-1]], ids=case_id)
def test_two_runs_give_the_same_bytes(case):
    from rfi_toolbox_amd.core import event_table
    T, F, seed, n = case
    batch = _sim(T, F, seed).generate_batch(n)
    runs = []
    for _ in range(2):
        area, box = event_table(batch)
        runs.append((area.numpy().tobytes(), box.numpy().tobytes(), _host(_instances(batch, max_instances=256))))
    assert runs[0][:2] == runs[1][:2]
    _same(runs[0][2], runs[1][2])


def test_detector_trains_on_emitter_families():
    """train_step on the family targets equals train_step on their list form bit for bit (the scheme of
    test_detector_takes_instance_targets), with labels above 1 present; a two-class detector refuses them."""
    from rfi_toolbox_amd.models import MaskRCNN
    from rfi_toolbox_amd.preprocessing import Normalizer
    batch = _sim(128, 128, 5).generate_batch(3, out="nhwc")
    x = Normalizer("robust_scale", scope="sample").fit_transform(batch.data, out="nhwc", layout="nhwc")
    targets = _instances(batch, min_side=2, max_instances=16)
    assert targets.num_classes == 6 and targets.labels.numpy().max() > 1
    _check(targets, ref.case_reference(128, 128, 5, 3), 128, 128, 16, min_side=2)
    det = MaskRCNN(6, 8, 16, 64, 128, seed=7)
    det.keep_trace = True
    runs = []
    for tg in (targets, targets.to_list(), targets):
        det.sample_step = 11
        losses = det.train_step(x, tg, lr=0.0, weight_decay=0.0, max_grad_norm=1e9)
        runs.append((losses, dict(det.last_trace["grad_norms"]), det.last_trace["rois"].copy(), det.last_trace["rpn_labels"].copy(),
                     det.last_trace["num_foreground"]))
    assert all(np.isfinite(v) for v in runs[0][0].values()) and runs[0][4] > 0 and runs[0][0]["loss_mask"] > 0
    for losses, norms, rois, rpn_labels, nf in runs[1:]:
        assert losses == runs[0][0] and norms == runs[0][1] and nf == runs[0][4]
        assert np.array_equal(rois, runs[0][2]) and np.array_equal(rpn_labels, runs[0][3])
    with pytest.raises(ValueError, match="train_step"):
        MaskRCNN(2, 8, 16, 64, 128, seed=7).train_step(x, targets)
    single = _instances(batch, min_side=2, max_instances=16, classes="single")
    assert single.num_classes == 2


def test_bad_arguments_are_error_codes():
    """Out-of-range arguments of the two entry points come back as the library's error code; nothing is launched."""
    import copy
    import ctypes as C
    from rfi_toolbox_amd._lib import lib
    from rfi_toolbox_amd.core.instances import _sim_args
    from rfi_toolbox_amd.runtime import P
    T, F, seed, n = CASES[3]
    batch = _sim(T, F, seed).generate_batch(n)
    tg = _instances(batch, max_instances=8)
    before = _host(tg)
    good = _sim_args(batch)
    tail = (P(tg.component), P(tg.count), P(tg.base))

    def params(**kw):
        p = copy.copy(batch.origin.params)              # (a ctypes structure: copied by value)
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    assert lib.rfi_sim_instances(*good, *tail, 8, 1, P(tg.labels), P(tg.masks)) == 0
    for G, mode in ((0, 1), (257, 1), (8, 2), (8, -1)):
        assert lib.rfi_sim_instances(*good, *tail, G, mode, P(tg.labels), P(tg.masks)) != 0, (G, mode)
    assert lib.rfi_sim_instances(*good, None, P(tg.count), P(tg.base), 8, 1, P(tg.labels), P(tg.masks)) != 0
    area, box = batch.mask.ctx.empty((n, tg.n_components_host[0]), np.int32), batch.mask.ctx.empty((n, tg.n_components_host[0], 4), np.int32)
    for bad in (params(time_bins=3), params(freq_bins=51), params(n_power=0), params(n_power=1025), params(clean=1),
                params(time_bins=1 << 16, freq_bins=1 << 16)):
        args = good[:4] + (bad,) + good[5:]
        assert lib.rfi_sim_event_table(*args, P(area), P(box)) != 0
        assert lib.rfi_sim_instances(*args, *tail, 8, 1, P(tg.labels), P(tg.masks)) != 0
    assert lib.rfi_sim_event_table(*good[:2], (1 << 32) - 1, *good[3:], P(area), P(box)) != 0          # sample counter past 2^32
    assert lib.rfi_sim_event_table(*good[:3], -1, *good[4:], P(area), P(box)) != 0
    assert lib.rfi_sim_event_table(*good, None, P(box)) != 0 and lib.rfi_sim_event_table(*good, P(area), C.c_void_p(box.ptr + 4)) != 0
    assert len(lib.rfi_last_error()) > 0
    _same(before, _host(tg))                            # the one good call rewrote the same bytes; the bad ones wrote nothing
