"""-m gpu: rfi_threshold_sweep / rfi_model_eval_sweep and their Python surface against the NumPy restatement
(tests/threshold_sweep_ref.py) and against the library's own single-threshold kernels.  Every comparison is exact
integer equality: the counts are integers, whatever the grid, the replicas or the order of the atomic adds."""
import ctypes as C

import numpy as np
import pytest
import torch

import threshold_sweep_ref as ref
from gpu_util import ctx
from rfi_toolbox_amd._lib import check, lib
from rfi_toolbox_amd.evaluation import confusion_counts, default_thresholds, threshold_sweep
from rfi_toolbox_amd.models import UNet, UNetOverfit
from rfi_toolbox_amd.training import evaluate_rfi_model, sweep_rfi_model

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 255, 1023, 4097, 100003)
KS = (1, 2, 63, 64, 65, 1024)


def _counts(sw):
    return np.stack([sw.tp, sw.fp, sw.fn], axis=-1)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", COUNTS)
def test_probabilities_against_the_restatement(n, K, dtype):
    thr = ref.thresholds(K)
    p, t = ref.scores(n, thr, n + K), ref.truth(n, dtype, n + K)
    sw = threshold_sweep(p, t, thr)
    assert sw.tp.dtype == np.int64 and sw.tp.shape == (K,) and int(sw.count) == n
    assert np.array_equal(_counts(sw), ref.sweep_counts(p, t, thr)[0])


def test_special_values_one_by_one():
    """strict '>', thresholds outside [0, 1], +-inf, NaN and -0.0, each as the only element"""
    thr = np.array([-0.5, 0.0, 0.5, 1.0, 1.5], np.float32)
    want = [(-0.5, 0), (0.0, 1), (-0.0, 1), (0.5, 2), (1.0, 3), (1.5, 4), (2.0, 5), (-1.0, 0), (np.inf, 5), (-np.inf, 0),
            (np.nan, 0), (np.nextafter(np.float32(0.5), np.float32(1)), 3)]
    for v, flagged_at in want:
        sw = threshold_sweep(np.array([v], np.float32), np.array([1], np.uint8), thr)
        assert sw.tp.tolist() == [1] * flagged_at + [0] * (5 - flagged_at), v
        assert sw.fn.tolist() == [0] * flagged_at + [1] * (5 - flagged_at), v
        assert sw.fp.tolist() == [0] * 5


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_device_slices_at_any_element_offset(dtype):
    n, thr = 5003, ref.thresholds(65)
    S = ref.scores(n + 3, thr, 7)
    T = ref.truth(n + 3, np.uint8 if dtype == torch.uint8 else np.float32, 7)
    Sd, Td = torch.from_numpy(S).cuda(), torch.from_numpy(T).cuda()
    for a in (0, 1, 3):
        for b in (0, 1, 3):
            got = _counts(threshold_sweep(Sd[a:a + n], Td[b:b + n], thr))
            host = _counts(threshold_sweep(S[a:a + n].copy(), T[b:b + n].copy(), thr))
            assert np.array_equal(got, host), (a, b)
            assert np.array_equal(got, ref.sweep_counts(S[a:a + n], T[b:b + n], thr)[0]), (a, b)


def _grouped(p, t, thr, group_elems):
    """the grouped call through the C entry point (any group size, not only a product of leading axes)"""
    n_groups = p.size // group_elems
    out = np.empty((n_groups, thr.size, 3), np.int64)
    check(lib.rfi_threshold_sweep(ctx().handle, p.ctypes.data_as(C.c_void_p), 0, 1, t.ctypes.data_as(C.c_void_p),
                                  0 if t.dtype == np.uint8 else 1, 0, p.size, group_elems, thr.ctypes.data_as(C.c_void_p),
                                  thr.size, out.ctypes.data_as(C.c_void_p)))
    return out


@pytest.mark.parametrize("n,group_elems", [(1001, 77), (1002, 3), (1001, 1001), (77 * 301, 301)])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_groups(n, group_elems, dtype):
    thr = ref.thresholds(9)
    p, t = ref.scores(n, thr, 11), ref.truth(n, dtype, 11)
    got = _grouped(p, t, thr, group_elems)
    assert np.array_equal(got, ref.sweep_counts(p, t, thr, group_elems))
    if group_elems == n:
        assert np.array_equal(got[0], _counts(threshold_sweep(p, t, thr)))


def test_groups_on_the_device_start_at_odd_elements():
    thr = ref.thresholds(9)
    p, t = ref.scores(1002, thr, 12), ref.truth(1002, np.uint8, 12)
    pd, td = torch.from_numpy(p).cuda()[1:].reshape(13, 77), torch.from_numpy(t).cuda()[1:].reshape(13, 77)
    sw = threshold_sweep(pd, td, thr, per=1)
    assert np.array_equal(_counts(sw), ref.sweep_counts(p[1:], t[1:], thr, 77))


def test_per_equals_separate_calls():
    thr = ref.thresholds(5)
    shape = (2, 3, 5, 7)
    p = ref.scores(210, thr, 13).reshape(shape)
    t = ref.truth(210, np.uint8, 13).reshape(shape)
    sw = threshold_sweep(p, t, thr, per=2)
    assert sw.tp.shape == (2, 3, 5) and sw.count.tolist() == [[35] * 3] * 2
    for i in range(2):
        for j in range(3):
            one = threshold_sweep(p[i, j], t[i, j], thr)
            assert np.array_equal(_counts(sw)[i, j], _counts(one)), (i, j)
    assert np.array_equal(_counts(sw.pooled()), _counts(threshold_sweep(p, t, thr)))
    assert np.array_equal(_counts(threshold_sweep(p, t, thr, per=0)), _counts(threshold_sweep(p, t, thr)))
    assert threshold_sweep(p, t, thr, per=4).tp.shape == shape + (5,)


@pytest.mark.parametrize("case", ["zeros", "ones", "bimodal"])
def test_hot_bins(case):
    rng = np.random.default_rng(3)
    n = (1 << 20) + 5
    thr = default_thresholds()
    if case == "bimodal":
        u = rng.random(n)
        p = np.where(u < 0.95, rng.uniform(0, 0.005, n), np.where(u < 0.99, rng.uniform(0.995, 1.0, n), rng.random(n)))
        p = p.astype(np.float32)
    else:
        p = np.full(n, 0.0 if case == "zeros" else 1.0, np.float32)
    t = (rng.random(n) < 0.3).astype(np.uint8)
    sw = threshold_sweep(p, t, thr)
    P = int(t.sum())
    assert np.all(sw.tp + sw.fn == P)
    if case == "bimodal":
        assert np.array_equal(_counts(sw), ref.sweep_counts(p, t, thr)[0])
    else:
        flagged = case == "ones"
        assert np.all(sw.tp == (P if flagged else 0)) and np.all(sw.fp == (n - P if flagged else 0))


def test_logits_equal_the_single_threshold_kernels():
    """kind='logits' against rfi_threshold_logits -> confusion_counts on the same device array: the existing kernels
    are the yardstick, no host expf takes part"""
    c = ctx()
    rng = np.random.default_rng(17)
    n = 100003
    thr = np.array([0.1, 0.3, 0.5, 0.7, 0.9], np.float32)
    x = (rng.standard_normal(n) * 3).astype(np.float32)
    # a third of the logits within a few float32 steps of the cuts' own logits, where one rounding decides
    near = np.log(thr.astype(np.float64) / (1 - thr.astype(np.float64))).astype(np.float32)
    at = rng.random(n) < 0.33
    step = rng.integers(-3, 4, int(at.sum()))
    base = near[rng.integers(0, 5, int(at.sum()))]
    x[at] = (base.view(np.int32) + step.astype(np.int32)).view(np.float32)
    x[:4] = [np.inf, -np.inf, np.nan, 0.0]
    t = ref.truth(n, np.uint8, 17)
    xd, td, mask = c.to_device(x), c.to_device(t), c.empty((n,), np.uint8)
    sw = threshold_sweep(xd, td, thr, kind="logits")
    for k in range(5):
        check(lib.rfi_threshold_logits(c.handle, C.c_void_p(xd.ptr), n, float(thr[k]), C.c_void_p(mask.ptr)))
        assert (int(sw.tp[k]), int(sw.fp[k]), int(sw.fn[k])) == confusion_counts(mask, td), k
    assert np.array_equal(_counts(threshold_sweep(x, t, thr, kind="logits")), _counts(sw))


def test_host_and_device_inputs_agree_and_repeat():
    c = ctx()
    thr = default_thresholds()
    p, t = ref.scores(100003, thr, 19), ref.truth(100003, np.float32, 19)
    host = _counts(threshold_sweep(p, t, thr))
    pd, td = c.to_device(p), c.to_device(t)
    assert np.array_equal(_counts(threshold_sweep(pd, td, thr)), host)
    assert np.array_equal(_counts(threshold_sweep(pd, td, thr)), host)
    assert np.array_equal(_counts(threshold_sweep(torch.from_numpy(p).cuda(), torch.from_numpy(t), thr)), host)
    assert np.array_equal(_counts(threshold_sweep(p, t != 0, thr)), host)          # bool truth
    assert np.array_equal(_counts(threshold_sweep(p, t, None)), host)             # the default list


def test_more_than_1024_thresholds_in_the_callers_order():
    rng = np.random.default_rng(23)
    thr = ref.thresholds(1500, -0.2, 1.2)
    thr = np.concatenate([thr, thr[:10]])[rng.permutation(1510)]                  # unsorted, with duplicates
    p, t = ref.scores(4097, thr, 23), ref.truth(4097, np.uint8, 23)
    sw = threshold_sweep(p, t, thr)
    assert np.array_equal(sw.thresholds, thr)
    assert np.array_equal(_counts(sw), ref.sweep_counts(p, t, thr)[0])


def test_library_rejects_bad_arguments():
    p, t = np.zeros(8, np.float32), np.zeros(8, np.uint8)
    out = np.empty((8, 2, 3), np.int64)

    def call(thr, count=8, group_elems=8, kind=1):
        thr = np.asarray(thr, np.float32)
        return lib.rfi_threshold_sweep(ctx().handle, p.ctypes.data_as(C.c_void_p), 0, kind, t.ctypes.data_as(C.c_void_p), 0, 0,
                                       count, group_elems, thr.ctypes.data_as(C.c_void_p), thr.size, out.ctypes.data_as(C.c_void_p))
    assert call([0.2, 0.8]) == 0
    assert call([0.8, 0.2]) != 0 and call([0.5, 0.5]) != 0 and call([np.nan]) != 0 and call([np.inf]) != 0
    assert call([0.5], group_elems=3) != 0 and call([0.5], count=0) != 0 and call([0.5], kind=2) != 0
    assert call(np.linspace(0, 1, 1025)) != 0 and call([]) != 0


def _model(cls):
    torch.manual_seed(31)
    return cls(3, 1, 4)


def _batch(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, size, size, 3, generator=g)
    y = (torch.rand(n, size, size, generator=g) > 0.6).to(torch.uint8)
    return x, y


# UNetOverfit pools five times, so its sides are multiples of 32: it runs at 2 x 32 x 32, the smallest input it takes
MODELS = [("unet", lambda: _model(UNet), 16), ("overfit", lambda: _model(UNetOverfit), 32)]


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name,make,size", MODELS, ids=[m[0] for m in MODELS])
def test_eval_sweep_equals_eval_batch(name, make, size, training):
    m = make()
    m.train(training)
    x, y = _batch(2, size, 5)
    thr = [0.3, 0.5, 0.7]
    got = m.eval_sweep(x, y, thr)
    assert got.dtype == np.int64 and got.shape == (3, 3) and m.training == training
    for k, t in enumerate(thr):
        assert tuple(int(v) for v in got[k]) == m.eval_batch(x, y, t), (k, t)
    # the caller's order, duplicates included; device-resident inputs
    again = m.eval_sweep(x.cuda(), y.cuda(), [0.7, 0.3, 0.7])
    assert np.array_equal(again, got[[2, 0, 2]])


@pytest.mark.parametrize("name,make,size", MODELS, ids=[m[0] for m in MODELS])
def test_sweep_rfi_model_equals_evaluate_rfi_model(name, make, size):
    m = make()
    m.train()
    x, y = _batch(6, size, 9)                                  # batches of 4 and 2
    res = sweep_rfi_model(m, (x, y), batch_size=4)
    assert m.training                                          # mode restored
    thr = res["thresholds"]
    assert np.array_equal(thr, default_thresholds())
    for cut in (0.5, 0.25):
        k = int(np.flatnonzero(thr == np.float32(cut))[0])
        want = evaluate_rfi_model(m, (x, y), batch_size=4, threshold=float(np.float32(cut)))
        for name_, v in want.items():
            assert res["mean_per_batch"][name_][k] == v, (cut, name_)     # same integers through the same host formulas
    m.eval()
    pooled = np.sum([m.eval_sweep(x[:4], y[:4], thr), m.eval_sweep(x[4:], y[4:], thr)], axis=0)
    assert np.array_equal(_counts(res["pooled"]), pooled) and int(res["pooled"].count) == y.numel()
    for name_, (cut, value) in res["best"].items():
        curve = res["mean_per_batch"][name_]
        assert value == curve.max() and cut == float(thr[int(np.argmax(curve))])
    with pytest.raises(ValueError):
        sweep_rfi_model(m, (x[:0], y[:0]))
