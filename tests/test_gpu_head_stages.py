"""-m gpu: the mask head, the RPN head and the box head stage by stage on the device's own tensors (tests/head_stages.py states the
method, the stage table, the per-mode oracles, the measured table and what was found).

test_head_stages[case-mode]       one forward + backward pass, every stored tensor read back through debug_tensor, the whole stage
                                  table checked at k = 16; every row checked, every tensor finite, exact zeros present; the
                                  contraction kernels the case is there for ran (the context profile's labels).  Prints HEADSTAGES
test_sequence[head]               one model over several RoI counts / map sizes and back: every run stage-checked, the last run
                                  equal to the first bit for bit, the RPN head's accumulated gradient within the summed bounds
test_bf16_vs_oracle[head]         RPN and box head in "bfloat16" against the oracle under unet_ref.bf16_operands(), with
                                  test_bf16_operand_mode's criterion
test_debug_tensor_names           element counts, refusals, and that the other models refuse the heads' names
"""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import head_stages as H
from rfi_toolbox_amd._lib import HOST, check, lib
from rfi_toolbox_amd.models import BoxHead, MaskHead, RPNHead, UNet
from rfi_toolbox_amd.models import detection_ops as ops
from rfi_toolbox_amd.runtime import Context, as_pointer

pytestmark = pytest.mark.gpu

FAMILIES = ("conv_igemm_mfma", "wgrad_igemm_mfma", "conv_direct_valu")


def _model(c, state, mode):
    cls = {"mask": MaskHead, "rpn": RPNHead, "box": BoxHead}[c.head]
    return cls(*c.args).load_state_dict(state).train().set_compute_dtype(mode)


def _backward_dlogits(m, x, d):
    """The mask head has no label form for several classes: the backward pass from a given dlogits, as RPNHead.backward runs it."""
    n, h, w, _ = x.shape
    xp, xm, keep = as_pointer(x, np.float32, m.ctx)
    d = np.ascontiguousarray(d, np.float32)
    check(lib.rfi_model_backward_dlogits(m._h, C.c_void_p(xp), xm, d.ctypes.data_as(C.c_void_p), HOST, n, h, w))
    del keep


def _pass(m, c, inp, shape=None):
    """One forward + backward pass -> (the loss value(s), the checker's tensor dictionary)."""
    x, given = inp["x"], None
    if H.own_loss(c):
        loss = (m.forward_backward(x, inp["y"]),)
    elif c.head == "mask":
        m.forward_nhwc(x)
        loss, given = (), inp["dlogits"]
        _backward_dlogits(m, x, given)
    elif c.head == "rpn":
        a = c.args[1]
        out = m.forward_nhwc(x)
        lo, lb, given = ops.rpn_loss(out.reshape(-1, 5 * a), inp["labels"], inp["targets"], a)
        loss = (lo, lb)
        m.backward(x, given)
    else:
        out = m.forward_rois(x)
        lc, lb, given = ops.fastrcnn_loss(out, inp["labels"], inp["targets"])
        loss = (lc, lb)
        m.backward(x, given)
    T = H.read_device(m, c, inp, shape)
    if given is not None:
        T["given"] = np.asarray(given, np.float32)
    return loss, T


def _profiled(fn):
    """fn() under the context profile -> (its result, the labels of the contraction families), read as
    tests/golden/make_launch_labels.py::launch_labels reads them."""
    ctx = Context.get(0)
    ctx.profile_reset()
    ctx.profile(True)
    try:
        out = fn()
    finally:
        ctx.profile(False)
    fd, path = tempfile.mkstemp(suffix=".csv")
    os.close(fd)
    try:
        ctx.profile_dump(path)
        rows = [line.rstrip("\n").split(",") for line in open(path)][1:]
    finally:
        os.remove(path)
        ctx.profile_reset()
    return out, [r[2] for r in rows if r[1] in FAMILIES]


def _checked(c, mode, P, T, run_id=None):
    ck = H.check(c, mode, P, T, run_id)
    print("%s %s %s" % (H.TAG, ck.id, " | ".join("%s %.3g %s" % (f.klass, f.ratio, f.tensor) for f in ck.worst_per_class().values())))
    for f in ck.failures():
        print("%s-FAIL %s %s %s %s %.4g > %.4g %s" % (H.TAG, ck.id, f.stage, f.klass, f.tensor, f.ratio, f.limit, f.detail))
    assert ck.unchecked_rows() == []                      # every row of the table, none skipped
    assert ck.nonfinite == []                             # every stored tensor and gradient is finite
    assert ck.undecided == 0                              # (masks are decided on the stored float32 value: by construction)
    assert ck.zeros > 0
    assert not ck.failures(), ck.failed_stages()
    return ck


@pytest.mark.parametrize("cid,mode", H.RUNS)
def test_head_stages(cid, mode):
    c = H.BY_ID[cid]
    state, P = H.init_params(c)
    m = _model(c, state, mode)
    inp = H.inputs(c)
    (_, T), labels = _profiled(lambda: _pass(m, c, inp))
    _checked(c, mode, P, T)
    assert H.kernel_mismatches(c, mode, labels) == [], labels


def _same_bits(a, b):
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


@pytest.mark.parametrize("head", list(H.SEQUENCES))
def test_sequence(head):
    cid, shapes = H.SEQUENCES[head]
    c = H.BY_ID[cid]
    mode = H.F32
    state, P = H.init_params(c)
    m = _model(c, state, mode)
    if head == "rpn":
        m.accumulate_gradients("begin")
    runs = []
    for k, shape in enumerate(shapes):
        inp = H.inputs(c, shape, 0 if k == len(shapes) - 1 else k)          # the last run repeats the first
        loss, T = _pass(m, c, inp, shape)
        ck = _checked(c._replace(shape=shape), mode, P, T, "%s/seq%d:%s" % (cid, k, "x".join(map(str, shape))))
        runs.append((loss, T, ck))
        if head == "rpn":
            m.accumulate_gradients("add")
    (l0, T0, _), (l1, T1, _) = runs[0], runs[-1]
    assert _same_bits(l0, l1), (l0, l1)
    for name in ("logits", "dlogits", "dx"):
        assert _same_bits(T0[name], T1[name]), name
    for k in T0["grad"]:
        assert _same_bits(T0["grad"][k], T1["grad"][k]), k
    if head == "rpn":
        m.accumulate_gradients("end")
        from rfi_toolbox_amd.models.unet import HipSegmenter
        total = {k: HipSegmenter.grad(m, nm) for k, nm in H.keys(c).items()}
        acc = H.check_accumulated(c, mode, [r[2] for r in runs], total)
        print("%s %s/accumulated %s" % (H.TAG, cid, " | ".join("%s %.3g %s" % (f.klass, f.ratio, f.tensor) for f in acc.worst_per_class().values())))
        assert len(acc.findings) == len(H.keys(c)) and not acc.failures(), [(f.tensor, f.ratio) for f in acc.failures()]


@pytest.mark.parametrize("cid", ["rpn_c16_a4_l1_2x8x8", "box_c16_r7_h64_k2_96"])
def test_bf16_vs_oracle(cid):
    c = H.BY_ID[cid]
    state, _ = H.init_params(c)
    inp = H.inputs(c)
    loss, T = _pass(_model(c, state, H.BF), c, inp)
    assert H.bf16_notices(c, state, inp, T, loss) == []


def test_debug_tensor_names():
    for cid in ("mask_c16_k1_l4_5x14x14", "rpn_c32_a4_l2_1x24x20", "box_c8_r3_h32_k5_37"):
        c = H.BY_ID[cid]
        state, _ = H.init_params(c)
        m = _model(c, state, H.F32)
        _pass(m, c, H.inputs(c))
        for name in H.tensor_names(c):
            assert m.debug_tensor(name).size == int(np.prod(H.shape_of(c, name))), name
        L = H.depth(c)
        bad = ["y.%d" % L, "dy.%d" % L, "y.-1", "y", "dy", "dx.0", "u.0", "y.0:pad", "encY1.1", "conv.0", "nonsense"]
        bad += [] if c.head == "mask" else ["u", "du"]
        for name in bad:
            with pytest.raises(RuntimeError):
                m.debug_tensor(name)
    mu = UNet(3, 1, 8, depth=1).train()
    mu.forward_backward(np.zeros((1, 16, 16, 3), np.float32), np.zeros((1, 16, 16), np.uint8))
    assert mu.debug_tensor("logits").size == 256
    for name in ("y.0", "dy.0", "u", "du", "dx"):
        with pytest.raises(RuntimeError):
            mu.debug_tensor(name)
