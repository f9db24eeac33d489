"""Case tables, call adapters and event scripts of tests/test_gpu_derived_copies.py (importable without a GPU; checked by
tests/test_derived_copy_cases_host.py).

Every conv-like layer keeps derived device copies of its filters ("Derived filter copies: who invalidates, who
rebuilds").  The tests drive a USED model through a script of events and, at every compared pass, build a TWIN -- a new
instance with the same constructor arguments, compute mode and train / eval flag, loaded with the used model's state
(state_dict, every Adam moment, the Adam step) as it was just before the call -- which makes the same single call on the
same inputs.  The twin builds every copy from scratch, so a copy the used model failed to rebuild is a byte difference.

ARCHS        one row per network: class, constructor arguments, call adapter, shapes, the mid-network layer of the partial
             load and of the negative control, the events it runs
MODES        the compute modes; every class accepts all five (set_compute_dtype's docstring: where a class has no plane flow
             it falls back, and the twin falls back the same way)
scripts()    {event: [op, ...]} for a row.  Ops:
               ("pass", name, shape_index[, "base"])   one call of PASSES; compared with a twin unless "base" (the fresh
                                                        model's own first passes: the values later passes must differ from)
               ("fused_raises",)                        train_step raises the documented error (models whose loss lives outside)
               ("load_partial", "weight" | "frozen")    load_state_dict({one tensor}, strict=False)
               ("load_full",)                           load_state_dict of a whole changed state
               ("mode", "A" | "B")                      set_compute_dtype
               ("overlap", bool) / ("profile", bool)    context switches
"""
from collections import OrderedDict, namedtuple

import numpy as np

MODES = ("float32", "float32_mfma", "bfloat16", "bfloat16_regs", "float32_planes")
# lr = 1e-2 without weight decay and with a clip that never binds: Adam moves every weight by ~1e-2, thousands of float32
# ulps and many bfloat16 ulps of a filter of magnitude ~1e-1
STEP = dict(lr=1e-2, weight_decay=0.0, max_grad_norm=1e9)
PERTURB = np.float32(1.0 + 2.0 ** -6)           # the negative control's factor on one filter element

ALL = "all"
Arch = namedtuple("Arch", "id cls args kwargs kind shapes mid frozen events")
# kind: seg (loss inside the model), mask (seg + input_grad), rpn / box / backbone (loss outside: forward, backward from a given
# output gradient, apply_gradients).  shapes: (n, h, w) of the input map; rpn: a tuple of levels; box: (rois,).
# mid: the layer of the partial load and the negative control, by its name in the library's table: a conv in the middle
# third of the forward order with conv layers on both sides (the RPN head has two layers: its output layer).
ARCHS = (
    Arch("unet_f16", "UNet", (3, 1, 16), {}, "seg", ((2, 64, 64), (1, 16, 16)), "decoder3.conv.conv.0.weight", None, ALL),
    # depth 2 instead of the default 4: 0.5 M parameters instead of 7.8 M.  Every compared step moves the whole state and both Adam
    # moments across the host boundary four times; at depth 4 this one row took half the file's time.  The stem kernels (4 -> 32)
    # and the transposed convs on the plane kernels (widths in whole 32-channel blocks) are reached at either depth
    Arch("unet_in4_f32", "UNet", (4, 1, 32), {"depth": 2}, "seg", ((2, 32, 32), (1, 16, 48)), "decoder2.conv.conv.0.weight", None, ALL),
    Arch("unet_f6", "UNet", (3, 1, 6), {}, "seg", ((2, 32, 32), (1, 16, 48)), "decoder3.conv.conv.0.weight", None, ALL),
    Arch("resnet18_f16", "UNetResNet18", (3, 1, 16), {}, "seg", ((2, 64, 64), (1, 32, 32)), "decoder3.conv.conv.0.weight", None, ALL),
    Arch("cnn_w64", "SimpleCNN", (3, 1, 64), {}, "seg", ((2, 32, 32), (1, 16, 48)), "encoder.2.weight", None, ALL),
    Arch("mask_head", "MaskHead", (16, 1, 4), {}, "mask", ((6, 14, 14), (10, 14, 14)), "mask_fcn3.weight", None, ALL),
    Arch("rpn_head", "RPNHead", (16, 4), {}, "rpn", (((2, 16, 16), (2, 8, 8)), ((1, 32, 32), (1, 16, 16))), "head.weight", None, ALL),
    Arch("box_head", "BoxHead", (16, 7, 64, 2), {}, "box", ((96,), (50,)), "fc7.weight", None, ALL),
    Arch("backbone", "ResNet50FPN", (3, 8, 16), {}, "backbone", ((2, 64, 64), (1, 128, 64)), "body.layer3.0.conv2.weight",
         "body.layer2.0.bn1.running_var", ALL),
    # every map of a depth-4 U-Net at 128 x 128 is at least 8 x 8: no 3 x bf16 record reads a dgrad layout, so the default
    # arithmetic splits its rebuild too (at 64 x 64 only bfloat16_regs and bfloat16 do)
    Arch("unet_f16_128", "UNet", (3, 1, 16), {}, "seg", ((1, 128, 128), (1, 16, 16)), "decoder3.conv.conv.0.weight", None,
         ("fused_step", "shape_round_trip", "profile_during_step", "three_steps")),
    # the other classes of the U-Net family share UNet's refresh code: the step events only
    Arch("unet_bigger_f8", "UNetBigger", (3, 1, 8), {}, "seg", ((1, 32, 32),), "decoder3.conv.conv.0.weight", None,
         ("fused_step", "three_steps")),
    Arch("unet_overfit_f8", "UNetOverfit", (3, 1, 8), {}, "seg", ((1, 32, 32),), "decoder3.conv.conv.0.weight", None,
         ("fused_step", "three_steps")),
    Arch("unet_leaky_f16", "UNetDifferentActivation", (3, 1, 16, 0.1), {}, "seg", ((2, 32, 32),), "decoder3.conv.conv.0.weight", None,
         ("fused_step", "three_steps")),
)
BY_ID = {a.id: a for a in ARCHS}

HAS_LOSS = ("seg", "mask")
HAS_BACKWARD_ONLY = ("mask", "rpn", "box", "backbone")
# what train_step raises where the loss lives outside the model (the message of the library's check that fires first)
FUSED_ERROR = {"rpn": "defined for out_channels == 1", "backbone": "labels: this model takes no label map",
               "box": r"BoxHead: the input is \[R, in_features\]"}

# name -> (changes the weights, the used model's earlier value a pass after a mutation must differ from)
PASSES = OrderedDict((
    ("eval", (False, "eval")),            # eval(): forward
    ("fb", (False, "train")),             # train(): forward + backward
    ("backward_only", (False, "eval")),   # eval(): the forward pass the backward entry point requires, then backward from a given dout
    ("fused", (True, "train")),           # train(): train_step
    ("split", (True, "train")),           # train(): forward + backward, then apply_gradients
    ("accum", (True, "train")),           # train(): accumulate_gradients around two backward passes, then apply_gradients
))
MUTATING_OPS = ("load_partial", "load_full")
TOGGLE_OPS = ("mode", "overlap", "profile")

EVENTS = ("fused_step", "separate_apply", "partial_load", "full_load", "shape_round_trip", "overlap_off",
          "overlap_off_after_step", "overlap_on_again", "profile_during_step", "three_steps")


def _p(name, s=0, *flags):
    return ("pass", name, s) + flags


def scripts(arch):
    """{event: ops} of one row (every event of EVENTS the row runs; "mode_round_trip" is built per pair by mode_script)"""
    step = "fused" if arch.kind in HAS_LOSS else "split"
    base = [_p("eval", 0, "base"), _p("fb", 0, "base")]
    raises = [] if arch.kind in HAS_LOSS else [("fused_raises",)]
    out = OrderedDict()
    # (a) an inference forward, then (b) a training pass: with a split rebuild the inference forward starts the side-stream
    # half and the later backward pass consumes it; (c) the backward-only entry points straight after another step
    out["fused_step"] = base + raises + [_p(step), _p("eval"), _p("fb")]
    if arch.kind in HAS_BACKWARD_ONLY:
        out["fused_step"] += [_p(step), _p("backward_only")]
    out["separate_apply"] = base + [_p("split"), _p("fb"), _p("accum"), _p("fb")]
    out["partial_load"] = base + [("load_partial", "weight"), _p("fb"), _p("eval")]
    if arch.frozen:
        out["partial_load"] += [("load_partial", "frozen"), _p("fb"), _p("eval")]
    out["full_load"] = base + [("load_full",), _p("eval"), _p("fb")]
    if len(arch.shapes) > 1:
        out["shape_round_trip"] = base + [_p("eval", 1, "base"), _p("fb", 1, "base"), _p(step, 0), _p("fb", 1), _p("eval", 1),
                                          _p(step, 1), _p("fb", 0), _p("eval", 0)]
    out["overlap_off"] = [("overlap", False)] + base + [_p(step), _p("eval"), _p("fb")]
    out["overlap_off_after_step"] = base + [_p(step), ("overlap", False), _p("fb"), _p("eval")]
    out["overlap_on_again"] = [("overlap", False)] + base + [_p(step), ("overlap", True), _p("fb"), _p("eval")]
    out["profile_during_step"] = base + [("profile", True), _p(step), ("profile", False), _p("fb"), _p("eval")]
    out["three_steps"] = base + [_p(step), _p(step), _p(step), _p("fb"), _p("eval")]
    if arch.events != ALL:
        out = OrderedDict((k, v) for k, v in out.items() if k in arch.events)
    return out


def mode_script(arch):
    """Build the copies of mode A, change the weights in mode B, compare in A: the copies of A were valid once."""
    step = "fused" if arch.kind in HAS_LOSS else "split"
    return [("mode", "A"), _p("eval", 0, "base"), _p("fb", 0, "base"), ("mode", "B"), _p(step), ("mode", "A"), _p("fb"), _p("eval")]


MODE_PAIRS = tuple((a, b) for a in MODES for b in MODES if a != b)


def check_script(ops):
    """Every mutation is followed -- with nothing but switches in between -- by a compared pass, and the script ends with a
    compared pass that changes nothing.  Returns the number of compared passes."""
    compared = 0
    pending = False
    for op in ops:
        if op[0] == "pass":
            assert op[1] in PASSES, op
            if "base" in op[3:]:
                assert not pending and not PASSES[op[1]][0], ("a base pass after a mutation, or a mutating base pass", op)
            else:
                compared += 1
                pending = False
            pending = pending or PASSES[op[1]][0]
        elif op[0] in MUTATING_OPS:
            pending = True
        else:
            assert op[0] in TOGGLE_OPS or op[0] == "fused_raises", op
    assert not pending, "the script ends with a mutation no compared pass has seen"
    last = [op for op in ops if op[0] == "pass"][-1]
    assert "base" not in last[3:] and not PASSES[last[1]][0], last
    return compared


# ------------------------------------------------------------------------------------------------ inputs (host only)
_INPUTS = {}


def inputs(arch, s, batch=0):
    """The batch of shape `s`: seg / mask (x NHWC, y uint8 labels of the output map); rpn [(x, dout) per level]; box (x, dout);
    backbone (x, [dP2 .. dP6]).  Built once and never written."""
    key = (arch.id, s, batch)
    if key in _INPUTS:
        return _INPUTS[key]
    rng = np.random.default_rng([ARCHS.index(arch), s, batch, 20240])
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    shape = arch.shapes[s]
    if arch.kind in ("seg", "mask"):
        n, h, w = shape
        up = 2 if arch.kind == "mask" else 1
        v = (f32(n, h, w, arch.args[0]), (rng.random((n, up * h, up * w)) > 0.7).astype(np.uint8))
    elif arch.kind == "rpn":
        c, a = arch.args
        v = [(f32(n, h, w, c), 0.1 * f32(n, h, w, 5 * a)) for n, h, w in shape]
    elif arch.kind == "box":
        c, res, _, k1 = arch.args
        v = (f32(shape[0], res, res, c), 0.1 * f32(shape[0], 5 * k1))
    else:
        n, h, w = shape
        v = (f32(n, h, w, arch.args[0]), [0.1 * f32(n, h >> (2 + i), w >> (2 + i), arch.args[2]) for i in range(5)])
    _INPUTS[key] = v
    return v


def mask_dout(arch, s):
    """the mask head's backward-only entry point: a given gradient of its (n, 2 h, 2 w, 1) logits"""
    key = (arch.id, s, "dout")
    if key not in _INPUTS:
        n, h, w = arch.shapes[s]
        rng = np.random.default_rng([ARCHS.index(arch), s, 20241])
        _INPUTS[key] = (0.1 * rng.standard_normal((n, 2 * h, 2 * w, arch.args[1]))).astype(np.float32)
    return _INPUTS[key]


def perturb_one(w, grad=None):
    """The negative control: ONE element times (1 + 2^-6), in float32.  -> (flat index, new array).
    Which element: to first order the loss moves by dL/dw_i * w_i * 2^-6.  A float32 loss near 1 has ulps of 1.2e-7, and for
    most elements of a filter with 10^4 .. 10^5 of them that product is below one ulp (measured: the element of largest
    magnitude left the float32-mode losses of seven of the thirteen rows unchanged to the bit, with every gradient changed).
    So the element is the one with the largest |grad_i * w_i|, `grad` being the used model's own gradient of the filter; without
    a gradient, the element of largest magnitude."""
    w = np.array(w, dtype=np.float32, copy=True)
    score = np.abs(w) if grad is None else np.abs(np.asarray(grad, np.float64).reshape(w.shape) * w)
    i = int(np.argmax(score))
    w.reshape(-1)[i] = w.reshape(-1)[i] * PERTURB
    return i, w


def bf16_round(x):
    """float32 -> nearest-even bfloat16, as float32 (integer arithmetic on the bit patterns; finite inputs)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


# ------------------------------------------------------------------------------------------------ adapters (need the GPU)
PARAM_KINDS = ("conv_w", "conv_b", "bn_g", "bn_b")
Snap = namedtuple("Snap", "state adam step training")


def _cls(arch):
    from rfi_toolbox_amd import models
    return getattr(models, arch.cls)


def _base():
    from rfi_toolbox_amd.models import HipSegmenter
    return HipSegmenter


def _frozen(arch, name):
    return arch.kind == "backbone" and (".bn" in name or "downsample.1" in name)


def table_names(arch, m):
    """parameters by their names in the library's table: what adam_state / load_adam_state take"""
    return [n for n, _, k in m._entries if k in PARAM_KINDS and not _frozen(arch, n)]


def grad_names(arch, m):
    """parameters by the names grad() takes (the RPN and box heads split their stacked output layer at the Python boundary)"""
    return list(m.state_dict().keys()) if arch.kind in ("rpn", "box") else table_names(arch, m)


def below_mid(arch, m):
    """the conv filters before `arch.mid` in forward order"""
    convs = [n for n, shape, k in m._entries if k == "conv_w" and len(shape) == 4]
    return convs[:convs.index(arch.mid)]


def table_state(m):
    return _base().state_dict(m)


def table_load(m, sd):
    """load_state_dict(sd, strict=False) with the library's own names (the public one of every class but the RPN / box heads)"""
    return _base().load_state_dict(m, sd, strict=False)


def build(arch, mode, snap=None, seed=None):
    """A new instance; with `snap`: the twin (same state, Adam moments and step, train / eval flag)"""
    import torch
    if seed is not None:
        torch.manual_seed(seed)
    m = _cls(arch)(*arch.args, **arch.kwargs).set_compute_dtype(mode)
    if snap is not None:
        m.train(snap.training)
        m.load_state_dict(snap.state)
        for k, (mm, vv) in snap.adam.items():
            m.load_adam_state(k, mm, vv)
        m.set_adam_step(snap.step)
    return m


def snapshot(arch, m):
    adam, step = OrderedDict(), 0
    for k in table_names(arch, m):
        mm, vv, step = m.adam_state(k)
        adam[k] = (mm, vv)
    return Snap(m.state_dict(), adam, step, m.training)


def _np(v):
    return v.numpy() if hasattr(v, "numpy") else np.asarray(v)


def _backward_dlogits(m, x, dout, n, h, w):
    import ctypes as C
    from rfi_toolbox_amd._lib import HOST, check, lib
    x, dout = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(dout, np.float32)
    check(lib.rfi_model_backward_dlogits(m._h, x.ctypes.data_as(C.c_void_p), HOST, dout.ctypes.data_as(C.c_void_p), HOST, n, h, w))


def _forward(arch, m, data):
    if arch.kind == "rpn":
        return np.concatenate([m.forward_nhwc(x).ravel() for x, _ in data])
    if arch.kind == "box":
        return m.forward_rois(data[0])
    if arch.kind == "backbone":
        return np.concatenate([f.ravel() for f in m.forward_features(data[0])])
    return m.forward_nhwc(data[0])


def _forward_backward(arch, m, data, out, tag=""):
    """one forward + backward pass into `out`: loss (where the model has one), output, input gradient (where it has one)"""
    if arch.kind in HAS_LOSS:
        x, y = data
        out[tag + "loss"] = np.float32(m.forward_backward(x, y))
        out[tag + "out"] = m.debug_tensor("logits")
        if arch.kind == "mask":
            out[tag + "input_grad"] = m.input_grad(x.shape)
    elif arch.kind == "rpn":
        # one head over two pyramid levels: the parameter gradients of the two backward passes are summed
        outs, gxs = [], []
        m.accumulate_gradients("begin")
        for x, dout in data:
            outs.append(m.forward_nhwc(x).ravel())
            m.backward(x, dout)
            gxs.append(m.input_grad(x.shape).ravel())
            m.accumulate_gradients("add")
        m.accumulate_gradients("end")
        out[tag + "out"], out[tag + "input_grad"] = np.concatenate(outs), np.concatenate(gxs)
    elif arch.kind == "box":
        x, dout = data
        out[tag + "out"] = m.forward_rois(x)
        m.backward(x, dout)
        out[tag + "input_grad"] = m.input_grad(x.shape)
    else:
        x, dfe = data
        out[tag + "out"] = np.concatenate([f.ravel() for f in m.forward_features(x)])
        m.backward(x, dfe)


def _grads(arch, m, out):
    for k in grad_names(arch, m):
        out["grad:" + k] = m.grad(k)


def _state(arch, m, out):
    for k, v in m.state_dict().items():
        out["state:" + k] = _np(v)
    step = 0
    for k in table_names(arch, m):
        out["adam_m:" + k], out["adam_v:" + k], step = m.adam_state(k)
    out["adam_step"] = np.int64(step)


def run_pass(arch, m, name, s):
    """One call of PASSES on the batch of shape `s` -> {what: array}, everything the call returns or leaves behind"""
    data = inputs(arch, s)
    out = OrderedDict()
    if name == "eval":
        m.eval()
        out["out"] = _forward(arch, m, data)
        return out
    if name == "backward_only":
        m.eval()
        if arch.kind == "mask":
            x, y = data
            n, h, w, _ = x.shape
            dout = mask_dout(arch, s)
            out["out"] = m.forward_nhwc(x)
            _backward_dlogits(m, x, dout, n, h, w)
            out["input_grad"] = m.input_grad(x.shape)
        else:
            _forward_backward(arch, m, data, out)
        _grads(arch, m, out)
        return out
    m.train()
    if name == "fused":
        x, y = data
        out["loss"] = np.float32(m.train_step(x, y, **STEP))
        out["out"] = m.debug_tensor("logits")
        if arch.kind == "mask":
            out["input_grad"] = m.input_grad(x.shape)
    elif name == "accum":
        m.accumulate_gradients("begin")
        for b in (0, 1):
            if arch.kind == "rpn":              # (its pass accumulates over the levels itself: one level per pass here)
                x, dout = inputs(arch, s)[b]
                out[f"b{b}.out"] = m.forward_nhwc(x)
                m.backward(x, dout)
                out[f"b{b}.input_grad"] = m.input_grad(x.shape)
            else:
                _forward_backward(arch, m, inputs(arch, s, b), out, f"b{b}.")
            m.accumulate_gradients("add")
        m.accumulate_gradients("end")
        if "b0.loss" in out:
            out["loss"] = out["b0.loss"]
        out["out"] = np.concatenate([out["b0.out"].ravel(), out["b1.out"].ravel()]) if arch.kind == "rpn" else out["b0.out"]
    else:
        _forward_backward(arch, m, data, out)
    _grads(arch, m, out)
    if name in ("split", "accum"):
        out["grad_norm"] = np.float32(m.apply_gradients(**STEP))
    if PASSES[name][0]:
        _state(arch, m, out)
    return out


def primary(arch, got):
    """the bytes a mutation must change: the loss and the output of the forward direction"""
    return b"".join(np.ascontiguousarray(got[k]).tobytes() for k in ("loss", "out") if k in got)


def differing(got, want):
    """the keys whose arrays are not byte-equal"""
    assert list(got) == list(want), (list(got)[:5], list(want)[:5])
    bad = []
    for k in got:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
            bad.append(k)
    return bad
