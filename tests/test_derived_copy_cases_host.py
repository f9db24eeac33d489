"""The tables and scripts of tests/derived_copy_cases.py, without a GPU: every script ends each mutation with a compared
pass, every HipSegmenter class and every compute mode is in the tables, and the negative control's perturbation survives
bfloat16 rounding."""
import inspect
import re

import numpy as np
import pytest
import torch

import derived_copy_cases as D
from rfi_toolbox_amd import models
from rfi_toolbox_amd.models import HipSegmenter


def _all_scripts():
    for a in D.ARCHS:
        for ev, ops in D.scripts(a).items():
            yield a, ev, ops
        yield a, "mode_round_trip", D.mode_script(a)


def test_every_script_ends_each_mutation_with_a_compared_pass():
    n = 0
    for a, ev, ops in _all_scripts():
        try:
            compared = D.check_script(ops)
        except AssertionError as e:
            raise AssertionError((a.id, ev, e.args))
        assert compared >= 2, (a.id, ev)
        # the value a pass after a mutation must differ from exists: a base pass of the same kind, shape and mode comes first
        seen, mode = set(), "A"
        for i, op in enumerate(ops):
            if op[0] == "mode":
                mode = op[1]
            if op[0] == "pass":
                key = (D.PASSES[op[1]][1], op[2], mode)
                mutated = any(o[0] in D.MUTATING_OPS or (o[0] == "pass" and D.PASSES[o[1]][0]) for o in ops[:i])
                assert key in seen or not mutated, (a.id, ev, op)
                seen.add(key)
        n += 1
    assert n >= len(D.ARCHS) * 3


def test_the_checker_rejects_a_script_without_the_closing_pass():
    for bad in ([("pass", "eval", 0, "base"), ("pass", "fused", 0)],
                [("pass", "eval", 0, "base"), ("load_full",)],
                [("pass", "eval", 0, "base"), ("load_full",), ("pass", "fb", 0, "base")],
                [("pass", "eval", 0, "base"), ("pass", "fused", 0), ("pass", "fb", 0), ("load_partial", "weight")]):
        with pytest.raises(AssertionError):
            D.check_script(bad)


def test_issue_rows_run_every_event():
    full = {a.id: a for a in D.ARCHS if a.events == D.ALL}
    assert {(a.cls, a.args) for a in full.values()} == {
        ("UNet", (3, 1, 16)), ("UNet", (4, 1, 32)), ("UNet", (3, 1, 6)), ("UNetResNet18", (3, 1, 16)), ("SimpleCNN", (3, 1, 64)),
        ("MaskHead", (16, 1, 4)), ("RPNHead", (16, 4)), ("BoxHead", (16, 7, 64, 2)), ("ResNet50FPN", (3, 8, 16))}
    assert full["unet_f16"].shapes == ((2, 64, 64), (1, 16, 16))
    assert full["backbone"].shapes == ((2, 64, 64), (1, 128, 64))
    assert full["rpn_head"].shapes == (((2, 16, 16), (2, 8, 8)), ((1, 32, 32), (1, 16, 16)))
    # every class with a prepare_shape of its own goes through the shape round trip: a second shape that changes every buffer's size
    assert {a.id: a.shapes[1] for a in full.values() if a.id not in ("unet_f16", "backbone", "rpn_head")} == {
        "unet_in4_f32": (1, 16, 48), "unet_f6": (1, 16, 48), "resnet18_f16": (1, 32, 32), "cnn_w64": (1, 16, 48),
        "mask_head": (10, 14, 14), "box_head": (50,)}
    for a in full.values():
        assert len(a.shapes) == 2, a.id
        want = set(D.EVENTS) - (set() if len(a.shapes) > 1 else {"shape_round_trip"})
        assert set(D.scripts(a)) == want, a.id
    for a in D.ARCHS:
        assert set(D.scripts(a)) <= set(D.EVENTS) and D.scripts(a), a.id
    assert len(D.MODE_PAIRS) == len(D.MODES) * (len(D.MODES) - 1)


def test_every_segmenter_class_is_in_the_table():
    classes = {n for n, c in vars(models).items() if inspect.isclass(c) and issubclass(c, HipSegmenter) and c is not HipSegmenter}
    assert classes and classes == {a.cls for a in D.ARCHS}
    for a in D.ARCHS:
        names = [e[0] for e in _entries(a)]
        assert a.mid in names and (a.frozen is None or a.frozen in names), a.id
        convs = [e[0] for e in _entries(a) if e[2] == "conv_w" and len(e[1]) == 4]
        assert 0 < convs.index(a.mid) < len(convs) - 1 or a.kind == "rpn", a.id     # (the RPN head has two layers)
        assert a.kind in ("seg", "mask", "rpn", "box", "backbone")
        assert (a.kind in D.HAS_LOSS) != (a.kind in D.FUSED_ERROR)


def _entries(a):
    """the parameter table of a row, from the host-side entry functions (no model is constructed)"""
    if a.cls.startswith("UNet") and a.cls != "UNetResNet18":
        depth = a.kwargs.get("depth", 5 if a.cls in ("UNetBigger", "UNetOverfit") else 4)
        return models.unet_entries(*a.args[:3], depth)
    if a.cls == "UNetResNet18":
        return models.resnet_unet_entries(*a.args)
    if a.cls == "SimpleCNN":
        return models.simple_cnn_entries(*a.args)
    if a.cls == "MaskHead":
        return models.mask_head_entries(*a.args)
    if a.cls == "RPNHead":
        return models.rpn_head_entries(*a.args)
    if a.cls == "ResNet50FPN":
        return models.resnet50_fpn_entries(*a.args)
    c, res, hid, k1 = a.args
    return [("fc6.weight", (hid, c * res * res, 1, 1), "conv_w"), ("fc7.weight", (hid, hid, 1, 1), "conv_w"),
            ("head.weight", (5 * k1, hid, 1, 1), "conv_w")]


def test_every_mode_string_is_used():
    src = inspect.getsource(HipSegmenter.set_compute_dtype)
    table = re.search(r"code = \{(.*?)\}", src, re.S).group(1)
    by_code = {}
    for name, code in re.findall(r'"(\w+)":\s*(\d)', table):
        by_code.setdefault(int(code), set()).add(name)
    assert len(by_code) == 5
    for code, names in by_code.items():
        assert names & set(D.MODES), (code, names)
    assert set(D.MODES) <= set().union(*by_code.values())
    # every row runs every mode: the GPU file's parameters are the product
    import test_gpu_derived_copies as G
    assert {(a, m) for a, m, _ in G.EVENT_CASES} == {(a.id, m) for a in D.ARCHS for m in D.MODES}


def test_inputs_are_fixed_and_shaped():
    for a in D.ARCHS:
        for s in range(len(a.shapes)):
            v, again = D.inputs(a, s), D.inputs(a, s)
            assert v is again
        if a.kind in ("seg", "mask"):
            x, y = D.inputs(a, 0)
            n, h, w = a.shapes[0]
            up = 2 if a.kind == "mask" else 1
            assert x.shape == (n, h, w, a.args[0]) and x.dtype == np.float32 and y.shape == (n, up * h, up * w) and y.dtype == np.uint8
            assert 0 < y.mean() < 1
            assert not np.array_equal(D.inputs(a, 0, 1)[0], x)
    assert D.mask_dout(D.BY_ID["mask_head"], 0).shape == (6, 28, 28, 1)


def test_the_perturbation_changes_the_bfloat16_rounding():
    """(1 + 2^-6) moves a float32 value by 2^-6 relative, two bfloat16 ulps or more (8 significand bits: one ulp is at most
    2^-7 relative), so the element differs after rounding to bfloat16 as well."""
    rng = np.random.default_rng(5)
    w = np.concatenate([rng.standard_normal(4096) * 0.1, [1.0, 1.9921875, 0.99609375, 2.0 ** -20, -3.0e-3, 1.0 + 2.0 ** -8, 1.0 - 2.0 ** -9],
                        np.float32(1.0) + np.arange(256) * np.float32(2.0 ** -8)]).astype(np.float32)
    w2 = (w * D.PERTURB).astype(np.float32)
    assert np.all(D.bf16_round(w2) != D.bf16_round(w))
    # bf16_round is torch's conversion
    assert np.array_equal(D.bf16_round(w), torch.from_numpy(w).to(torch.bfloat16).float().numpy())
    for shape in ((4, 3, 3, 3), (7,)):
        a = rng.standard_normal(shape).astype(np.float32)
        i, b = D.perturb_one(a)
        assert i == int(np.argmax(np.abs(a))) and (a != b).sum() == 1 and b.reshape(-1)[i] == a.reshape(-1)[i] * D.PERTURB
        g = rng.standard_normal(a.size).astype(np.float32)              # (a gradient in any shape of the same size)
        j, c = D.perturb_one(a, g)
        assert j == int(np.argmax(np.abs(g.astype(np.float64) * a.reshape(-1)))) and (a != c).sum() == 1
        assert c.reshape(-1)[j] == a.reshape(-1)[j] * D.PERTURB
