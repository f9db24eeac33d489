"""No GPU: the stage checker of the U-Net's bfloat16 data flow (tests/unet_bf16_stages.py) on its float32 CPU stand-in.

test_standin_passes            the stand-in passes the whole stage table on every case, with zero undecided masks / routes
test_standin_against_oracle    its loss, logits and gradients agree with unet_ref.bf16_operands(round_outputs=True) to the bounds
                               test_gpu_bf16.py::test_bf16_data_flow_other_shapes holds the device to: the new oracle is tied to the old
test_mutation_*                a wrong stand-in fails, and the failure names the mutated stage ONLY (teacher forcing: every later
                               stage reads the wrong tensor as its input and agrees with it)
test_gate_coverage             every gate value is reached by a case; each case's `covers` is true of it
test_stage_table               the table names only tensors the checker reads, in launch order
"""
import functools

import numpy as np
import pytest
import torch

import unet_bf16_stages as S
from oracle import unet_ref


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = S.BY_ID[cid]
    x, y = S.inputs(c)
    return c, S.init_state(c), x, y


def _run(cid, mutate=None):
    c, st, x, y = _inputs(cid)
    si = S.StandIn(c, st, x.numpy(), y.numpy(), mutate)
    return si, S.check(c, st, si.run())


@pytest.mark.parametrize("cid", list(S.BY_ID))
def test_standin_passes(cid):
    _, ck = _run(cid)
    for line in ck.report():
        print(line)
    assert ck.undecided == 0
    assert not ck.failures(), [(f.stage, f.tensor, f.ratio, f.detail) for f in ck.failures()]
    assert {f.klass for f in ck.findings} >= {"elem", "f32", "sums", "stats", "pad"}
    if not S.BY_ID[cid].slope:
        assert ck.tie_windows > 0


@pytest.mark.parametrize("cid", list(S.BY_ID))
def test_standin_against_oracle(cid):
    c, st, x, y = _inputs(cid)
    si, _ = _run(cid)
    T = si.T
    fwd = unet_ref.variant_forward(negative_slope=c.slope) if c.slope else None
    xo, yo = unet_ref.nhwc_to_nchw(x), y.float().unsqueeze(1)
    with unet_ref.bf16_operands(round_outputs=(c.feat % 4 == 0)):
        lb, lgb, gb, _ = unet_ref.loss_and_grads(st, xo, yo, forward_fn=fwd)
    l32, lg32, g32, _ = unet_ref.loss_and_grads(st, xo, yo, forward_fn=fwd)
    assert si.loss == pytest.approx(float(lb), rel=5e-3)
    want = lgb.permute(0, 2, 3, 1).reshape(-1).numpy()
    w32 = lg32.permute(0, 2, 3, 1).reshape(-1).numpy()
    span = float(np.abs(want).max())
    e_same, e_arith = np.abs(T["logits"].reshape(-1) - want), np.abs(w32 - want)
    assert e_same.max() <= max(0.75 * e_arith.max(), 5e-3 * span), (e_same.max(), e_arith.max(), span)
    assert np.median(e_same) <= max(0.6 * np.median(e_arith), 1e-3 * span)
    rels = []
    for k, gk in gb.items():
        if k.endswith((".0.bias", ".3.bias")) and "conv" in k:
            continue
        gk = gk.numpy().ravel()
        nrm = np.linalg.norm(gk) + 1e-30
        rel_same = np.linalg.norm(T["grad"][k].ravel() - gk) / nrm
        rel_arith = np.linalg.norm(g32[k].numpy().ravel() - gk) / nrm
        rels.append(rel_same / max(rel_arith, 1e-9))
        assert rel_same <= max(1.5 * rel_arith, 3e-2), (k, rel_same, rel_arith)
    assert np.median(rels) <= 1.0, np.median(rels)


# ------------------------------------------------------------------------------------------------------------ mutations
def _only(cid, mutate, stage):
    _, ck = _run(cid, mutate)
    assert ck.failures(), "the mutation went unnoticed"
    assert ck.failed_stages() == [stage], (ck.failed_stages(), [(f.stage, f.tensor, f.ratio) for f in ck.failures()][:6])
    return ck


def _other_neighbour_of_one(acc):
    """Round to nearest, but ONE element (a large one whose accumulator lies next to its bf16 value) to the other side."""
    r = S.rne(acc)
    ulp = S.ulp_bf16(r)
    d = np.where(np.abs(acc) >= np.median(np.abs(acc)), np.abs(acc.astype(np.float64) - r) / np.maximum(ulp, 1e-300), np.inf)
    i = np.unravel_index(int(d.argmin()), d.shape)
    r = r.copy()
    r[i] = np.float32(S.other_neighbour(r[i], float(acc[i])))
    assert S.is_bf16(r).all()
    return r


@pytest.mark.parametrize("cid,name,stage", [("f32_d2_1x24x40", "encY2.1", "enc1.conv2"), ("f16_d2_2x24x40", "up.2", "dec2.up"),
                                            ("f32_d2_1x24x40", "up.1", "dec1.up"), ("f16_d2_2x24x40", "gB.2", "enc2.dgrad2"),
                                            ("f32_d2_1x24x40", "dconcat.2", "dec2.dgrad1")])
def test_mutation_other_bf16_neighbour(cid, name, stage):
    ck = _only(cid, {"round:" + name: _other_neighbour_of_one}, stage)
    assert {f.tensor for f in ck.failures()} == {name}


@pytest.mark.parametrize("cid,name,stage", [
    ("f32_d2_1x24x40", "xin", "act_split(x)"), ("f20_d1_1x16x24", "a1e.1", "enc1.act_split"), ("f32_d2_1x24x40", "bottY1", "bott.conv1"),
    ("in5_f12_d2_3x16x16", "decY1.2", "dec2.conv1"), ("f16_d2_2x24x40", "up.1", "dec1.up"), ("f32_d2_1x24x40", "up.2", "dec2.up"),
    ("f20_d1_1x16x24", "up.1", "dec1.act_split(upf)"), ("f16_d2_2x24x40", "dpool.1", "enc2.dgrad1"), ("f16_d2_2x24x40", "gA.2", "enc2.pool_bwd_merge"),
    ("f32_d2_1x24x40", "gBottA", "dec2.up"), ("f32_d2_1x24x40", "dYaE.1", "enc1.bn_bwd2"), ("in1_f8_d3_1x32x32", "dYbottB", "bott.bn_bwd1")])
def test_mutation_truncation(cid, name, stage):
    """Truncation to bf16 instead of round-to-nearest-even in ONE stage."""
    _only(cid, {"round:" + name: S.trunc_bf16}, stage)


@pytest.mark.parametrize("name,stage", [("gB_dec.1", "dec1.bn_bwd1"), ("gA_dec.2", "dec2.bn_bwd2")])
def test_mutation_truncation_of_an_unreadable_gradient(name, stage):
    """The decoder's gB / gA are overwritten within the pass: a truncating producer shows in the BatchNorm backward that reads them."""
    _only("f32_d2_1x24x40", {"round:" + name: S.trunc_bf16}, stage)


@pytest.mark.parametrize("cid,name,stage", [("f32_d2_1x24x40", "encY2.1", "enc1.conv2"), ("f32_d2_1x24x40", "dconcat.1", "dec1.dgrad1"),
                                            ("f6_d1_1x16x24", "bottY2", "bott.conv2"), ("f32_d2_1x24x40", "up.1", "dec1.up")])
def test_mutation_last_column_dropped(cid, name, stage):
    def drop(v):
        v = v.copy()
        v[:, :, -1, :] = 0
        return v
    _only(cid, {"out:" + name: drop}, stage)


@pytest.mark.parametrize("cid,name,stage", [("f32_d2_1x24x40", "bottY1", "bott.conv1"), ("f20_d1_1x16x24", "encY2.1", "enc1.conv2"),
                                            ("f16_d2_2x24x40", "decY2.1", "dec1.conv2")])
def test_mutation_statistics_of_the_accumulators(cid, name, stage):
    """The conv epilogue sums the ROUNDED values; sums of the float32 accumulators are a different (wrong) answer."""
    ck = _only(cid, {"stats_source:" + name: lambda Y, acc: acc}, stage)
    assert all(f.klass in ("stats", "elem") for f in ck.failures())


def test_mutation_bias_gradient_of_the_stored_dy():
    """... and the conv-bias gradient is the sum of dY BEFORE its rounding: summing the stored bf16 values is caught too."""
    def hook(o, chan, gamma):
        return S.rne(o)                                       # (the stored values take the place of the float32 ones: same dY)
    ck = _only("f32_d2_1x24x40", {"dy32:dYaE.1": hook}, "enc1.bn_bwd2")
    assert {f.tensor for f in ck.failures()} == {"encoder1.conv.conv.3.bias"}


@pytest.mark.parametrize("cid,l", [("f32_d2_1x24x40", 1), ("f20_d1_1x16x24", 1), ("in1_f8_d3_1x32x32", 3)])
def test_mutation_tie_to_the_last_maximum(cid, l):
    def last(arg, windows):
        return 3 - windows[..., ::-1].argmax(-1)
    ck = _only(cid, {"route:%d" % l: last}, "enc%d.pool_bwd_merge" % l)
    assert ck.tie_windows > 0


@pytest.mark.parametrize("when,cid,name", [("pad_fwd", "f20_d1_1x16x24", "skip.1"), ("pad_bwd", "f20_d1_1x16x24", "skip.1"),
                                           ("pad_fwd", "in5_f12_d2_3x16x16", "xin"), ("pad_bwd", "in5_f12_d2_3x16x16", "xin"),
                                           ("pad_bwd", "f6_d1_1x16x24", "dYbottA"), ("pad_fwd", "f20_d1_1x16x24", "encY1.1"),
                                           ("pad_bwd", "f20_d1_1x16x24", "encY1.1")])
def test_mutation_one_padding_lane(when, cid, name):
    def lane(v):
        v = v.copy()
        v[v.shape[0] // 2, -1] = 2.0 ** -126
        return v
    ck = _only(cid, {"pad:%s:%s" % (when, name): lane}, when)
    assert [f.tensor for f in ck.failures()] == [name + ":pad"]


@pytest.mark.parametrize("cid,name,stage", [("f20_d1_1x16x24", "a1e.1", "enc1.act_split"), ("f20_d1_1x16x24", "skip.1", "enc1.bn_relu_pool_planes"),
                                            ("in5_f12_d2_3x16x16", "dYb.2", "dec2.bn_bwd1"), ("f20_d1_1x16x24", "decY1.1", "dec1.conv1"),
                                            ("f6_d1_1x16x24", "xin", "act_split(x)")])
def test_mutation_last_partial_chunk_channel_zeroed(cid, name, stage):
    def zero(v):
        v = v.copy()
        v[..., -1] = 0
        return v
    _only(cid, {"out:" + name: zero}, stage)


@pytest.mark.parametrize("cid,name,stage", [("f32_d2_1x24x40", "dYbE.1", "enc1.bn_bwd1"), ("f20_d1_1x16x24", "dYa.1", "dec1.bn_bwd2"),
                                            ("f32_d2_1x24x40", "dYb.2", "dec2.bn_bwd1")])
def test_mutation_dbeta_term_omitted(cid, name, stage):
    def no_c1(o, chan, gamma):
        return (o + (S.f32(gamma) * chan["invstd"]) * chan["c1"]).astype(np.float32)
    _only(cid, {"dy32:" + name: no_c1}, stage)


def test_undecided_elements_are_counted():
    """A pre-activation planted on the threshold and a pooling window with two nearly equal candidates are reported, not decided."""
    Y = np.array([[[[1.0, 2.0]], [[3.0, 4.0]]]], np.float32).reshape(1, 2, 2, 1)
    scale, shift = np.array([1.0]), np.array([-2.0 * (1 + 2.0 ** -24)])
    _, und = S.relu_mask(Y, scale, shift)
    assert und == 1
    Y2 = np.array([1.0, 1.0 + 2.0 ** -23, 0.5, 0.25], np.float32).reshape(1, 2, 2, 1)
    arg, und, ties = S.pool_routes(Y2, np.array([1.0]), np.array([0.0]), 0.0)
    assert (und, ties) == (1, 0)
    arg, und, ties = S.pool_routes(np.array([0.5, 1.0, 1.0, 0.25], np.float32).reshape(1, 2, 2, 1), np.array([1.0]), np.array([0.0]), 0.0)
    assert (int(arg[0, 0, 0, 0]), und, ties) == (1, 0, 1)      # an exact tie: decided, the first maximum in row-major order
    a, gap, und = S.operand_in_registers(np.array([1.0 + 2.0 ** -8], np.float32).reshape(1, 1, 1, 1), np.array([1.0]), np.array([0.0]), 0.0)
    assert und == 1 and gap.ravel()[0] == 2.0 ** -7            # halfway between two bf16 values: the gap widens what it feeds


def test_bf16_helpers():
    v = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -9, 3.0e-39], np.float32)
    want = torch.from_numpy(v).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(S.rne(v), want)                       # ties to even, both directions
    g = torch.Generator().manual_seed(0)
    r = (torch.randn(4096, generator=g) * 10 ** (torch.rand(4096, generator=g) * 8 - 4)).numpy()
    assert np.array_equal(S.rne(r), torch.from_numpy(r).to(torch.bfloat16).to(torch.float32).numpy())
    assert S.is_bf16(S.rne(r)).all() and S.is_bf16(S.trunc_bf16(r)).all() and (np.abs(S.trunc_bf16(r)) <= np.abs(r)).all()
    assert S.ulp_bf16(1.0) == 2.0 ** -7 and S.ulp_bf16(1.99) == 2.0 ** -7 and S.ulp_bf16(2.0) == 2.0 ** -6 and S.ulp_bf16(0.0) == 0.0


# ------------------------------------------------------------------------------------------------------------ the tables
def test_gate_coverage():
    hit = {}
    for c in S.CASES:
        values = S.gate_values(c)
        missing = [v for v in c.covers if v not in values]
        assert not missing, (c.id, missing, sorted(values))
        for v in values:
            hit.setdefault(v, []).append(c.id)
    for v in S.ALL_GATE_VALUES:
        assert hit.get(v), "no case reaches " + v
    assert len({c.id for c in S.CASES}) == len(S.CASES)
    for c in S.CASES:
        assert c.h % (1 << c.depth) == 0 and c.w % (1 << c.depth) == 0 and c.n * (c.h >> c.depth) * (c.w >> c.depth) >= 2, c.id
    # the issue's cases, by (in, feat, depth, n, h, w, slope)
    assert {(c.in_ch, c.feat, c.depth, c.n, c.h, c.w, c.slope) for c in S.CASES} == {
        (3, 32, 2, 1, 24, 40, 0.0), (3, 16, 2, 2, 24, 40, 0.0), (3, 20, 1, 1, 16, 24, 0.0), (5, 12, 2, 3, 16, 16, 0.0),
        (1, 8, 3, 1, 32, 32, 0.0), (3, 6, 1, 1, 16, 24, 0.0), (3, 32, 1, 1, 16, 24, 0.1), (4, 32, 1, 1, 16, 16, 0.0)}
    base = S.BY_ID[S.RESHAPE_BASE]
    assert S.gates(base)["ctp"] and S.RESHAPE_SEQUENCE == [(1, 48, 80), (1, 24, 40), (1, 48, 80)]


@pytest.mark.parametrize("cid", list(S.BY_ID))
def test_stage_table(cid):
    c = S.BY_ID[cid]
    rows = S.stage_table(c)
    known = set(S.tensor_names(c)) | {"x", "logits", "dlogits"} | {"chan.%d" % i for i in range(4 * c.depth + 2)}
    written = {"x"}
    for launch, ins, outs, gate in rows:
        for t in ins:
            t = t.split(":")[0].split(" ")[0]
            assert t in known, (launch, t)
            assert t in written or t.startswith(("gA.", "gB.")), (launch, t, "read before it is written")
        for t in outs:
            t = t.split(":")[0].split(" ")[0]
            if t in known:
                written.add(t)
    assert rows[0][0] == "act_split" and rows[-1][0].startswith("pwgrad enc1.conv1")
    # every stored tensor of the case is some launch's output
    assert set(S.tensor_names(c)) <= written, sorted(set(S.tensor_names(c)) - written)
    # the gates select the forms the table lists
    g = S.gates(c)
    assert any("zblocks" in r[0] for r in rows) == g["ctp"]
    assert any(r[0].startswith("act_split dec") and r[1][0].startswith("upf.") for r in rows) == any(
        (c.feat << (l - 1)) % 16 for l in range(1, c.depth + 1))
