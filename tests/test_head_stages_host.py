"""No GPU: the stage checker of the detector heads (tests/head_stages.py) on its float32 CPU stand-in.

test_standin_passes            the stand-in passes the whole stage table of every (case, mode): every row checked, every tensor
                               finite, exact zeros present in the stored raw outputs (the dead channels)
test_standin_against_oracle    its loss, logits and gradients agree with oracle/mask_head_ref.py (loss_and_grads; rpn_forward +
                               rpn_loss_torch; BoxHeadModule + fastrcnn_loss_torch) at test_gpu_mask_head.py's tolerances: the
                               stage table is tied to the oracle
test_mutation[...]             a wrong stand-in fails, in the rows head_stages.MUTATIONS names and in no other; and what the
                               whole-head criteria of test_gpu_mask_head.py say of the same tensors is the table below
test_relu_ge_needs_exact_zeros with the modules' default initialisation (what test_gpu_mask_head.py draws) `>=` and `>` give the
                               same bits: no test of values can tell them apart there
test_gate_coverage             the union of gate_values over the cases is ALL_GATE_VALUES; the issue's cases and sequences
test_stage_table               every row reads only what was written before it

WHAT THE WHOLE-HEAD CRITERIA SEE (``head_stages.whole_head_notices``: test_gradients_vs_oracle's max(4 rel_ref, 1e-3) for the mask
head, 1e-4 / 2e-4 of a norm for the RPN / box head, test_bf16_operand_mode's max(1.1 rel_arith, 1e-2) in "bfloat16"), evaluated on
the mutated stand-in at THIS module's cases, and whether test_gpu_mask_head.py runs a configuration where the mutation can show:

  mutation                    stage rows that turn red             whole-head criterion   configuration in test_gpu_mask_head.py
  head_da_overwritten         head_bwd                             notices                box head only (2e-4 of a norm); never the
                                                                                          RPN head in float32_mfma or a mask head K > 1
  relu_bwd_ge                 head_bwd, up_bwd, conv_bwd.<i>       notices, given zeros   none: default initialisation stores no exact
                                                                                          zero, the wrong build is bit-identical there
  bias_before_mask            up_bwd, conv_bwd.<i> (the :db rows)  notices                every head
  convt_taps_swapped          up                                   notices                mask head
  rpn_rows_swapped            head                                 notices                RPN head, float32 only
  fc6_chw                     conv.0                               notices                box head, float32 only
  operand_truncation          every contraction row                notices                mask head only (no RPN / box head in bfloat16)
  box_rows_permuted           conv.0                               notices                box head, float32 only
  truncation_in_one_launch    conv_bwd.0                           GREEN on all 5 runs    --

A wrong value everywhere is within reach of a norm criterion once the configuration is run; the stage table adds the configurations
(mode x head form x depth x map size x layout), names the launch, and holds each launch to float32 rounding, which is what it takes
to see one launch truncate.
"""
import functools
import re

import numpy as np
import pytest

import head_stages as H
import unet_bf16_stages as S


@functools.lru_cache(maxsize=None)
def _setup(cid):
    c = H.BY_ID[cid]
    st, P = H.init_params(c)
    return c, st, P, H.inputs(c)


def _run(cid, mode, mutate=None):
    c, st, P, inp = _setup(cid)
    si = H.StandIn(c, mode, P, inp, mutate)
    return si, H.check(c, mode, P, si.run())


@pytest.mark.parametrize("cid,mode", H.RUNS)
def test_standin_passes(cid, mode):
    _, ck = _run(cid, mode)
    for line in ck.report():
        print(line)
    assert ck.unchecked_rows() == []
    assert ck.nonfinite == [] and ck.undecided == 0
    assert ck.zeros > 0
    assert not ck.failures(), [(f.stage, f.tensor, f.ratio, f.detail) for f in ck.failures()][:8]
    assert {f.klass for f in ck.findings} == {"f32", "sums", "loss" if H.own_loss(ck.c) else "elem"}
    assert set(ck.oracle) == set(H.keys(ck.c))                   # every parameter's gradient has a row


@pytest.mark.parametrize("cid,mode", H.RUNS)
def test_standin_against_oracle(cid, mode):
    c, st, P, inp = _setup(cid)
    si, _ = _run(cid, mode)
    assert H.whole_head_notices(c, mode, st, inp, si.T, si.loss) == []


# ------------------------------------------------------------------------------------------------------------ mutations
F32, MF, BF = H.F32, H.MF, H.BF
MUTATION_RUNS = {
    "head_da_overwritten": [("mask_c12_k3_l2_2x10x6", F32), ("mask_c16_k8_l1_1x7x7", MF), ("rpn_c16_a4_l1_2x8x8", MF),
                            ("box_c16_r7_h64_k2_96", F32), ("box_c8_r3_h32_k5_37", BF)],
    "relu_bwd_ge": [("mask_c16_k1_l4_5x14x14", F32), ("rpn_c32_a4_l2_1x24x20", F32), ("box_c16_r7_h64_k2_96", F32),
                    ("mask_c32_k1_l2_3x14x14", BF)],
    "bias_before_mask": [("mask_c16_k1_l4_5x14x14", F32), ("rpn_c16_a4_l1_2x8x8", F32), ("box_c8_r3_h32_k5_37", F32),
                         ("mask_c32_k1_l2_3x14x14", BF)],
    "convt_taps_swapped": [("mask_c16_k1_l4_5x14x14", F32), ("mask_c32_k1_l2_3x14x14", BF), ("mask_c16_k8_l1_1x7x7", F32)],
    "rpn_rows_swapped": [("rpn_c16_a4_l1_2x8x8", F32), ("rpn_c16_a8_l1_2x1x1", F32), ("rpn_c16_a4_l1_2x8x8", BF)],
    "fc6_chw": [("box_c16_r7_h64_k2_96", F32), ("box_c8_r3_h32_k5_37", BF), ("box_c4_r3_h36_k2_33", F32)],
    "operand_truncation": [("mask_c32_k1_l2_3x14x14", BF), ("mask_c16_k8_l1_1x7x7", BF), ("rpn_c16_a4_l1_2x8x8", BF),
                           ("box_c16_r7_h64_k2_96", BF), ("box_c8_r3_h32_k5_37", BF)],
    "box_rows_permuted": [("box_c16_r7_h64_k2_96", F32), ("box_c16_r7_h64_k2_96", BF)],
    "truncation_in_one_launch": [("mask_c32_k1_l2_3x14x14", BF), ("mask_c16_k8_l1_1x7x7", BF), ("rpn_c16_a4_l1_2x8x8", BF),
                                 ("box_c16_r7_h64_k2_96", BF), ("box_c8_r3_h32_k5_37", BF)],
}
# the docstring's third column: does the whole-head criterion flag anything on the mutated stand-in
OLD_CRITERION_NOTICES = {k: k != "truncation_in_one_launch" for k in MUTATION_RUNS}
# the rows of each kind a mutation may touch (":da" the masked input gradients, ":db" the bias gradients)
ROW_KIND = {"relu_bwd_ge": ":da", "bias_before_mask": ":db", "head_da_overwritten": ":da", "truncation_in_one_launch": ":da"}


@pytest.mark.parametrize("mut,cid,mode", [(m, c, md) for m, runs in MUTATION_RUNS.items() for c, md in runs])
def test_mutation(mut, cid, mode):
    c, st, P, inp = _setup(cid)
    si, ck = _run(cid, mode, mut)
    stages = ck.failed_stages()
    print("MUTATION %s %s/%s red: %s" % (mut, cid, mode, stages))
    assert stages, "the mutation went unnoticed"
    rx = H.MUTATIONS[mut][1]
    assert all(re.search(rx, s) for s in stages), (stages, rx)
    if mut in ROW_KIND:
        assert all(f.stage.endswith(ROW_KIND[mut]) for f in ck.failures()), [f.stage for f in ck.failures()]
    if mut == "operand_truncation":                               # every contraction of the pass, forward and backward
        assert {"conv.0", "conv_bwd.0"} <= set(stages)
    if mut == "relu_bwd_ge":
        assert "head_bwd" in stages and ck.zeros > 0
    old = H.whole_head_notices(c, mode, st, inp, si.T, si.loss)
    print("MUTATION %s %s/%s whole-head criterion: %s" % (mut, cid, mode, old or "green"))
    assert bool(old) == OLD_CRITERION_NOTICES[mut], old


def test_every_mutation_has_runs():
    assert list(MUTATION_RUNS) == list(H.MUTATIONS)


@pytest.mark.parametrize("cid", ["mask_c16_k1_l4_5x14x14", "rpn_c32_a4_l2_1x24x20", "box_c16_r7_h64_k2_96"])
def test_relu_ge_needs_exact_zeros(cid):
    c = H.BY_ID[cid]
    _, P = H.init_params(c, dead=False)
    inp = H.inputs(c)
    a, b = H.StandIn(c, F32, P, inp).run(), H.StandIn(c, F32, P, inp, "relu_bwd_ge").run()
    assert all(np.array_equal(a[k], b[k]) for k in H.tensor_names(c)) and all(np.array_equal(a["grad"][k], b["grad"][k]) for k in a["grad"])
    assert H.check(c, F32, P, a).zeros == 0


# ------------------------------------------------------------------------------------------------------------ the tables
def test_gate_coverage():
    hit = set()
    for c in H.CASES:
        values = H.gate_values(c)
        assert not [v for v in c.covers if v not in values], (c.id, sorted(values))
        hit |= values
    assert hit == set(H.ALL_GATE_VALUES), sorted(hit ^ set(H.ALL_GATE_VALUES))
    # the issue's cases: (head, args, shape, modes)
    want = [("mask", (16, 1, 4), (5, 14, 14), (F32, MF)), ("mask", (32, 1, 2), (3, 14, 14), (F32, BF)), ("mask", (8, 1, 1), (2, 14, 14), (F32,)),
            ("mask", (12, 3, 2), (2, 10, 6), (F32,)), ("mask", (16, 8, 1), (1, 7, 7), (F32, BF, MF)), ("mask", (64, 1, 8), (1, 8, 8), (F32,)),
            ("rpn", (16, 4, 1), (2, 8, 8), (F32, MF, BF)), ("rpn", (32, 4, 2), (1, 24, 20), (F32,)), ("rpn", (8, 4, 1), (2, 4, 4), (F32,)),
            ("rpn", (16, 8, 1), (2, 1, 1), (F32,)), ("rpn", (16, 8, 1), (2, 2, 2), (F32,)),
            ("box", (16, 7, 64, 2), (96,), (F32, MF, BF)), ("box", (8, 3, 32, 5), (37,), (F32, BF)), ("box", (4, 1, 4, 2), (1,), (F32,)),
            ("box", (4, 3, 36, 2), (31,), (F32,)), ("box", (4, 3, 36, 2), (32,), (F32,)), ("box", (4, 3, 36, 2), (33,), (F32,))]
    assert [(c.head, c.args, c.shape, c.modes) for c in H.CASES] == want
    assert [s for _, s in H.SEQUENCES.values()] == [[(5, 14, 14), (37, 14, 14), (1, 14, 14), (5, 14, 14)], [(96,), (37,), (1,), (96,)],
                                                   [(2, 16, 16), (2, 8, 8), (2, 1, 1), (2, 16, 16)]]
    assert [H.BY_ID[b].args for b, _ in H.SEQUENCES.values()] == [(16, 1, 4), (16, 7, 64, 2), (16, 4, 1)]
    assert (H.EPS, H.K_CONTRACTION) == (S.EPS, 16.0) and H.Criteria is S.Criteria and H.wgrad_stage is S.wgrad_stage
    # both sides of head_on_mfma() are taken by one width
    r = H.BY_ID["rpn_c16_a4_l1_2x8x8"]
    assert H.head_on_mfma(r, F32) and H.head_on_mfma(r, BF) and not H.head_on_mfma(r, MF)


@pytest.mark.parametrize("cid,mode", H.RUNS)
def test_stage_table(cid, mode):
    c = H.BY_ID[cid]
    rows = H.stage_table(c, mode)
    written = {"x"} | set(H.keys(c))
    for r in rows:
        assert r.klass in ("f32", "sums", "loss", "elem")
        for t in r.ins:
            assert t.startswith("(") or t in written, (r.stage, t, "read before it is written")
        written |= set(r.outs)
    assert set(H.tensor_names(c)) <= written and {"grad " + k for k in H.keys(c)} <= written
    L = H.depth(c)
    assert len(rows) == L + 2 + 3 + 3 * L + (4 if c.head == "mask" else 0)
    assert len({r.stage for r in rows}) == len(rows) and rows[0].stage == "conv.0" and rows[-1].outs == ["dx"]
    for name in H.tensor_names(c):
        assert len(H.shape_of(c, name)) == 4
