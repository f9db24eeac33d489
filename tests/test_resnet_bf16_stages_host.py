"""No GPU: the stage checker of the ResNet-encoder U-Net's bfloat16 data flow (tests/resnet_bf16_stages.py) on its float32 CPU stand-in.

test_standin_passes            the stand-in passes the whole stage table on every case with zero undecided masks, and has ties
test_standin_against_oracle    its loss, logits and gradients agree with resnet_unet_ref under unet_ref.bf16_operands(round_outputs=True)
                               to the bounds test_gpu_resnet_unet.py holds the device to: the new oracle is tied to the old
test_mutation_*                a wrong stand-in fails, in the mutated row(s) only (a wrong dz_<b> is carried into block b - 1's
                               composite rows: the module docstring says why)
test_gate_coverage             every gate value is reached by a case; each case's `covers` is true of it
test_stage_table               the table names only tensors the checker reads, in launch order
"""
import functools

import numpy as np
import pytest

import resnet_bf16_stages as R
import unet_bf16_stages as S


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = R.BY_ID[cid]
    x, y = R.inputs(c)
    return c, R.init_state(c), x, y


def _run(cid, mutate=None):
    c, st, x, y = _inputs(cid)
    si = R.StandIn(c, st, x.numpy(), y.numpy(), mutate)
    return si, R.check(c, st, si.run())


@pytest.mark.parametrize("cid", list(R.BY_ID))
def test_standin_passes(cid):
    _, ck = _run(cid)
    for line in ck.report():
        print(line)
    assert ck.undecided == 0, "a ReLU mask is undecided at this seed: pick another"
    assert ck.tie_windows > 0
    assert not ck.failures(), [(f.stage, f.tensor, f.ratio, f.detail) for f in ck.failures()][:8]
    assert {f.klass for f in ck.findings} >= {"elem", "conv16", "f32", "sums", "stats", "pad", "composite"}
    # all 20 encoder weight gradients have a row
    assert len({f.tensor for f in ck.findings if f.klass == "f32" and f.tensor.endswith(".weight")}) == R.N_ENC_CONVS


@pytest.mark.parametrize("cid", list(R.BY_ID))
def test_standin_against_oracle(cid):
    c, st, x, y = _inputs(cid)
    si, _ = _run(cid)
    assert R.whole_model_notices(c, st, x, y, si.T, si.loss) == []


# ------------------------------------------------------------------------------------------------------------ mutations
def _fails_in(cid, mutate, first, also=()):
    """The mutation is noticed: in stage `first`, and nowhere but there and in `also`."""
    _, ck = _run(cid, mutate)
    assert ck.failures(), "the mutation went unnoticed"
    stages = ck.failed_stages()
    assert first in stages and set(stages) <= {first, *also}, (stages, [(f.stage, f.tensor, f.ratio) for f in ck.failures()][:6])
    return ck


def _carried(b):
    """A wrong dz_<b> shows in block b's BatchNorm rows and is carried into block b - 1's (stride-1 b only)."""
    own = ["block%d.bn2" % b] + (["block%d.bnd" % b] if b in (2, 4, 6) else [])
    if b in (2, 4, 6):
        return own
    return own + (["block0.dz(composite)"] if b == 1 else ["block%d.bn2" % (b - 1), "block%d.bnd" % (b - 1)])


@pytest.mark.parametrize("cid,b", [("f16_1x32x48", 0), ("f16_3x16x16", 2), ("f32_2x32x32", 5), ("f64_1x32x32", 6)])
def test_mutation_bn_add_relu16_truncates(cid, b):
    ck = _fails_in(cid, {"round:rA.%d" % b: S.trunc_bf16}, "block%d.bn_add_relu16" % b)
    assert {f.tensor for f in ck.failures()} == {"rA.%d" % b}


@pytest.mark.parametrize("cid,b", [("f16_3x16x16", 6), ("f32_2x32x32", 2), ("f64_1x32x32", 6), ("f16_1x32x48", 4)])
def test_mutation_class0_without_the_projection_segment(cid, b):
    stages = _carried(b - 1)
    _fails_in(cid, {"classes:%d" % b: lambda acc, main: main}, stages[0], stages[1:])


@pytest.mark.parametrize("cid,b", [("f16_3x16x16", 6), ("f16_1x32x48", 2), ("f32_2x32x32", 4), ("f64_1x32x32", 6)])
def test_mutation_two_parity_classes_swapped(cid, b):
    def swap(acc, main):
        out = acc.copy()
        out[:, 0::2, 1::2], out[:, 1::2, 0::2] = acc[:, 1::2, 0::2], acc[:, 0::2, 1::2]      # (ooy, oox) of classes 1 and 2
        return out
    stages = _carried(b - 1)
    _fails_in(cid, {"classes:%d" % b: swap}, stages[0], stages[1:])


@pytest.mark.parametrize("cid,b", [("f16_1x32x48", 1), ("f16_3x16x16", 5), ("f32_2x32x32", 3), ("f64_1x32x32", 5)])
def test_mutation_relu_mask_sum16_drops_the_skip_gradient(cid, b):
    """The third term: a float32 view (widths 16) or a bfloat16 view (widths 32, 64) of dconcat."""
    stages = _carried(b)
    _fails_in(cid, {"terms:%d" % b: lambda terms: terms[:1]}, stages[0], stages[1:])


@pytest.mark.parametrize("cid,b", [("f16_1x32x48", 2), ("f16_3x16x16", 6), ("f64_1x32x32", 4)])
def test_mutation_stride2_conv_reads_the_wrong_rows(cid, b):
    """Row 2 y + r instead of 2 y + r - 1: the halo shifted by one row."""
    ck = _fails_in(cid, {"halo:rY1.%d" % b: lambda p: (1, 1, 0, 2)}, "block%d.conv1" % b)
    assert {f.tensor for f in ck.failures()} == {"rY1.%d" % b}


@pytest.mark.parametrize("cid", list(R.BY_ID))
def test_mutation_folded_sums_of_the_unrounded_values(cid):
    ck = _fails_in(cid, {"sums_source:dA1.0": lambda dA1, acc: acc}, "block0.bn1")
    assert all(f.klass == "sums" for f in ck.failures())


@pytest.mark.parametrize("cid", list(R.BY_ID))
def test_mutation_pool_backward_routes_ties_to_the_last_maximum(cid):
    def last(arg, windows):
        return 3 - windows[..., ::-1].argmax(-1)
    stages = _carried(7)
    ck = _fails_in(cid, {"route": last}, stages[0], stages[1:])
    assert ck.tie_windows > 0


def test_mutation_one_padding_lane():
    def lane(v):
        v = v.copy()
        v[v.shape[0] // 2, -1] = 2.0 ** -126
        return v
    for when in ("pad_fwd", "pad_bwd"):
        ck = _fails_in("f16_3x16x16", {"pad:%s:xin" % when: lane}, when)
        assert [f.tensor for f in ck.failures()] == ["xin:pad"]


# ------------------------------------------------------------------------------------------------------------ the tables
def test_gate_coverage():
    hit = {}
    for c in R.CASES:
        values = R.gate_values(c)
        missing = [v for v in c.covers if v not in values]
        assert not missing, (c.id, missing, sorted(values))
        for v in values:
            hit.setdefault(v, []).append(c.id)
    for v in R.ALL_GATE_VALUES:
        assert hit.get(v), "no case reaches " + v
    # the issue's cases, by (feat, n, h, w), and its reshape run
    assert [(c.feat, c.n, c.h, c.w) for c in R.CASES] == [(16, 1, 32, 48), (16, 3, 16, 16), (32, 2, 32, 32), (64, 1, 32, 32)]
    assert all(c.feat % 16 == 0 and c.h % 16 == 0 and c.w % 16 == 0 and c.in_ch == 3 and c.depth == 4 for c in R.CASES)
    assert R.RESHAPE_SEQUENCE == [(1, 32, 64), (1, 16, 32), (1, 32, 64)]
    assert (S.K_CONTRACTION, S.K_ELEM) == (16.0, 4.0) and R.K_CONTRACTION is S.K_CONTRACTION


@pytest.mark.parametrize("cid", list(R.BY_ID))
def test_stage_table(cid):
    c = R.BY_ID[cid]
    rows = R.stage_table(c)
    known = set(R.tensor_names(c)) | {"x"} | {"chan.%d" % i for i in range(R.N_ENC_CONVS)} | {"dconcat.%d" % l for l in range(1, 5)}
    written = {"x"}
    for launch, ins, outs, kind in rows:
        assert kind.split(":")[0] in ("direct", "composite", "unreachable", "tests/unet_bf16_stages.py"), kind
        for t in ins:
            if t.startswith("("):
                continue
            assert t in known and t in written, (launch, t, "unknown or read before it is written")
        for t in outs:
            if t in known:
                written.add(t)
    assert set(R.tensor_names(c)) <= written, sorted(set(R.tensor_names(c)) - written)
    assert sum("class" in r[0] for r in rows) == 12 and sum(r[0].startswith("pwgrad") for r in rows) == R.N_ENC_CONVS
    assert rows[0][0] == "act_split" and rows[-1][0] == "pwgrad stem"
    # every stored tensor of the table has the shape the reader gives it
    for name in R.tensor_names(c):
        assert len(R.shape_of(c, name)) == 4
