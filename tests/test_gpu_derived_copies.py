"""-m gpu: the derived filter copies follow the weights, bit for bit ("Derived filter copies: who invalidates, who
rebuilds"; tables, adapters and scripts: tests/derived_copy_cases.py).

A copy that lags the parameters by one optimiser step moves a gradient by about lr relative, inside every oracle tolerance
of the suite.  Here a USED model runs a script of events and, at every compared pass, a TWIN -- a new instance of the same
class, arguments, compute mode and train / eval flag, given the used model's state_dict, Adam moments and Adam step of
just before the call -- makes the same single call on the same inputs.  The twin builds every copy from scratch; loss,
logits or feature maps, every grad(k), input_grad and, after a step, every state_dict entry and Adam moment are compared
as bytes.  After every mutation the used model's loss / output must differ from its own value of before the mutation on
the same batch (same mode, same shape), so the mutation is in sight of the comparison.

test_event            every row of ARCHS x every mode x every event script (fused step; separate apply and accumulated
                      gradients; partial load; full load; shape round trip; the four stream / profile conditions; three
                      steps in a row)
test_mode_round_trip  every row x every ordered pair of modes: copies of A built, weights changed in B, compared in A
test_negative_control every row x mode: one element of a mid-network filter of a twin times (1 + 2^-6) -- the loss (the
                      output, where the loss lives outside the model) and a gradient below that layer are no longer equal

Combinations that raise by design (asserted by the "fused_raises" op, then the step is forward + backward + apply_gradients):
    RPNHead x every mode x fused_step:      train_step -> "loss: ... defined for out_channels == 1"
    BoxHead x every mode x fused_step:      train_step -> "BoxHead: the input is [R, in_features]"
    ResNet50FPN x every mode x fused_step:  train_step -> "labels: this model takes no label map"
The mask head's backward-only entry point has no Python method: the test calls rfi_model_backward_dlogits as MaskRCNN does.

What the scripts found when they were written (both fixed with them):
  * shape_round_trip, op 5 ("fb" at 1x16x16 after passes at the larger shape), unet_f16 and unet_f16_128, bfloat16 and
    float32_planes: loss, logits and all 80 gradients differed from the twin.  No stale filter copy -- a result that depended
    on history: plane tensors are grow-only, the plane kernels point out-of-image lanes at the 64 bytes behind the tensor
    of the shape in use, and inside the allocation of a larger shape those bytes held its activations.  PlaneBuf::ensure
    zeroes them again when the shape in use changes.
  * fused_step, backbone, every mode: train_step on a ResNet50FPN copied the label map into a 64-byte buffer
    (hipMemcpyAsync refused it with "invalid argument", which then surfaced at the next launch of the next model); the
    label staging now checks its size and raises the error listed above.
No derived filter copy was found stale: every event x mode x network was byte-equal to its twin after these two fixes.

What the shape round trip of the other rows found (fixed with them):
  * shape_round_trip, op 5 ("fb" at 1x16x48 after a step at 2x32x32), unet_in4_f32, float32: the 20 gradients below the
    bottleneck's second conv differed from the twin -- a stale copy.  At 32x32 no 3 x bf16 record of this model reads a dgrad
    layout, so the forward pass left the dgrad layouts to the side stream; at 16x48 the bottleneck's maps are under 8 x 8, the
    record list of the new shape splits its dgrad layouts, and it did so before they were rebuilt.  UNetModel::wd_split_ok now
    splits the rebuild only while the record list is the prepared shape's.
"""
import numpy as np
import pytest

import derived_copy_cases as D
from rfi_toolbox_amd.runtime import Context

pytestmark = pytest.mark.gpu


class Used:
    """the used model of one test and what it remembers of its own earlier passes"""

    def __init__(self, arch, mode):
        self.arch, self.mode = arch, mode
        self.m = D.build(arch, mode, seed=1000 + D.ARCHS.index(arch))
        self.prev = {}                # (train | eval, shape, mode) -> (loss + output bytes, mutations so far)
        self.mutations = 0
        self.fb_grads = {}            # shape -> the gradients of the last forward + backward pass there
        self.must_differ = None       # set by a partial load: (shape-independent) names whose gradients must change

    def run(self, ops, modes=None):
        ctx = Context.get(0)
        try:
            for i, op in enumerate(ops):
                self.step(ctx, i, op, modes)
        finally:
            ctx.set_overlap(True)
            ctx.profile(False)
            ctx.profile_reset()

    def step(self, ctx, i, op, modes):
        arch, m = self.arch, self.m
        if op[0] == "overlap":
            ctx.set_overlap(op[1])
        elif op[0] == "profile":
            ctx.profile(op[1])
        elif op[0] == "mode":
            self.mode = modes[op[1]]
            m.set_compute_dtype(self.mode)
        elif op[0] == "fused_raises":
            x = D.inputs(arch, 0)[0][0] if arch.kind == "rpn" else D.inputs(arch, 0)[0]
            with pytest.raises(RuntimeError, match=D.FUSED_ERROR[arch.kind]):
                m.train().train_step(x, np.zeros(x.shape[:3], np.uint8), **D.STEP)
        elif op[0] == "load_partial":
            key = arch.mid if op[1] == "weight" else arch.frozen
            old = D.table_state(m)[key].numpy()
            rng = np.random.default_rng(77)
            new = old * (1.0 + 0.25 * rng.standard_normal(old.shape)) if op[1] == "weight" else old * 1.5 + 0.25
            D.table_load(m, {key: new.astype(np.float32)})
            self.mutations += 1
            self.must_differ = D.below_mid(arch, m) if op[1] == "weight" else None
        elif op[0] == "load_full":
            rng = np.random.default_rng(78)
            sd = m.state_dict()
            for k, v in sd.items():
                if v.ndim >= 2:
                    sd[k] = v.numpy() * (1.0 + 0.1 * rng.standard_normal(tuple(v.shape))).astype(np.float32)
            m.load_state_dict(sd)
            self.mutations += 1
        else:
            self.compared_pass(i, op)

    def compared_pass(self, i, op):
        arch, m = self.arch, self.m
        name, s, base = op[1], op[2], "base" in op[3:]
        where = (arch.id, self.mode, i, op)
        snap = None if base else D.snapshot(arch, m)
        got = D.run_pass(arch, m, name, s)
        if not base:
            twin = D.build(arch, self.mode, snap)
            want = D.run_pass(arch, twin, name, s)
            del twin
            bad = D.differing(got, want)
            assert not bad, (where, len(bad), bad[:6])
        # the mutation is visible in the forward direction
        mutates, probe = D.PASSES[name]
        key, now = (probe, s, self.mode), D.primary(arch, got)
        if key in self.prev:
            before, at = self.prev[key]
            if at != self.mutations:
                assert before != now, (where, "loss and output are what they were before the mutation")
        else:
            assert self.mutations == 0, (where, "no value of before the mutation to compare with")
        self.prev[key] = (now, self.mutations)
        if name == "fb":
            grads = {k[5:]: v for k, v in got.items() if k.startswith("grad:")}
            if self.must_differ is not None:      # the dgrad-direction copies of the loaded layer are in the comparison's sight
                same = [k for k in self.must_differ if np.array_equal(grads[k], self.fb_grads[s][k])]
                assert not same, (where, "gradients below the loaded layer did not change", same)
                self.must_differ = None
            self.fb_grads[s] = grads
        if mutates:
            self.mutations += 1


EVENT_CASES = [(a.id, mode, ev) for a in D.ARCHS for mode in D.MODES for ev in D.scripts(a)]


@pytest.mark.parametrize("arch_id,mode,event", EVENT_CASES, ids=lambda v: v)
def test_event(arch_id, mode, event):
    arch = D.BY_ID[arch_id]
    Used(arch, mode).run(D.scripts(arch)[event])


MODE_CASES = [(a.id, ma, mb) for a in D.ARCHS if a.events == D.ALL for ma, mb in D.MODE_PAIRS]


@pytest.mark.parametrize("arch_id,mode_a,mode_b", MODE_CASES, ids=lambda v: v)
def test_mode_round_trip(arch_id, mode_a, mode_b):
    arch = D.BY_ID[arch_id]
    Used(arch, mode_a).run(D.mode_script(arch), {"A": mode_a, "B": mode_b})


@pytest.mark.parametrize("mode", D.MODES)
@pytest.mark.parametrize("arch", D.ARCHS, ids=lambda a: a.id)
def test_negative_control(arch, mode):
    """The comparison can fail: a twin with ONE filter element of the mid-network layer times (1 + 2^-6) no longer gives the
    used model's loss (output, for the models whose loss lives outside) nor its gradients below that layer.  The element is
    the one with the largest first-order effect on the loss (derived_copy_cases.perturb_one says why); the passes are
    deterministic, so the float32 loss moves by the same 2 (resnet18_f16) to 30 ulps in every run."""
    u = Used(arch, mode)
    snap = D.snapshot(arch, u.m)
    twin = D.build(arch, mode, snap)
    got = D.run_pass(arch, u.m, "fb", 0)
    w, g = D.table_state(twin)[arch.mid].numpy(), u.m.grad(arch.mid)
    idx, w2 = D.perturb_one(w, g)
    assert D.bf16_round(w2.reshape(-1)[idx:idx + 1]) != D.bf16_round(w.reshape(-1)[idx:idx + 1])
    D.table_load(twin, {arch.mid: w2})
    want = D.run_pass(arch, twin, "fb", 0)
    bad = D.differing(got, want)
    first = "loss" if arch.kind in D.HAS_LOSS else "out"
    below = ["grad:" + k for k in D.below_mid(arch, u.m)]
    predicted = float(g.reshape(-1)[idx]) * float(w.reshape(-1)[idx]) * 2.0 ** -6
    print(f"\nDERIVEDCTL {arch.id} {mode} differing={len(bad)}/{len(got)} {first}: {got[first].ravel()[:1]} vs {want[first].ravel()[:1]} "
          f"first-order change {predicted:.2e} below differing={sum(k in bad for k in below)}/{len(below)}")
    assert first in bad, (arch.id, mode, "the perturbed twin returns the same " + first)
    assert below and any(k in bad for k in below), (arch.id, mode, "no gradient below the perturbed layer changed")
