"""-m gpu: the plain U-Net's bfloat16 data flow stage by stage on the device's own tensors (tests/unet_bf16_stages.py states the
method, the stage table, the criteria, the measured table and the mutation record).

test_bf16_stages[case]            one forward pass (padding lanes read), one forward_backward, every tensor read back through
                                  UNet.debug_tensor, the whole stage table checked; zero undecided masks / routes
test_bf16_stages_after_reshape    one model at 1x48x80, 1x24x40, 1x48x80: the second and third runs are stage-checked
                                  (PlaneBuf::ensure's zero area and the padding lanes after a shape change)
test_debug_tensor_names           what the debug path refuses: unknown names, levels out of range, :pad of a float32 tensor, and on
                                  the ResNet-encoder U-Net every tensor the bfloat16 mode stores as bfloat16
"""
import numpy as np
import pytest
import torch

import unet_bf16_stages as S
from rfi_toolbox_amd.models import UNet, UNetResNet18

pytestmark = pytest.mark.gpu


def _model(c, state):
    cls = UNet
    if c.slope:
        cls = type("UNetLeaky", (UNet,), {"negative_slope": float(c.slope)})        # (UNet._create reads the attribute)
    return cls(c.in_ch, 1, c.feat, depth=c.depth).load_state_dict(state).train().set_compute_dtype("bfloat16")


def _run(c, m, state, n=None, h=None, w=None, seed_offset=0):
    x, y = S.inputs(c, n, h, w, seed_offset)
    m.forward_nhwc(x.numpy())                            # (train mode: batch statistics) -> the padding lanes after a forward pass
    pads = S.read_pads(m, c, forward_only=True)
    m.forward_backward(x, y)
    T = S.read_device(m, c, x.numpy(), n, h, w, pads=pads)
    ck = S.check(c, state, T)
    for line in ck.report():
        print(line)
    print("UNETBF16 %s undecided %d operand_undecided %d tie_windows %d" % (c.id, ck.undecided, ck.operand_undecided, ck.tie_windows))
    for f in ck.failures():
        print("UNETBF16-FAIL %s %s %s %s %.4g > %.4g %s" % (c.id, f.stage, f.klass, f.tensor, f.ratio, f.limit, f.detail))
    return ck


@pytest.mark.parametrize("cid", list(S.BY_ID))
def test_bf16_stages(cid):
    c = S.BY_ID[cid]
    state = S.init_state(c)
    ck = _run(c, _model(c, state), state)
    assert ck.undecided == 0, "a ReLU mask or a pooling route is undecided at this seed: pick another"
    if not c.slope:
        assert ck.tie_windows > 0                         # exact ties at the maximum (ReLU zeros): routed to the first one
    assert not ck.failures(), ck.failed_stages()


def test_bf16_stages_after_reshape():
    c = S.BY_ID[S.RESHAPE_BASE]
    state = S.init_state(c)
    m = _model(c, state)
    for k, (n, h, w) in enumerate(S.RESHAPE_SEQUENCE):
        if k == 0:
            x, y = S.inputs(c, n, h, w, 10)
            m.forward_backward(x, y)
            continue
        ck = _run(c, m, state, n, h, w, 10 + k)
        assert ck.undecided == 0
        assert not ck.failures(), (k, ck.failed_stages())


def test_debug_tensor_names():
    c = S.BY_ID["f20_d1_1x16x24"]
    state = S.init_state(c)
    m = _model(c, state)
    x, y = S.inputs(c)
    m.forward_backward(x, y)
    for bad in ("nonsense", "skip.0", "skip.2", "skip", "upin.1", "logits:pad", "dconcat.1:pad", "gB.1:pad"):
        with pytest.raises(RuntimeError):
            m.debug_tensor(bad)
    assert m.debug_tensor("skip.1").size == 16 * 24 * 20 and m.debug_tensor("skip.1:pad").size == 16 * 24 * 12
    assert m.debug_tensor("encY1.1:pad").size == 16 * 24 * 12 and m.debug_tensor("xin:pad").size == 16 * 24 * 13
    # the float32 modes keep their tensors and have no plane tensors
    m32 = UNet(3, 1, 20, depth=1).load_state_dict(state).train()
    m32.forward_backward(x, y)
    assert m32.debug_tensor("encY1.1").size == 16 * 24 * 20
    with pytest.raises(RuntimeError):
        m32.debug_tensor("skip.1")
    # float32 by three bf16 pieces: the same names, the sum of the pieces
    m3 = UNet(3, 1, 20, depth=1).load_state_dict(state).train().set_compute_dtype("float32_planes")
    m3.forward_backward(x, y)
    assert np.array_equal(m3.debug_tensor("xin").reshape(16, 24, 3), x.numpy()[0])       # (three pieces carry a float32 value exactly)
    assert not m3.debug_tensor("skip.1:pad").any() and m3.debug_tensor("skip.1").size == 16 * 24 * 20
    # the ResNet-encoder U-Net exposes its decoder's float32 tensors under these names (its encoder's bfloat16 tensors have names
    # of their own: test_gpu_resnet_bf16_stages.py): what the bfloat16 mode stores as bfloat16 is refused
    # (width 32: all three gates), and so are the tensors its own encoder replaces; dconcat is converted on a host read
    g = torch.Generator().manual_seed(5)
    xr = torch.randn(1, 32, 32, 3, generator=g)
    yr = (torch.rand(1, 32, 32, generator=g) > 0.7).to(torch.uint8)
    mr = UNetResNet18(3, 1, 32).train().set_compute_dtype("bfloat16")
    mr.forward_backward(xr, yr)
    for bad in ("decY1.1", "decY2.1", "decY2.2", "bottY1", "bottY2", "gB.1", "gBottA", "gBottB", "encY1.1", "pool.1"):
        with pytest.raises(RuntimeError):
            mr.debug_tensor(bad)
    dcat = mr.debug_tensor("dconcat.1")
    assert dcat.size == 32 * 32 * 64 and S.is_bf16(dcat).all() and dcat.any()
    assert mr.debug_tensor("concat.1").size == 32 * 32 * 64
