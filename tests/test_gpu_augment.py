"""-m gpu: the augmentation kernel (csrc/augment.hip) against the NumPy oracle tests/augment_ref.py, its exact cases
(flip-only samples, all gates off, host vs device inputs, repeated calls), and train_rfi_model(augment=True)."""
import numpy as np
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(5, 16, 24, 3),        # baseline
          (3, 17, 9, 8),         # odd sizes, 16-byte path
          (2, 1, 7, 1),          # H = 1: reflect period 0
          (4, 12, 12, 5),        # generic channel count, scalar tail
          (64, 32, 32, 3)]       # many workgroups, about 18 flip-only samples
SEED, CALL = 7, 3
_cache = {}


def _case(shape):
    """inputs, oracle output and the device output of one shape (computed once, shared by the tests, never written)"""
    if shape not in _cache:
        from rfi_toolbox_amd.training import Augmenter
        x, y = R.inputs(shape)
        p = R.draw(*shape[:3], seed=SEED, call=CALL)
        want = R.warp(x, y, p)
        gx, gy = Augmenter(seed=SEED)(x, y, call=CALL)
        _cache[shape] = (x, y, p, want, (gx.numpy(), gy.numpy()))
    return _cache[shape]


def _flip_only(p):
    return np.flatnonzero((p["gates"][:, 2] == 0) & (p["gates"][:, 3] == 0))


def _flipped(a, gates):
    return a[::-1 if gates[1] else 1, ::-1 if gates[0] else 1]


@pytest.mark.parametrize("shape", SHAPES)
def test_matches_oracle(shape):
    x, y, p, (wx, wy, ties), (gx, gy) = _case(shape)
    assert gx.shape == x.shape and gx.dtype == np.float32 and gy.shape == y.shape and gy.dtype == np.uint8
    err, bound = np.abs(gx.astype(np.float64) - wx).max(), 2.0 ** -23 * np.abs(x).max()
    share = ties.mean()
    mism = int(((gy != wy) & ~ties).sum())
    print(f"{shape}: image error {err:.3e} (bound {bound:.3e}); tie share {share:.2e}; mask mismatches off ties {mism}")
    assert err <= bound           # one float32 rounding of a convex combination formed in fp64
    assert share <= 1e-3
    assert mism == 0
    assert set(np.unique(gy)) <= {0, 1, 2, 255}


def test_flip_only_samples_are_bit_exact_copies():
    x, y, p, _, (gx, gy) = _case((64, 32, 32, 3))
    sel = _flip_only(p)
    assert 8 <= len(sel) <= 32 and len({tuple(g) for g in p["gates"][sel, :2]}) == 4      # every flip combination occurs
    for i in sel:
        assert np.array_equal(gx[i].view(np.uint32), _flipped(x[i], p["gates"][i]).view(np.uint32))
        assert np.array_equal(gy[i], _flipped(y[i], p["gates"][i]))


def test_flip_only_samples_copy_non_finite_values():
    from rfi_toolbox_amd.training import Augmenter
    for shape in [(64, 32, 32, 3), (24, 9, 11, 8)]:
        x, y = R.inputs(shape)
        x = x.copy()
        x[:, 0, 0, 0], x[:, -1, 2, -1], x[:, 3, -1, 0] = np.inf, np.nan, -np.inf
        x.view(np.uint32)[:, 2, 2, 0] = 0x7FC01234                                        # a NaN with a payload
        p = R.draw(*shape[:3], seed=SEED, call=CALL)
        gx, gy = Augmenter(seed=SEED)(x, y, call=CALL)
        gx = gx.numpy()
        sel = _flip_only(p)
        assert len(sel) >= 3
        for i in sel:
            assert np.array_equal(gx[i].view(np.uint32), _flipped(x[i], p["gates"][i]).view(np.uint32))


@pytest.mark.parametrize("shape", [(5, 16, 24, 3), (3, 17, 9, 8), (4, 12, 12, 5)])
def test_host_device_and_repeated_calls_agree_bitwise(shape):
    from rfi_toolbox_amd.runtime import Context
    from rfi_toolbox_amd.training import Augmenter
    x, y, _, _, (gx, gy) = _case(shape)
    ctx = Context.get(0)
    aug = Augmenter(seed=SEED)
    dx, dy = ctx.to_device(x), ctx.to_device(y)
    for src in ((dx, dy), (dx, dy), (torch.from_numpy(x), torch.from_numpy(y)), (torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())):
        ox, oy = aug(*src, call=CALL)
        assert np.array_equal(ox.numpy().view(np.uint32), gx.view(np.uint32)) and np.array_equal(oy.numpy(), gy)
    assert np.array_equal(dx.numpy(), x) and np.array_equal(dy.numpy(), y)                # the inputs are untouched
    other, _ = aug(dx, dy, call=CALL + 1)
    assert not np.array_equal(other.numpy(), gx)


@pytest.mark.parametrize("shape", SHAPES)
def test_all_gates_off_returns_the_input(shape):
    from rfi_toolbox_amd.training import Augmenter
    x, y = _case(shape)[:2]
    ox, oy = Augmenter(seed=SEED, p_hflip=0, p_vflip=0, p_rotate=0, p_ssr=0)(x, y, call=CALL)
    assert np.array_equal(ox.numpy().view(np.uint32), x.view(np.uint32)) and np.array_equal(oy.numpy(), y)


def test_empty_batch_and_library_argument_checks():
    from rfi_toolbox_amd._lib import RfiHipError
    from rfi_toolbox_amd.training import Augmenter
    ox, oy = Augmenter()(np.zeros((0, 8, 8, 3), np.float32), np.zeros((0, 8, 8), np.uint8))
    assert ox.shape == (0, 8, 8, 3) and oy.shape == (0, 8, 8)
    a = Augmenter()
    a.p_rotate = 2.0                                          # past the constructor: the library checks as well
    with pytest.raises(RfiHipError, match="probabilities"):
        a(np.zeros((1, 8, 8, 3), np.float32), np.zeros((1, 8, 8), np.uint8))


def test_train_rfi_model_with_augmentation():
    from rfi_toolbox_amd.models import UNet
    from rfi_toolbox_amd.training import Augmenter, train_rfi_model
    g = torch.Generator().manual_seed(12)
    x = torch.randn(8, 32, 32, 3, generator=g)
    y = (torch.rand(8, 32, 32, generator=g) > 0.7).to(torch.uint8)
    vx = torch.randn(4, 32, 32, 3, generator=g)
    vy = (torch.rand(4, 32, 32, generator=g) > 0.7).to(torch.uint8)

    def model():
        torch.manual_seed(33)
        return UNet(3, 1, 4)

    def run(**kw):
        m = model()
        torch.manual_seed(99)                                 # the shuffle
        return m, train_rfi_model(m, (x, y), (vx, vy), num_epochs=2, batch_size=4, lr=1e-3, log=lambda s: None, **kw)

    m_aug, h_aug = run(augment=True, augment_seed=5)
    _, h_plain = run()
    _, h_false = run(augment=False, augment_seed=5)
    assert h_plain == h_false

    m = model()                                               # the same loop by hand
    torch.manual_seed(99)
    aug, by_hand = Augmenter(seed=5), []
    for e in range(2):
        m.train()
        order = torch.randperm(8).numpy()
        losses = []
        for b in range(2):
            sel = order[4 * b:4 * b + 4]
            ax, ay = aug(x[sel], y[sel], call=(e << 32) | b)
            losses.append(m.train_step(ax, ay, lr=1e-3, weight_decay=1e-5))
        m.eval()
        by_hand.append((float(np.mean(losses)), float(m.loss(vx, vy))))
    assert [(r["train_loss"], r["val_loss"]) for r in h_aug] == by_hand                   # bit-equal histories
    assert [r["train_loss"] for r in h_aug] != [r["train_loss"] for r in h_plain]
    m_aug.eval()
    assert h_aug[-1]["val_loss"] == float(m_aug.loss(vx, vy))                             # validation on the raw arrays
