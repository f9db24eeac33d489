"""No GPU: pins tests/family_step_cases.py -- the models and shapes of the whole-step test, the label bytes, the loss
definition against the float64 reference of tests/class_loss_ref.py, and the seeds' margin from the ReLU threshold."""
import numpy as np
import pytest
import torch

import class_loss_ref as R
import family_step_cases as F
from rfi_toolbox_amd.class_labels import unpack_class_bits


def test_case_table():
    assert [(c.in_ch, c.K, c.feat, c.depth, c.n, c.h, c.w) for c in F.CASES[:2]] == [(8, 5, 4, 2, 2, 8, 12), (3, 2, 8, 4, 2, 16, 16)]
    assert any(c.feat % 16 == 0 and c.K > 1 for c in F.CASES)
    for c in F.CASES:
        x, y = F.inputs(c)
        assert tuple(x.shape) == (c.n, c.h, c.w, c.in_ch) and y.dtype == torch.uint8 and c.h % (1 << c.depth) == 0
        t = F.targets(y, c.K)
        assert np.array_equal(t.numpy() != 0, unpack_class_bits(y.numpy(), c.K))
        assert all(0 < float(t[:, k].mean()) < 1 for k in range(c.K))


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.id)
def test_seeds_keep_clear_of_the_relu_threshold(case):
    margin = F.relu_margin(case)
    print(f"FAMILYCASE {case.id} seed={case.seed} margin={margin:.2e}")
    assert margin >= F.MARGIN


def test_loss_definition_is_the_reference():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 5, 6, 10, generator=g, dtype=torch.float64)
    y = torch.randint(0, 256, (2, 6, 10), generator=g).to(torch.uint8)
    want, _ = R.reference(("bce_class_dice",), x.permute(0, 2, 3, 1).reshape(-1, 5), y.numpy())
    assert abs(float(F.class_dice_loss(x, F.targets(y, 5).double())) - float(want)) <= 1e-13
