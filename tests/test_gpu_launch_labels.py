"""The contraction kernels every network launches, pinned launch by launch.

One forward + backward pass of each case of tests/golden/make_launch_labels.py (Cnn3, the ResNet-encoder U-Net, the mask,
RPN and box heads, the ResNet-50-FPN backbone; several shapes; every compute mode) under the context profile: the ordered
(family, label) rows of the conv, weight-gradient and direct-kernel families must equal tests/golden/launch_labels.json,
which was recorded with the library as it was before kernel selection moved into csrc/dispatch.cpp.  The labels carry
kernel, shape, arithmetic and split count, so a changed choice, tile gate or slab plan shows as a changed row.  (The plain
U-Net's launches are pinned against the gates themselves by test_gpu_unet_configs.py::test_intended_kernels_ran.)"""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_launch_labels", os.path.join(GOLDEN, "make_launch_labels.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

with open(G.JSON_PATH) as _f:
    WANT = json.load(_f)


def test_fixture_covers_the_cases():
    assert sorted(WANT) == sorted(G.case_id(c, mode) for c, mode in G.CASES)
    assert all(len(rows) > 0 for rows in WANT.values())


@pytest.mark.gpu
@pytest.mark.parametrize("case,mode", G.CASES, ids=lambda v: v if isinstance(v, str) else f"{v.model}{'_'.join(map(str, v.args))}-{'x'.join(map(str, v.shape))}")
def test_launches_are_the_recorded_ones(case, mode):
    got = G.launch_labels(case, mode)
    want = WANT[G.case_id(case, mode)]
    diff = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert len(got) == len(want) and not diff, (len(got), len(want), diff[:5])
