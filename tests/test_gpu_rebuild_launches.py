"""The launches of a pass that rebuilds derived filter copies, pinned launch by launch.

Each case of tests/golden/make_rebuild_launches.py (the U-Net, the ResNet-encoder U-Net, the mask head and the
ResNet-50-FPN backbone; every compute mode; a second step, a pass after a partial load_state_dict, a pass after a round
trip through another mode) runs its last pass under the context profile.  The number of launches, the SHA-256 of their
ordered family,label,mbytes lines and the ordered rows of the elementwise family -- where every rebuild launch records
itself -- must equal tests/golden/rebuild_launches.json, which was recorded with the library as it was before the
staleness of the copies moved into rfi_model::stale and sync_filters.  So a rebuild that runs twice, not at all, in
another order or over another table shows as a changed row.

The profile turns the split rebuild off (sync_filters splits only while ctx->profiling is off), so every launch here
is on the main stream: the side-stream half of a split rebuild is checked by the byte comparisons of
test_gpu_derived_copies.py (overlap on and off, profile on and off), not by this fixture."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_rebuild_launches", os.path.join(GOLDEN, "make_rebuild_launches.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

with open(G.JSON_PATH) as _f:
    WANT = json.load(_f)


def test_fixture_covers_the_cases():
    assert sorted(WANT) == sorted(G.case_id(*c) for c in G.CASES)
    assert all(v["rows"] > 0 and v["elementwise"] for v in WANT.values())


@pytest.mark.gpu
@pytest.mark.parametrize("row,mode,script", G.CASES)
def test_rebuild_launches_are_the_recorded_ones(row, mode, script):
    got = G.rebuild_launches(row, mode, script)
    want = WANT[G.case_id(row, mode, script)]
    ge, we = got["elementwise"], want["elementwise"]
    diff = [(i, g, w) for i, (g, w) in enumerate(zip(ge, we)) if g != w]
    assert len(ge) == len(we) and not diff, (len(ge), len(we), diff[:5])
    assert (got["rows"], got["sha256"]) == (want["rows"], want["sha256"])
