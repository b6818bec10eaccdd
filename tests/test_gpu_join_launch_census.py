"""The self-join's twelve calls launch what the parent commits launched (self_join.hip.h).

tests/join_launch_census.json holds, per call and case, `launches` and `scans` of smafa_last_call_stats and the whole list of
smafa_last_call_kernels, recorded by tools/join_census.py from a build of a parent commit (three repeats): pairs, components,
levels, density and peaks from the commit before the driver/consumer split ("build"), neighbours, forest, pairs_since and
components_update from the commit before join_span and the watching consumer, reach_forest, stable and chimeras from the commit
before the kernels' shared pieces (piece.hip.h) and the forests' shared span phase ("builds").  The cases are
the stores of the other GPU suites: the dense 4 000-row store at its bounds (the rescan at the default ceiling, the halving at
1 000 000 rows), nt60 x 3 020 rows with the kept list unset, 0 and half the pairs, aa60 x 20 020 rows in blocks of 128 at
stride 2 (many spans, a short last block), no row, one row, bounds at and above the sequence length, and a peaks radius
below the bound under and at a crowned bound.  Neighbours runs every case without a cut and at k = 3, and nt60 once more in two
sorts; pairs_since from row n // 2; components_update with the labels of the first n // 2 rows, the rest appended; reach_forest
at min_pts 3 with the cores, stable at min_pts 3 and min_cluster_size 2, chimeras at the peaks call's radius and fold 2.  Where the
parent's own repeats differed in `launches` — the jump rounds of a peaks call that climbed — the table holds null and only
scans and kernels are pinned."""
import json
import os
import sys

import pytest

from smafa_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import join_census  # noqa: E402

pytestmark = pytest.mark.gpu
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "join_launch_census.json")) as f:
    TABLE = json.load(f)


@pytest.mark.parametrize("call", join_census.EVERY_CALL)
def test_launches_scans_and_kernels_are_the_parents(call):
    want = TABLE["calls"][call]
    got = join_census.census(join_census.load(_lib.LIB_PATH), call)
    assert sorted(got) == sorted(want)
    for cid, rec in want.items():
        print(call, cid, got[cid]["launches"], got[cid]["scans"], got[cid]["kernels"])
        assert got[cid]["scans"] == rec["scans"], (call, cid)
        assert got[cid]["kernels"] == rec["kernels"], (call, cid)
        if rec["launches"] is not None:
            assert got[cid]["launches"] == rec["launches"], (call, cid)
