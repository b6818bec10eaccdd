"""The kernel census of the consensus call's namespace (CPU): the consensus:: kernels in the gfx950 code object of the built
libsmafa_amd.so must be exactly the ones tabled here, each beside the GPU test that runs it and asserts it by name.  The
namespace does not begin with `smafa`: tests/test_stable_kernel_census.py::test_no_other_namespace_appeared holds every such
namespace to the eleven it knows, each pinned to its kernels.  The call also hands the radix sort and the exclusive sum
nothing of its own (no functor, no type): no kernel name in the whole code object may carry a word the other census files
forbid outside their namespaces."""
import os
import re

from test_join_kernel_census import ROOT, binary_kernels  # noqa: F401  (the fixture that lists the code object's kernels)
from test_delta_kernel_census import NB_WORDS
from test_forest_kernel_census import DL_WORDS
from test_neighbours_kernel_census import FORBIDDEN
from test_reach_kernel_census import WORDS
from test_stable_kernel_census import ISSUE_WORDS

DENSE = "tests/test_gpu_consensus.py::test_dense_store"
STATES = "tests/test_gpu_consensus.py::test_store_states"
SHAPES = "tests/test_gpu_consensus.py::test_every_shape_equals_the_model"
# kernel -> the GPU test that runs it and asserts it by name (smafa_last_call_kernels)
CONSENSUS_KERNELS = {
    "consensus::mark_groups_kernel": DENSE,
    "consensus::group_ids_kernel": DENSE,
    "consensus::group_keys_kernel": DENSE,
    "consensus::segment_bounds_kernel": DENSE,
    "consensus::tally_vote_kernel<2>": DENSE,
    "consensus::vote_tables_kernel<2>": STATES,
    "consensus::tally_vote_kernel<3>": STATES,
    "consensus::vote_tables_kernel<3>": STATES,
    "consensus::tally_vote_kernel<5>": SHAPES,
    "consensus::vote_tables_kernel<5>": "tests/test_gpu_consensus.py::test_chunks_of_64",
    "consensus::measure_kernel": DENSE,
    "consensus::finish_groups_kernel": DENSE,
}
EVERY_WORD = tuple(sorted(set(ISSUE_WORDS) | set(WORDS) | set(FORBIDDEN) | set(NB_WORDS) | set(DL_WORDS)))
# the namespaces that own those words (the census files of each pin their kernels)
OWNERS = ("smafa_cc::", "smafa_lv::", "smafa_dn::", "smafa_pk::", "smafa_nb::", "smafa_dl::", "smafa_sf::", "smafa_mr::", "smafa_st::")


def test_consensus_kernels_are_the_tabled_ones(binary_kernels):  # noqa: F811
    found = {n for n in binary_kernels if n.startswith("consensus::")}
    assert found == set(CONSENSUS_KERNELS), (sorted(found - set(CONSENSUS_KERNELS)), sorted(set(CONSENSUS_KERNELS) - found))
    assert len({n for n in binary_kernels if n.startswith("smafa::")}) == 199  # nothing added to the scan's namespace


def test_no_forbidden_word_in_any_name(binary_kernels):  # noqa: F811
    """rocprim's kernels included: a functor or a type handed to the sort or the scan would show in their names"""
    assert not sorted(n for n in binary_kernels if not n.startswith(OWNERS) and any(w in n for w in EVERY_WORD))
    assert not [n for n in CONSENSUS_KERNELS if any(w in n for w in EVERY_WORD)]


def test_tabled_tests_exist_and_name_their_kernel():
    for name, test in CONSENSUS_KERNELS.items():
        path, func = test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        assert re.search(r"^def %s\(" % re.escape(func), text, re.M), (name, test)
        assert name in text, name
