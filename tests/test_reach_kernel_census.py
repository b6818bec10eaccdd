"""The kernel census of the mutual-reachability forest's namespace (CPU): the smafa_mr:: kernels in the gfx950 code object of the
built libsmafa_amd.so must be exactly the three tabled here, each beside the GPU test that runs it and asserts it by name.  The
call reuses smafa_sf::init_forest_kernel and star_roots_kernel (and unite_won, a device function) and adds no kernel to any other
namespace — tests/test_forest_kernel_census.py pins those — and none of the three names carries a word the other census files
forbid outside their namespaces."""
import os
import re

from test_join_kernel_census import ROOT, binary_kernels  # noqa: F401  (the fixture that lists the code object's kernels)
from test_delta_kernel_census import NB_WORDS
from test_forest_kernel_census import DL_WORDS, SF_KERNELS
from test_neighbours_kernel_census import FORBIDDEN

# kernel -> the GPU test that runs it and asserts it by name (smafa_last_call_kernels)
MR_KERNELS = {
    "smafa_mr::tally_keep_kernel": "tests/test_gpu_reach_forest.py::test_dense_store",
    "smafa_mr::core_dist_kernel": "tests/test_gpu_reach_forest.py::test_dense_store",
    "smafa_mr::span_reach_kernel": "tests/test_gpu_reach_forest.py::test_dense_store",
}
WORDS = ("label", "levels", "hook", "density", "count_keep", "weigh_keep", "link_cores", "climb", "crown", "settle", "jump",
         "mirror_pack", "row_bounds", "cut_degrees", "emit_kernel", "gather_records", "delta_filter", "seed_parents")


def test_reach_kernels_are_the_tabled_ones(binary_kernels):  # noqa: F811
    found = {n for n in binary_kernels if n.startswith("smafa_mr::")}
    assert found == set(MR_KERNELS), (sorted(found - set(MR_KERNELS)), sorted(set(MR_KERNELS) - found))
    assert {n for n in binary_kernels if n.startswith("smafa_sf::")} == set(SF_KERNELS)  # nothing added to the forest's


def test_no_forbidden_word_in_a_name():
    assert not [n for n in MR_KERNELS if any(w in n for w in WORDS + FORBIDDEN + NB_WORDS + DL_WORDS)]


def test_tabled_tests_exist_and_name_their_kernel():
    for name, test in MR_KERNELS.items():
        path, func = test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        assert re.search(r"^def %s\(" % re.escape(func), text, re.M), (name, test)
        assert name in text, name
