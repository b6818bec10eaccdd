"""The kernel census of the stable clusters' namespace (CPU): the smafa_st:: kernels in the gfx950 code object of the built
libsmafa_amd.so must be exactly the seven tabled here, each beside the GPU test that runs it and asserts it by name.  The call
reuses the reach forest's kernels and smafa_sf::init_forest_kernel as they are and adds no kernel to any other namespace —
tests/test_reach_kernel_census.py and tests/test_forest_kernel_census.py pin those — and none of the seven names carries a word
the other census files forbid outside their namespaces."""
import os
import re

from test_join_kernel_census import ROOT, binary_kernels  # noqa: F401  (the fixture that lists the code object's kernels)
from test_delta_kernel_census import NB_WORDS
from test_forest_kernel_census import DL_WORDS, SF_KERNELS
from test_neighbours_kernel_census import FORBIDDEN
from test_reach_kernel_census import MR_KERNELS, WORDS

# kernel -> the GPU test that runs it and asserts it by name (smafa_last_call_kernels)
ST_KERNELS = {
    "smafa_st::unite_class_kernel": "tests/test_gpu_stable.py::test_dense_store",
    "smafa_st::snapshot_kernel": "tests/test_gpu_stable.py::test_dense_store",
    "smafa_st::census_kernel": "tests/test_gpu_stable.py::test_dense_store",
    "smafa_st::adopt_kernel": "tests/test_gpu_stable.py::test_dense_store",
    "smafa_st::excess_kernel": "tests/test_gpu_stable.py::test_dense_store",
    "smafa_st::choose_kernel": "tests/test_gpu_stable.py::test_dense_store",
    "smafa_st::assign_kernel": "tests/test_gpu_stable.py::test_dense_store",
}
# every word the issue lists, whether or not another census file already forbids it
ISSUE_WORDS = ("label", "link_rows", "levels", "hook", "density", "count_keep", "link_cores", "peaks", "weigh_keep", "climb", "crown",
               "settle", "jump", "mirror_pack", "row_bounds", "cut_degrees", "emit_kernel", "gather_records", "delta_filter", "seed_parents")


def test_stable_kernels_are_the_tabled_ones(binary_kernels):  # noqa: F811
    found = {n for n in binary_kernels if n.startswith("smafa_st::")}
    assert found == set(ST_KERNELS), (sorted(found - set(ST_KERNELS)), sorted(set(ST_KERNELS) - found))
    assert {n for n in binary_kernels if n.startswith("smafa_mr::")} == set(MR_KERNELS)  # nothing added to the reach forest's
    assert {n for n in binary_kernels if n.startswith("smafa_sf::")} == set(SF_KERNELS)  # ... or to the forest's
    assert len({n for n in binary_kernels if n.startswith("smafa::")}) == 199


def test_no_other_namespace_appeared(binary_kernels):  # noqa: F811
    known = ("smafa::", "smafa_join::", "smafa_cc::", "smafa_lv::", "smafa_dn::", "smafa_pk::", "smafa_nb::", "smafa_dl::", "smafa_sf::",
             "smafa_mr::", "smafa_st::")
    assert not sorted(n for n in binary_kernels if n.startswith("smafa") and not n.startswith(known))


def test_no_forbidden_word_in_a_name():
    assert not [n for n in ST_KERNELS if any(w in n for w in ISSUE_WORDS + tuple(WORDS) + tuple(FORBIDDEN) + tuple(NB_WORDS) + tuple(DL_WORDS))]


def test_tabled_tests_exist_and_name_their_kernel():
    for name, test in ST_KERNELS.items():
        path, func = test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        assert re.search(r"^def %s\(" % re.escape(func), text, re.M), (name, test)
        assert name in text, name
