"""The kernel census of the forest's namespace (CPU): the smafa_sf:: kernels in the gfx950 code object of the built
libsmafa_amd.so must be exactly the four tabled here, each beside the GPU test that runs it.  The forest call launches no
smafa_cc::, smafa_lv:: or smafa_dn:: kernel (its union-find reuses smafa_cc::find_root / load_parent as device functions,
which are no kernels) and adds nothing to smafa::, smafa_join::, smafa_cc::, smafa_lv::, smafa_dn::, smafa_pk::, smafa_nb:: or
smafa_dl:: — pinned here at 199 / 3 / 3 / 3 / 4 / 6 / 4 / 3 as the other census files pin them — and none of the four names
carries a word those files forbid outside their namespaces."""
import os
import re

from test_join_kernel_census import ROOT, binary_kernels  # noqa: F401  (the fixture that lists the code object's kernels)
from test_delta_kernel_census import DL_KERNELS, NB_WORDS
from test_neighbours_kernel_census import FORBIDDEN, NB_KERNELS
from test_peaks_kernel_census import PK_KERNELS

# kernel -> the GPU test that runs it and asserts it by name (smafa_last_call_kernels)
SF_KERNELS = {
    "smafa_sf::init_forest_kernel": "tests/test_gpu_forest.py::test_dense_store",
    "smafa_sf::keep_pairs_kernel": "tests/test_gpu_forest.py::test_dense_store",
    "smafa_sf::span_edges_kernel": "tests/test_gpu_forest.py::test_dense_store",
    "smafa_sf::star_roots_kernel": "tests/test_gpu_forest.py::test_edges_and_errors",
}
DL_WORDS = ("gather_records", "delta_filter", "seed_parents")


def test_forest_kernels_are_the_tabled_ones(binary_kernels):  # noqa: F811
    found = {n for n in binary_kernels if n.startswith("smafa_sf::")}
    assert found == set(SF_KERNELS), (sorted(found - set(SF_KERNELS)), sorted(set(SF_KERNELS) - found))
    assert not [n for n in SF_KERNELS if any(w in n for w in FORBIDDEN + NB_WORDS + DL_WORDS)]


def test_other_namespaces_are_unchanged(binary_kernels):  # noqa: F811
    assert len({n for n in binary_kernels if n.startswith("smafa::")}) == 199
    assert {n for n in binary_kernels if n.startswith("smafa_join::")} == {
        "smafa_join::store_records_kernel", "smafa_join::inverse_order_kernel", "smafa_join::join_filter_kernel"}
    assert {n for n in binary_kernels if n.startswith("smafa_cc::")} == {
        "smafa_cc::init_labels_kernel", "smafa_cc::link_rows_kernel", "smafa_cc::flatten_labels_kernel"}
    assert {n for n in binary_kernels if n.startswith("smafa_lv::")} == {
        "smafa_lv::init_levels_kernel", "smafa_lv::hook_levels_kernel", "smafa_lv::flatten_levels_kernel"}
    assert {n for n in binary_kernels if n.startswith("smafa_dn::")} == {
        "smafa_dn::init_density_kernel", "smafa_dn::count_keep_kernel", "smafa_dn::link_cores_kernel",
        "smafa_dn::flatten_density_kernel"}
    assert {n for n in binary_kernels if n.startswith("smafa_pk::")} == set(PK_KERNELS) and len(PK_KERNELS) == 6
    assert {n for n in binary_kernels if n.startswith("smafa_nb::")} == set(NB_KERNELS) and len(NB_KERNELS) == 4
    assert {n for n in binary_kernels if n.startswith("smafa_dl::")} == set(DL_KERNELS) and len(DL_KERNELS) == 3
    others = {n for n in binary_kernels if not n.startswith(("smafa::", "smafa_join::", "smafa_cc::", "smafa_lv::", "smafa_dn::",
                                                              "smafa_pk::", "smafa_nb::", "smafa_dl::"))}
    assert not [n for n in others if any(w in n for w in FORBIDDEN + NB_WORDS + DL_WORDS)], others


def test_tabled_tests_exist_and_name_their_kernel():
    for name, test in SF_KERNELS.items():
        path, func = test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        assert re.search(r"^def %s\(" % re.escape(func), text, re.M), (name, test)
        assert name in text, name
