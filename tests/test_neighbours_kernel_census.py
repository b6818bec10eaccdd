"""The kernel census of the neighbours call's namespace (CPU): the smafa_nb:: kernels in the gfx950 code object of the built
libsmafa_amd.so must be exactly the four tabled here, each beside the GPU test that runs it.  The neighbours call launches no
smafa_cc::, smafa_lv::, smafa_dn:: or smafa_pk:: kernel and adds none to smafa::, smafa_join::, smafa_cc::, smafa_lv::,
smafa_dn:: or smafa_pk:: — pinned here at 199 / 3 / 3 / 3 / 4 / 6 as the other census files pin them.  The sorts and the sum
are the radix sort's and the scan's own kernels (rocprim::), which no census file counts; none of them carries a word the
other census files forbid outside their namespaces."""
import os
import re

from test_join_kernel_census import ROOT, binary_kernels  # noqa: F401  (the fixture that lists the code object's kernels)
from test_peaks_kernel_census import PK_KERNELS

# kernel -> the GPU test that runs it and asserts it by name (smafa_last_call_kernels)
NB_KERNELS = {
    "smafa_nb::mirror_pack_kernel": "tests/test_gpu_neighbours.py::test_neighbours_equal_brute_force",
    "smafa_nb::row_bounds_kernel": "tests/test_gpu_neighbours.py::test_neighbours_equal_brute_force",
    "smafa_nb::cut_degrees_kernel": "tests/test_gpu_neighbours.py::test_neighbours_equal_brute_force",
    "smafa_nb::emit_kernel": "tests/test_gpu_neighbours.py::test_neighbours_equal_brute_force",
}
FORBIDDEN = ("label", "link_rows", "levels", "hook", "density", "count_keep", "link_cores", "peaks", "weigh_keep", "climb", "crown",
             "settle", "jump")


def test_neighbours_kernels_are_the_tabled_ones(binary_kernels):  # noqa: F811
    found = {n for n in binary_kernels if n.startswith("smafa_nb::")}
    assert found == set(NB_KERNELS), (sorted(found - set(NB_KERNELS)), sorted(set(NB_KERNELS) - found))


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
    others = {n for n in binary_kernels
              if not n.startswith(("smafa::", "smafa_join::", "smafa_cc::", "smafa_lv::", "smafa_dn::", "smafa_pk::", "smafa_nb::"))}
    assert not [n for n in others if any(w in n for w in FORBIDDEN)], others
    assert not [n for n in others if any(w in n for w in ("mirror_pack", "row_bounds", "cut_degrees", "emit_kernel"))], others


def test_tabled_tests_exist_and_name_their_kernel():
    for name, test in NB_KERNELS.items():
        path, func = test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        assert re.search(r"^def %s\(" % re.escape(func), text, re.M), (name, test)
        assert name in text, name
