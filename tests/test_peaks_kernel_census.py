"""The kernel census of the peaks call's namespace (CPU): the smafa_pk:: kernels in the gfx950 code object of the built
libsmafa_amd.so must be exactly the six tabled here, each beside the GPU test that runs it.  The peaks call launches no
smafa_cc::, smafa_lv:: or smafa_dn:: kernel and adds none to smafa::, smafa_join::, smafa_cc::, smafa_lv:: or smafa_dn:: —
pinned here at 199 / 3 / 3 / 3 / 4 as the other census files pin them."""
import os
import re

from test_join_kernel_census import ROOT, binary_kernels  # noqa: F401  (the fixture that lists the code object's kernels)

# kernel -> the GPU test that runs it and asserts it by name (smafa_last_call_kernels)
PK_KERNELS = {
    "smafa_pk::init_peaks_kernel": "tests/test_gpu_peaks.py::test_dense_store",
    "smafa_pk::weigh_keep_kernel": "tests/test_gpu_peaks.py::test_dense_store",
    "smafa_pk::climb_kernel": "tests/test_gpu_peaks.py::test_one_join_against_two_joins",
    "smafa_pk::crown_kernel": "tests/test_gpu_peaks.py::test_edges_and_errors",
    "smafa_pk::settle_kernel": "tests/test_gpu_peaks.py::test_dense_store",
    "smafa_pk::jump_kernel": "tests/test_gpu_peaks.py::test_climb_chain",
}


def test_peaks_kernels_are_the_tabled_ones(binary_kernels):  # noqa: F811
    found = {n for n in binary_kernels if n.startswith("smafa_pk::")}
    assert found == set(PK_KERNELS), (sorted(found - set(PK_KERNELS)), sorted(set(PK_KERNELS) - found))


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
    others = {n for n in binary_kernels
              if not n.startswith(("smafa::", "smafa_join::", "smafa_cc::", "smafa_lv::", "smafa_dn::", "smafa_pk::"))}
    assert not [n for n in others if any(w in n for w in ("peaks", "weigh_keep", "climb", "crown", "settle", "jump"))], others


def test_tabled_tests_exist_and_name_their_kernel():
    for name, test in PK_KERNELS.items():
        path, func = test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        assert re.search(r"^def %s\(" % re.escape(func), text, re.M), (name, test)
        assert name in text, name
