"""The kernel census of the levels' namespace (CPU): the smafa_lv:: kernels in the gfx950 code object of the built
libsmafa_amd.so must be exactly the ones tabled here, each beside the GPU test that runs it.  The levels call launches no
smafa_cc:: kernel (its union-find reuses smafa_cc::find_root / unite as device functions, which are no kernels) and adds
none to smafa::, smafa_join:: or smafa_cc:: — pinned here at 199 / 3 / 3 as the other census files pin them."""
import os
import re

from test_join_kernel_census import ROOT, binary_kernels  # noqa: F401  (the fixture that lists the code object's kernels)

# kernel -> the GPU test that runs it and asserts it by name (smafa_last_call_kernels)
LV_KERNELS = {
    "smafa_lv::init_levels_kernel": "tests/test_gpu_levels.py::test_dense_store",
    "smafa_lv::hook_levels_kernel": "tests/test_gpu_levels.py::test_dense_store",
    "smafa_lv::flatten_levels_kernel": "tests/test_gpu_levels.py::test_nesting_and_the_components_call_at_scale",
}


def test_levels_kernels_are_the_tabled_ones(binary_kernels):  # noqa: F811
    found = {n for n in binary_kernels if n.startswith("smafa_lv::")}
    assert found == set(LV_KERNELS), (sorted(found - set(LV_KERNELS)), sorted(set(LV_KERNELS) - found))


def test_other_namespaces_are_unchanged(binary_kernels):  # noqa: F811
    assert len({n for n in binary_kernels if n.startswith("smafa::")}) == 199
    assert {n for n in binary_kernels if n.startswith("smafa_join::")} == {
        "smafa_join::store_records_kernel", "smafa_join::inverse_order_kernel", "smafa_join::join_filter_kernel"}
    assert {n for n in binary_kernels if n.startswith("smafa_cc::")} == {
        "smafa_cc::init_labels_kernel", "smafa_cc::link_rows_kernel", "smafa_cc::flatten_labels_kernel"}
    others = {n for n in binary_kernels if not n.startswith(("smafa::", "smafa_join::", "smafa_cc::", "smafa_lv::"))}
    assert not [n for n in others if "label" in n or "link_rows" in n or "levels" in n or "hook" in n], others


def test_tabled_tests_exist_and_name_their_kernel():
    for name, test in LV_KERNELS.items():
        path, func = test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        assert re.search(r"^def %s\(" % re.escape(func), text, re.M), (name, test)
        assert name in text, name
