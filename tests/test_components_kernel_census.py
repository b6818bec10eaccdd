"""The kernel census of the components' namespace (CPU): the smafa_cc:: kernels in the gfx950 code object of the built
libsmafa_amd.so must be exactly the ones tabled here, each beside the GPU test that runs it.  The components add no kernel
to smafa:: or smafa_join:: (tests/test_kernel_census.py and tests/test_join_kernel_census.py pin those at 199 and at three
names, and keep doing so)."""
import os
import re

import pytest

from test_join_kernel_census import ROOT, binary_kernels  # noqa: F401  (the fixture that lists the code object's kernels)

# kernel -> the GPU test that runs it and asserts it by name (smafa_last_call_kernels)
CC_KERNELS = {
    "smafa_cc::init_labels_kernel": "tests/test_gpu_components.py::test_dense_store",
    "smafa_cc::link_rows_kernel": "tests/test_gpu_components.py::test_dense_store",
    "smafa_cc::flatten_labels_kernel": "tests/test_gpu_components.py::test_against_the_join_and_the_query_path_at_scale",
}


def test_components_kernels_are_the_tabled_ones(binary_kernels):  # noqa: F811
    found = {n for n in binary_kernels if n.startswith("smafa_cc::")}
    assert found == set(CC_KERNELS), (sorted(found - set(CC_KERNELS)), sorted(set(CC_KERNELS) - found))


def test_other_namespaces_are_unchanged(binary_kernels):  # noqa: F811
    assert len({n for n in binary_kernels if n.startswith("smafa::")}) == 199
    assert {n for n in binary_kernels if n.startswith("smafa_join::")} == {
        "smafa_join::store_records_kernel", "smafa_join::inverse_order_kernel", "smafa_join::join_filter_kernel"}
    others = {n for n in binary_kernels if not n.startswith(("smafa::", "smafa_join::", "smafa_cc::"))}
    assert not [n for n in others if "label" in n or "link_rows" in n], others


def test_tabled_tests_exist_and_name_their_kernel():
    for name, test in CC_KERNELS.items():
        path, func = test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        assert re.search(r"^def %s\(" % re.escape(func), text, re.M), (name, test)
        assert name in text, name
