"""The kernel census of the self-join's namespace (CPU), as it stood before tests/test_namespace_census.py: the smafa_join::
kernels in the gfx950 code object are exactly the tabled ones, and the join adds no kernel to smafa::.  The table is
tests/kernel_namespaces.py's and the reader tests/code_object.py's; nothing imports this module."""
import os
import re

import pytest

from code_object import ROOT, kernel_names
from kernel_namespaces import NAMESPACES

JOIN_KERNELS = NAMESPACES["smafa_join::"]


@pytest.fixture(scope="module")
def binary_kernels():
    return kernel_names()


def test_join_kernels_are_the_tabled_ones(binary_kernels):
    found = {n for n in binary_kernels if n.startswith("smafa_join::")}
    assert found == set(JOIN_KERNELS), (sorted(found - set(JOIN_KERNELS)), sorted(set(JOIN_KERNELS) - found))


def test_scan_namespace_is_unchanged(binary_kernels):
    assert len({n for n in binary_kernels if n.startswith("smafa::")}) == 199


def test_tabled_tests_exist():
    for name, test in JOIN_KERNELS.items():
        path, func = test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            assert re.search(r"^def %s\(" % re.escape(func), f.read(), re.M), (name, test)
