"""The kernel census of the components' namespace (CPU), as it stood before tests/test_namespace_census.py: the smafa_cc::
kernels in the gfx950 code object are exactly the tabled ones, each beside the GPU test that names it.  The table is tests/kernel_namespaces.py's and the reader tests/code_object.py's; nothing imports this module."""
import os
import re

import pytest

from code_object import ROOT, kernel_names
from kernel_namespaces import NAMESPACES

CC_KERNELS = NAMESPACES["smafa_cc::"]


@pytest.fixture(scope="module")
def binary_kernels():
    return kernel_names()


def test_components_kernels_are_the_tabled_ones(binary_kernels):
    found = {n for n in binary_kernels if n.startswith("smafa_cc::")}
    assert found == set(CC_KERNELS), (sorted(found - set(CC_KERNELS)), sorted(set(CC_KERNELS) - found))


def test_tabled_tests_exist_and_name_their_kernel():
    for name, test in CC_KERNELS.items():
        path, func = test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        assert re.search(r"^def %s\(" % re.escape(func), text, re.M), (name, test)
        assert name in text, name
