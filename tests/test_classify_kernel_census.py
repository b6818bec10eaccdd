"""The kernel census of the classification's namespace (CPU): the classify:: kernels in the gfx950 code object of the built
libsmafa_amd.so must be exactly the ones tabled here, each beside the GPU test that runs it and asserts it by name.  The call
adds no kernel to any other namespace — assign:: included, whose best, heads and fold kernels it launches as they are — and hands
the radix sort and the exclusive sum plain integer types only: no kernel name in the whole code object may carry a word the other
census files forbid outside their namespaces."""
import os
import re

from test_join_kernel_census import ROOT, binary_kernels  # noqa: F401  (the fixture that lists the code object's kernels)
from test_assign_kernel_census import ASSIGN_KERNELS, PINNED
from test_consensus_kernel_census import EVERY_WORD, OWNERS

SHAPES = "tests/test_gpu_classify.py::test_every_shape_equals_the_model"
# kernel -> the GPU test that runs it and asserts it by name (smafa_last_call_kernels)
CLASSIFY_KERNELS = {
    "classify::start_kernel": SHAPES,
    "classify::agree_kernel": SHAPES,
    "classify::key_kernel": SHAPES,
}


def test_classify_kernels_are_the_tabled_ones(binary_kernels):  # noqa: F811
    found = {n for n in binary_kernels if n.startswith("classify::")}
    assert found == set(CLASSIFY_KERNELS), (sorted(found - set(CLASSIFY_KERNELS)), sorted(set(CLASSIFY_KERNELS) - found))
    assert len({n for n in binary_kernels if n.startswith("smafa::")}) == 199  # nothing added to the scan's namespace


def test_every_other_namespace_is_unchanged(binary_kernels):  # noqa: F811
    for prefix, table in {**PINNED, "assign::": ASSIGN_KERNELS}.items():
        found = {n for n in binary_kernels if n.startswith(prefix)}
        assert found == set(table), (prefix, sorted(found ^ set(table)))


def test_no_forbidden_word_in_any_name(binary_kernels):  # noqa: F811
    """rocprim's kernels included: a functor or a type handed to the sort or the sum would show in their names"""
    assert not sorted(n for n in binary_kernels if not n.startswith(OWNERS) and any(w in n for w in EVERY_WORD))
    assert not [n for n in CLASSIFY_KERNELS if any(w in n for w in EVERY_WORD)]


def test_tabled_tests_exist_and_name_their_kernel():
    for name, test in CLASSIFY_KERNELS.items():
        path, func = test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        assert re.search(r"^def %s\(" % re.escape(func), text, re.M), (name, test)
        assert name in text, name
