"""The kernel census of the subset's namespace (CPU): the subset:: kernels in the gfx950 code object of the built libsmafa_amd.so
must be exactly the ones tabled here, each beside the GPU test that runs it and asserts it by name.  The two calls add no kernel to
any other namespace — smafa::zone_kernel and smafa_join::inverse_order_kernel are launched as they are — and hand the exclusive
sums plain integer types only: no kernel name in the whole code object may carry a word the other census files forbid outside
their namespaces."""
import os
import re

from test_join_kernel_census import ROOT, binary_kernels  # noqa: F401  (the fixture that lists the code object's kernels)
from test_assign_kernel_census import ASSIGN_KERNELS, PINNED
from test_classify_kernel_census import CLASSIFY_KERNELS
from test_consensus_kernel_census import EVERY_WORD, OWNERS

NAMES = "tests/test_gpu_subset.py::test_kernels_by_name"
# kernel -> the GPU test that runs it and asserts it by name (smafa_last_call_kernels)
SUBSET_KERNELS = {
    "subset::keep_flags_kernel": NAMES,
    "subset::run_ends_kernel": NAMES,
    "subset::move_rows_kernel": NAMES,
    "subset::unpack_rows_kernel<2>": NAMES,
    "subset::unpack_rows_kernel<3>": NAMES,
    "subset::unpack_rows_kernel<5>": NAMES,
}
SUBSET_CALL = ["subset::keep_flags_kernel", "subset::run_ends_kernel", "subset::move_rows_kernel", "smafa::zone_kernel"]


def test_subset_kernels_are_the_tabled_ones(binary_kernels):  # noqa: F811
    found = {n for n in binary_kernels if n.startswith("subset::")}
    assert found == set(SUBSET_KERNELS), (sorted(found - set(SUBSET_KERNELS)), sorted(set(SUBSET_KERNELS) - found))
    assert len({n for n in binary_kernels if n.startswith("smafa::")}) == 199  # nothing added to the scan's namespace


def test_every_other_namespace_is_unchanged(binary_kernels):  # noqa: F811
    for prefix, table in {**PINNED, "assign::": ASSIGN_KERNELS, "classify::": CLASSIFY_KERNELS}.items():
        found = {n for n in binary_kernels if n.startswith(prefix)}
        assert found == set(table), (prefix, sorted(found ^ set(table)))


def test_no_forbidden_word_in_any_name(binary_kernels):  # noqa: F811
    """rocprim's kernels included: a functor or a type handed to the sum would show in their names"""
    assert not sorted(n for n in binary_kernels if not n.startswith(OWNERS) and any(w in n for w in EVERY_WORD))
    assert not [n for n in SUBSET_KERNELS if any(w in n for w in EVERY_WORD)]


def test_tabled_tests_exist_and_name_their_kernel():
    for name, test in SUBSET_KERNELS.items():
        path, func = test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        assert re.search(r"^def %s\(" % re.escape(func), text, re.M), (name, test)
        assert name.split("<")[0] in text, name
