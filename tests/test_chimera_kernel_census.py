"""The kernel census of the chimera check's namespace (CPU): the chimera:: kernels in the gfx950 code object of the built
libsmafa_amd.so must be exactly the three tabled here, each beside the GPU test that runs it and asserts it by name.  The
namespace does not begin with `smafa` (tests/test_stable_kernel_census.py::test_no_other_namespace_appeared pins those), the call
launches smafa_pk::init_peaks_kernel and smafa_pk::weigh_keep_kernel as they are and adds nothing to smafa_pk:: or smafa::, and
none of the three names carries a word the other census files forbid outside their namespaces."""
import os
import re

from test_join_kernel_census import ROOT, binary_kernels  # noqa: F401  (the fixture that lists the code object's kernels)
from test_consensus_kernel_census import CONSENSUS_KERNELS, EVERY_WORD, OWNERS
from test_peaks_kernel_census import PK_KERNELS

KERNELS = "tests/test_gpu_chimeras.py::test_kernels_by_name_and_statistics"
# kernel -> the GPU test that runs it and asserts it by name (smafa_last_call_kernels)
CHIMERA_KERNELS = {
    "chimera::init_sides_kernel": KERNELS,
    "chimera::offer_sides_kernel": KERNELS,
    "chimera::verdict_kernel": KERNELS,
}


def test_chimera_kernels_are_the_tabled_ones(binary_kernels):  # noqa: F811
    found = {n for n in binary_kernels if n.startswith("chimera::")}
    assert found == set(CHIMERA_KERNELS), (sorted(found - set(CHIMERA_KERNELS)), sorted(set(CHIMERA_KERNELS) - found))
    assert len({n for n in binary_kernels if n.startswith("smafa::")}) == 199  # nothing added to the scan's namespace
    assert {n for n in binary_kernels if n.startswith("smafa_pk::")} == set(PK_KERNELS)  # ... or to the peaks call's
    assert {n for n in binary_kernels if n.startswith("consensus::")} == set(CONSENSUS_KERNELS)


def test_no_forbidden_word_in_a_name(binary_kernels):  # noqa: F811
    assert not [n for n in CHIMERA_KERNELS if any(w in n for w in EVERY_WORD)]
    assert not sorted(n for n in binary_kernels if not n.startswith(OWNERS) and any(w in n for w in EVERY_WORD))


def test_tabled_tests_exist_and_name_their_kernel():
    for name, test in CHIMERA_KERNELS.items():
        path, func = test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        assert re.search(r"^def %s\(" % re.escape(func), text, re.M), (name, test)
        assert name in text, name
