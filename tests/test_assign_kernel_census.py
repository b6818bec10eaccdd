"""The kernel census of the abundance table's namespace (CPU): the assign:: kernels in the gfx950 code object of the built
libsmafa_amd.so must be exactly the ones tabled here, each beside the GPU test that runs it and asserts it by name.  The call
adds no kernel to any other namespace and hands the radix sort and the exclusive sum plain integer types only: no kernel name in
the whole code object may carry a word the other census files forbid outside their namespaces."""
import os
import re

from test_join_kernel_census import JOIN_KERNELS, ROOT, binary_kernels  # noqa: F401  (the fixture that lists the code object's kernels)
from test_chimera_kernel_census import CHIMERA_KERNELS
from test_components_kernel_census import CC_KERNELS
from test_consensus_kernel_census import CONSENSUS_KERNELS, EVERY_WORD, OWNERS
from test_delta_kernel_census import DL_KERNELS
from test_density_kernel_census import DN_KERNELS
from test_forest_kernel_census import SF_KERNELS
from test_levels_kernel_census import LV_KERNELS
from test_neighbours_kernel_census import NB_KERNELS
from test_peaks_kernel_census import PK_KERNELS
from test_reach_kernel_census import MR_KERNELS
from test_stable_kernel_census import ST_KERNELS

SHAPES = "tests/test_gpu_assign.py::test_every_shape_equals_the_model"
# kernel -> the GPU test that runs it and asserts it by name (smafa_last_call_kernels)
ASSIGN_KERNELS = {
    "assign::init_kernel": SHAPES,
    "assign::best_kernel": SHAPES,
    "assign::bin_kernel": SHAPES,
    "assign::heads_kernel": SHAPES,
    "assign::fold_kernel": SHAPES,
}
PINNED = {"smafa_join::": JOIN_KERNELS, "smafa_cc::": CC_KERNELS, "smafa_lv::": LV_KERNELS, "smafa_dn::": DN_KERNELS, "smafa_pk::": PK_KERNELS,
          "smafa_nb::": NB_KERNELS, "smafa_dl::": DL_KERNELS, "smafa_sf::": SF_KERNELS, "smafa_mr::": MR_KERNELS, "smafa_st::": ST_KERNELS,
          "consensus::": CONSENSUS_KERNELS, "chimera::": CHIMERA_KERNELS}


def test_assign_kernels_are_the_tabled_ones(binary_kernels):  # noqa: F811
    found = {n for n in binary_kernels if n.startswith("assign::")}
    assert found == set(ASSIGN_KERNELS), (sorted(found - set(ASSIGN_KERNELS)), sorted(set(ASSIGN_KERNELS) - found))
    assert len({n for n in binary_kernels if n.startswith("smafa::")}) == 199  # nothing added to the scan's namespace


def test_every_other_namespace_is_unchanged(binary_kernels):  # noqa: F811
    for prefix, table in PINNED.items():
        found = {n for n in binary_kernels if n.startswith(prefix)}
        assert found == set(table), (prefix, sorted(found ^ set(table)))


def test_no_forbidden_word_in_any_name(binary_kernels):  # noqa: F811
    """rocprim's kernels included: a functor or a type handed to the sort or the sum would show in their names"""
    assert not sorted(n for n in binary_kernels if not n.startswith(OWNERS) and any(w in n for w in EVERY_WORD))
    assert not [n for n in ASSIGN_KERNELS if any(w in n for w in EVERY_WORD)]


def test_tabled_tests_exist_and_name_their_kernel():
    for name, test in ASSIGN_KERNELS.items():
        path, func = test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        assert re.search(r"^def %s\(" % re.escape(func), text, re.M), (name, test)
        assert name in text, name
