"""The kernel census (CPU): the smafa:: kernels in the gfx950 code object of the built libsmafa_amd.so must be exactly the
scan-family instantiations of tests/kernel_census_table.py's CENSUS (each with a GPU case in test_gpu_kernel_census.py) plus
the kernels of its EXEMPT map (each with the existing test that runs it).  A new instantiation without a case fails, and so
does a table entry the binary no longer has."""
import os
import re

import pytest

from code_object import ROOT, kernel_names
from kernel_census_table import CENSUS, EXEMPT, SWITCHES


@pytest.fixture(scope="module")
def binary_kernels():
    return {n for n in kernel_names() if n.startswith("smafa::")}


def test_every_kernel_in_the_binary_is_mapped(binary_kernels):
    tabled = set(CENSUS) | set(EXEMPT)
    assert not set(CENSUS) & set(EXEMPT)
    assert len(binary_kernels) == 199, len(binary_kernels)
    unmapped = sorted(binary_kernels - tabled)
    stale = sorted(tabled - binary_kernels)
    assert not unmapped, "instantiations without a census case or an exempting test: %s" % unmapped
    assert not stale, "table entries the binary no longer has: %s" % stale
    assert len(CENSUS) == 178


def test_census_cases_are_well_formed():
    for name, cases in CENSUS.items():
        assert cases, name
        for c in cases:
            assert c["switches"] in SWITCHES, (name, c)
            assert c["kind"] in ("nt2", "nt3", "aa") and 1 <= c["L"] <= 255, (name, c)
            assert c["nq"] in (1, 64, 65, 129), (name, c)
            assert c["D"] is not None or c["k"] >= 1, (name, c)
            assert c["E"] is not None and c["E"] <= c["L"], (name, c)
            if "scan_zone_few" in name:
                assert c["nq"] <= 64 and c["zone"] == 2, name
            if "scan_zone_kernel" in name:
                assert c["nq"] > 64 and c["zone"] == 2, name
    # wide kernels: every non-seed instantiation with a zone level of its own has a case for both forms
    for name, cases in CENSUS.items():
        m = re.match(r"smafa::scan_wide_kernel<\d, \d, false, 3, 0>", name)
        if m:
            assert sorted(c["marker"] or "" for c in cases) == ["", "zone level on"], name
    # the k-th seed kernel: every instantiation has its seed form (no marker) and its counting form over a sample, once each
    seeds = [name for name in CENSUS if name.startswith("smafa::kth_seed_kernel<")]
    assert len(seeds) == 13, seeds
    for name in seeds:
        cases = CENSUS[name]
        assert sorted(c["marker"] or "" for c in cases) == ["", "sample counts"], name
        plain, counts = sorted(cases, key=lambda c: c["marker"] or "")
        assert counts["switches"] == "kth_sample" and plain["switches"] == "default", name
        assert all(plain[f] == counts[f] for f in ("kind", "L", "D", "k", "nq", "E")) and plain["k"] == 3 and plain["nq"] == 65, name
    # no other marker, and none anywhere else
    for name, cases in CENSUS.items():
        for c in cases:
            assert c["marker"] in (None, "zone level on", "sample counts"), (name, c)
            assert c["marker"] != "zone level on" or name.startswith("smafa::scan_wide_kernel<"), name
            assert c["marker"] != "sample counts" or name.startswith("smafa::kth_seed_kernel<"), name


def test_exempt_tests_exist():
    for name, test in EXEMPT.items():
        path, func = test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            assert re.search(r"^def %s\(" % re.escape(func), f.read(), re.M), (name, test)
