"""The kernel census of every namespace (CPU): the gfx950 code object of the built libsmafa_amd.so holds exactly the kernels
tabled in tests/kernel_namespaces.py and tests/kernel_census_table.py, nothing outside those namespaces but the library's own
kernels, and each reserved word in its owner's names only; every tabled GPU test exists and names its kernel.  Each rule is a
function (names, table) -> offenders, so the last test can show that a doctored set of names trips it."""
import os
import re

import pytest

import code_object
from kernel_census_table import CENSUS, EXEMPT
from kernel_namespaces import LIBRARY_NAMESPACES, NAMESPACES, RESERVED, STEM_ONLY

TABLES = {"smafa::": set(CENSUS) | set(EXEMPT), **{ns: set(table) for ns, table in NAMESPACES.items()}}


def exact_set(names, ns, tabled):
    found = {n for n in names if n.startswith(ns)}
    return ["unmapped: " + n for n in sorted(found - tabled)] + ["stale: " + n for n in sorted(tabled - found)]


def closed_set(names, known):
    return sorted(n for n in names if not n.startswith(known))


def strayed_words(names, reserved):
    return sorted((w, n) for w, owner in reserved.items() for n in names if w in n and not n.startswith(owner))


def unused_words(names, reserved):
    return sorted(w for w, owner in reserved.items() if not any(w in n for n in names if n.startswith(owner)))


def offenders(names):
    """rule -> its offenders, for the rules that have any"""
    found = {"exact set " + ns: exact_set(names, ns, tabled) for ns, tabled in TABLES.items()}
    found["closed set"] = closed_set(names, tuple(TABLES) + LIBRARY_NAMESPACES)
    found["strayed words"] = strayed_words(names, RESERVED)
    found["unused words"] = unused_words(names, RESERVED)
    return {rule: bad for rule, bad in found.items() if bad}


@pytest.fixture(scope="module")
def names():
    return code_object.kernel_names()


@pytest.mark.parametrize("ns", TABLES)
def test_namespace_holds_exactly_its_tabled_kernels(names, ns):
    assert not exact_set(names, ns, TABLES[ns])


def test_no_kernel_outside_the_known_namespaces(names):
    assert not closed_set(names, tuple(TABLES) + LIBRARY_NAMESPACES)


def test_reserved_words_stay_with_their_owner(names):
    """rocprim's kernels included: a functor or a type handed to a sort, a scan or a sum would show in their names"""
    assert not strayed_words(names, RESERVED)


def test_every_reserved_word_is_carried_by_its_owner(names):
    assert not unused_words(names, RESERVED)


@pytest.mark.parametrize("ns", NAMESPACES)
def test_tabled_tests_exist_and_name_their_kernel(ns):
    for name, test in NAMESPACES[ns].items():
        path, func = test.split("::")
        with open(os.path.join(code_object.ROOT, path)) as f:
            text = f.read()
        assert re.search(r"^def %s\(" % re.escape(func), text, re.M), (name, test)
        assert (name.split("<")[0] if name in STEM_ONLY else name) in text, name


DOCTORED = {
    "unchanged": (lambda names: names, None),
    "a kernel added": (lambda names: names | {"classify::vote_kernel"}, "exact set classify::"),
    "a kernel removed": (lambda names: names - {"smafa_mr::core_dist_kernel"}, "exact set smafa_mr::"),
    "an unknown namespace": (lambda names: names | {"foo::bar_kernel"}, "closed set"),
    "label in rocprim::": (lambda names: names | {"rocprim::detail::sort_kernel<label_less>"}, "strayed words"),
    "peaks in smafa_st::": (lambda names: names | {"smafa_st::peaks_kernel"}, "strayed words"),
    "hook in smafa::": (lambda names: names | {"smafa::hook_kernel"}, "strayed words"),
}


@pytest.mark.parametrize("case", DOCTORED)
def test_doctored_names_trip_their_rule(names, case):
    doctor, rule = DOCTORED[case]
    found = offenders(doctor(names))
    assert (rule in found) if rule else not found, found
    assert code_object.runs == 1  # every census of this process read one unbundling of the library
