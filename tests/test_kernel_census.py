"""The kernel census (CPU): the smafa:: kernels in the gfx950 code object of the built libsmafa_amd.so must be exactly the
scan-family instantiations of tests/kernel_census_table.py's CENSUS (each with a GPU case in test_gpu_kernel_census.py) plus
the kernels of its EXEMPT map (each with the existing test that runs it).  A new instantiation without a case fails, and so
does a table entry the binary no longer has."""
import os
import re
import shutil
import subprocess

import pytest

from kernel_census_table import CENSUS, EXEMPT, SWITCHES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "smafa_amd", "lib", "libsmafa_amd.so")
LLVM = "/opt/rocm/llvm/bin"
TOOLS = {t: os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")}


def _tool(name):
    path = TOOLS.get(name) or shutil.which(name)
    return path if path and os.access(path, os.X_OK) else None


def _strip_signature(name):
    """'void smafa::k<1, 2>(args)' -> 'smafa::k<1, 2>'"""
    name = name.strip()
    if name.startswith("void "):
        name = name[5:]
    depth = 0
    for i, ch in enumerate(name):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return name[:i]
    return name


@pytest.fixture(scope="module")
def binary_kernels(tmp_path_factory):
    missing = [t for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "c++filt") if not _tool(t)]
    if missing:
        pytest.skip("kernel census needs the LLVM tools of ROCm and c++filt: missing %s" % ", ".join(missing))
    if not os.path.exists(LIB):
        import smafa_amd

        smafa_amd.build()
    tmp = tmp_path_factory.mktemp("census")
    fatbin, host, co = (str(tmp / n) for n in ("fatbin", "host.so", "gfx950.co"))
    subprocess.run([_tool("llvm-objcopy"), "--dump-section=.hip_fatbin=" + fatbin, LIB, host], check=True, capture_output=True)
    listed = subprocess.run([_tool("clang-offload-bundler"), "--list", "--type=o", "--input=" + fatbin], check=True,
                            capture_output=True, text=True).stdout.split()
    target = [t for t in listed if t.endswith("gfx950")]
    assert len(target) == 1, listed
    subprocess.run([_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fatbin, "--targets=" + target[0],
                    "--output=" + co], check=True, capture_output=True)
    syms = subprocess.run([_tool("llvm-readelf"), "-s", "--wide", co], check=True, capture_output=True, text=True).stdout
    mangled = sorted({f[-1][: -len(".kd")] for f in (ln.split() for ln in syms.splitlines()) if f and f[-1].endswith(".kd")})
    demangled = subprocess.run([_tool("c++filt")], input="\n".join(mangled), check=True, capture_output=True,
                               text=True).stdout.splitlines()
    assert len(demangled) == len(mangled)
    return {n for n in map(_strip_signature, demangled) if n.startswith("smafa::")}


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
