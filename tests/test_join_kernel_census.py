"""The kernel census of the self-join's namespace (CPU): the smafa_join:: kernels in the gfx950 code object of the built
libsmafa_amd.so must be exactly the ones tabled here, each beside the GPU test that runs it — and the join adds no kernel to
smafa:: (tests/test_kernel_census.py pins that namespace at 199: the join launches scan instantiations that exist)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "smafa_amd", "lib", "libsmafa_amd.so")
LLVM = "/opt/rocm/llvm/bin"

# kernel -> the GPU test that runs it (every self-join builds records and filters; the inverse order map is asserted by name)
JOIN_KERNELS = {
    "smafa_join::store_records_kernel": "tests/test_gpu_self_join.py::test_self_pairs_equal_brute_force",
    "smafa_join::inverse_order_kernel": "tests/test_gpu_self_join.py::test_stale_state_after_push",
    "smafa_join::join_filter_kernel": "tests/test_gpu_self_join.py::test_every_engine_one_answer",
}


def _tool(name):
    path = os.path.join(LLVM, name)
    path = path if os.access(path, os.X_OK) else shutil.which(name)
    return path if path and os.access(path, os.X_OK) else None


def _strip_signature(name):
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
    tmp = tmp_path_factory.mktemp("join_census")
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
    return {_strip_signature(n) for n in demangled}


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
