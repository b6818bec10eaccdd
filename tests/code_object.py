"""The reader of the built library's device code: kernel_names() lists the kernels in the gfx950 code object of
smafa_amd/lib/libsmafa_amd.so, demangled and without their signatures.  Every census reads it (tests/test_kernel_census.py,
tests/test_namespace_census.py); a pytest process unbundles the library once."""
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "smafa_amd", "lib", "libsmafa_amd.so")
LLVM = "/opt/rocm/llvm/bin"
TOOLS = {t: os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")}

runs = 0  # how often this process has unbundled the library to the end (tests/test_namespace_census.py holds it to one)


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


@functools.lru_cache(maxsize=None)
def kernel_names():
    """-> frozenset of names such as 'smafa::zone_kernel' or 'subset::unpack_rows_kernel<3>'; skips the calling test without
    the LLVM tools of ROCm and c++filt, builds the library where it is missing"""
    global runs
    missing = [t for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "c++filt") if not _tool(t)]
    if missing:
        pytest.skip("kernel census needs the LLVM tools of ROCm and c++filt: missing %s" % ", ".join(missing))
    if not os.path.exists(LIB):
        import smafa_amd

        smafa_amd.build()
    with tempfile.TemporaryDirectory(prefix="census") as tmp:
        fatbin, host, co = (os.path.join(tmp, n) for n in ("fatbin", "host.so", "gfx950.co"))
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
    runs += 1
    return frozenset(map(_strip_signature, demangled))
