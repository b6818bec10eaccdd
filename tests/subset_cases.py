"""Stores, keep masks and the numpy model of the subset and rows calls (tests/test_gpu_subset.py).

The model is two lines: the subset of a store whose rows are `codes` under a boolean mask `keep` is a store whose rows are
codes[keep], and old_of_new = flatnonzero(keep); the rows of a store are the code bytes it was given.  Nothing here comes from the
code under test."""
import ctypes as C
import functools

import numpy as np

import smafa_amd

KINDS = ("nt2", "nt3", "aa")                       # 2-plane nt, 3-plane nt (code 4 present), aa with all 28 codes
LENGTHS = (1, 31, 32, 33, 60, 64, 65, 130)         # around the 32-column word and the 64-column slice; 130: five words, wide kernel
SIZES = (1, 255, 256, 257, 4095, 4096, 5000)       # around the 256-row tile; 4096 is the first sorted append
PLANES = {"nt2": 2, "nt3": 3, "aa": 5}
MASKS = ("all", "none", "first", "last", "last_tile", "every_second", "random10", "random90")
SUBSET_CALL = ["subset::keep_flags_kernel", "subset::run_ends_kernel", "subset::move_rows_kernel", "smafa::zone_kernel"]  # one subset call's launches


def alphabet_of(kind):
    return smafa_amd.ALPHABET_AA if kind == "aa" else smafa_amd.ALPHABET_NT


@functools.lru_cache(maxsize=None)
def random_codes(kind, L, n, seed=0):
    """n x L code bytes: nt2 0..3, nt3 0..4 with a 4 in row 0, aa 0..27 (every code where the store has room for them)"""
    rng = np.random.default_rng(1000 * L + n + 7 * KINDS.index(kind) + seed)
    top = {"nt2": 4, "nt3": 5, "aa": 28}[kind]
    codes = rng.integers(0, top, size=(n, L), dtype=np.uint8)
    if kind == "nt3":
        codes[0, 0] = 4
    if kind == "aa" and n * L >= 28:
        codes.reshape(-1)[rng.choice(n * L, size=28, replace=False)] = np.arange(28, dtype=np.uint8)
        assert len(np.unique(codes)) == 28
    codes.setflags(write=False)
    return codes


def keep_mask(name, n, seed=0):
    """the issue's masks over n rows, as booleans"""
    rng = np.random.default_rng(n + seed)
    keep = np.zeros(n, dtype=bool)
    if name == "all":
        keep[:] = True
    elif name == "first":
        keep[0] = True
    elif name == "last":
        keep[n - 1] = True
    elif name == "last_tile":
        keep[(n - 1) // 256 * 256:] = True
    elif name == "every_second":
        keep[::2] = True
    elif name == "random10":
        keep = rng.random(n) < 0.1
    elif name == "random90":
        keep = rng.random(n) < 0.9
    else:
        assert name == "none", name
    return keep


def expected_subset(codes, keep):
    """-> (rows of the subset, old_of_new)"""
    keep = np.asarray(keep) != 0
    return codes[keep], np.flatnonzero(keep).astype(np.uint32)


def make_store(kind, L, codes=None, pieces=None):
    store = smafa_amd.SubjectStore(L, alphabet_of(kind))
    for piece in (pieces if pieces is not None else [codes]):
        if len(piece):
            store.push(piece)
    return store


@functools.lru_cache(maxsize=None)
def two_family_case(n=8192, L=60, seed=3):
    """-> (codes, family, queries): n amino-acid rows of two families, A and B, whose members differ from their family's seed in
    up to 4 of the LAST 28 columns and whose seeds differ in every column — so the two families' filter prefixes differ whatever
    columns the layout puts first; 200 queries planted within 3 columns of a row, half of them from each family"""
    rng = np.random.default_rng(seed)
    seeds = np.stack([rng.integers(0, 14, size=L), 14 + rng.integers(0, 14, size=L)]).astype(np.uint8)
    family = rng.integers(0, 2, size=n)
    codes = seeds[family].copy()
    for r in range(4):
        who = np.flatnonzero(rng.random(n) < 0.7)
        col = rng.integers(L - 28, L, size=len(who))
        codes[who, col] = rng.integers(0, 28, size=len(who))
    pick = np.concatenate([rng.choice(np.flatnonzero(family == f), size=100, replace=False) for f in (0, 1)])
    queries = codes[pick].copy()
    for q in queries:
        q[rng.integers(0, L, size=rng.integers(0, 4))] = rng.integers(0, 28)
    for a in (codes, family, queries):
        a.setflags(write=False)
    return codes, family, queries


# ---- device memory for the launch forms, from the HIP runtime the library itself is linked to
@functools.lru_cache(maxsize=None)
def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


class DeviceArray:
    """a host array's bytes in device memory: .ptr for a launch form, .get() to read them back"""

    def __init__(self, host):
        self.host = np.ascontiguousarray(host)
        self.ptr = C.c_void_p()
        assert _hip().hipMalloc(C.byref(self.ptr), max(self.host.nbytes, 16)) == 0
        assert _hip().hipMemcpy(self.ptr, self.host.ctypes.data, self.host.nbytes, 1) == 0  # hipMemcpyHostToDevice
        self.ptr = self.ptr.value

    def get(self):
        out = np.empty_like(self.host)
        assert _hip().hipMemcpy(out.ctypes.data, self.ptr, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return out

    def free(self):
        if self.ptr:
            _hip().hipFree(self.ptr)
            self.ptr = 0
