"""Launch census of the twelve self-join calls: launches, scans and the kernel list of smafa_last_call_stats /
smafa_last_call_kernels, per call and case — tests/join_launch_census.json, which tests/test_gpu_join_launch_census.py holds
this tree against.

The table is recorded from a build of the PARENT commit: one library (SMAFA_AMD_LIB, or this tree's) is loaded through ctypes
alone, so that the parent's build runs the very same cases:

    SMAFA_AMD_LIB=$PARENT python tools/join_census.py --repeat 3 --out tests/join_launch_census.json

With --calls only the named calls are recorded and merged into the file that is there: the other calls' entries stay as they
are, from the parent they were recorded from, and "builds" names the build of every call recorded this way:

    SMAFA_AMD_LIB=$PARENT python tools/join_census.py --repeat 3 --calls neighbours,forest --out tests/join_launch_census.json

A peaks call that climbed ends in jump rounds, whose number may differ from run to run (pointer doubling in place): where
`launches` differed between the repeats it is recorded as null and only scans and kernels are pinned."""
import argparse
import ctypes as C
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CALLS = ["pairs", "components", "levels", "density", "peaks"]  # recorded from the commit before the driver/consumer split
NEWER_CALLS = ["neighbours", "forest", "pairs_since", "components_update"]  # recorded later (--calls), each from its own parent
ALL_CALLS = CALLS + NEWER_CALLS  # (the nine of the tables recorded before piece.hip.h: a test of those commits runs these)
NEWEST_CALLS = ["reach_forest", "stable", "chimeras"]  # recorded from the commit before the kernels' shared pieces (piece.hip.h)
EVERY_CALL = ALL_CALLS + NEWEST_CALLS
KNOBS = ["SMAFA_JOIN_BLOCK", "SMAFA_JOIN_STRIDE", "SMAFA_JOIN_SCRATCH_MAX", "SMAFA_DENSITY_KEEP_MAX", "SMAFA_NEIGHBOUR_SORT"]
NONE = 0xFFFFFFFF  # SMAFA_NONE


@functools.lru_cache(maxsize=None)
def stores():
    """the existing stores of the GPU suites -> {name: (codes, alphabet)}, and the pair count of nt60 at its bound"""
    from components_cases import dense_store
    from self_join_cases import brute_pairs, planted_store

    nt60 = planted_store(11 + 300 + 4, "nt", 60, 300)
    aa60 = planted_store(11 + 2000 + 4, "aa", 60, 2000)
    one = nt60[:1].copy()
    return ({"dense": (dense_store()[0], 0), "nt60": (nt60, 0), "aa60": (aa60, 1), "n0": (nt60[:0].copy(), 0), "n1": (one, 0)},
            len(brute_pairs(nt60, 5)))


def cases(call=None):
    """-> [(id, store, max_div, radius of the peaks call, knobs)]; neighbours: every case at both cuts, and one in two sorts"""
    if call == "neighbours":
        both = cases() + [("nt60 two sorts", "nt60", 5, NONE, {"SMAFA_NEIGHBOUR_SORT": "2"})]
        return [(cid + ", k %s" % ("none" if k == NONE else k), name, D, k, knobs) for cid, name, D, _, knobs in both for k in (NONE, 3)]
    pairs = stores()[1]
    out = []
    for D in (0, 3):  # the dense store at its bounds: the rescan at the default ceiling, the halving at 1 000 000 rows
        out.append(("dense D=%d" % D, "dense", D, NONE, {}))
        out.append(("dense D=%d ceiling 1000000" % D, "dense", D, NONE, {"SMAFA_JOIN_SCRATCH_MAX": "1000000"}))
    for keep in (None, 0, pairs // 2):  # the kept list: every pair, none, half of them
        out.append(("nt60 keep %s" % ("unset" if keep is None else keep), "nt60", 5, NONE,
                    {} if keep is None else {"SMAFA_DENSITY_KEEP_MAX": str(keep)}))
    out.append(("aa60 block 128 stride 2", "aa60", 5, NONE, {"SMAFA_JOIN_BLOCK": "128", "SMAFA_JOIN_STRIDE": "2"}))
    out.append(("n = 0", "n0", 5, NONE, {}))
    out.append(("n = 1", "n1", 5, NONE, {}))
    out.append(("nt60 max_div = L", "nt60", 60, NONE, {}))
    out.append(("nt60 max_div = L + 10", "nt60", 70, NONE, {}))
    out.append(("nt60 radius 2 below a crowned bound", "nt60", 5, 2, {}))
    out.append(("nt60 radius 2 at a crowned bound", "nt60", 60, 2, {}))
    return out


def load(path):
    lib = C.CDLL(path)
    vp, u64p, u32p = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    lib.smafa_last_error.restype = C.c_char_p
    lib.smafa_build_id.restype = C.c_char_p
    lib.smafa_db_destroy.restype = None
    lib.smafa_db_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_uint32]
    lib.smafa_db_append.argtypes = [vp, vp, C.c_uint64]
    lib.smafa_db_destroy.argtypes = [vp]
    lib.smafa_db_self_hits.argtypes = [vp, C.c_uint32, vp, C.c_uint64, u64p]
    lib.smafa_db_self_components.argtypes = [vp, C.c_uint32, vp, C.c_uint64, u64p]
    lib.smafa_db_self_levels.argtypes = [vp, C.c_uint32, vp, C.c_uint64, u64p]
    lib.smafa_db_self_density.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64, u64p]
    lib.smafa_db_self_peaks.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint64, u64p]
    lib.smafa_db_self_neighbours.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint64, u64p]
    lib.smafa_db_self_forest.argtypes = [vp, C.c_uint32, vp, C.c_uint64, u64p]
    lib.smafa_db_self_reach_forest.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_uint64, u64p, vp]
    lib.smafa_db_self_stable.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint64, u64p]
    lib.smafa_db_self_chimeras.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, u64p]
    lib.smafa_db_self_hits_since.argtypes = [vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, u64p]
    lib.smafa_db_self_components_update.argtypes = [vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, u64p]
    lib.smafa_last_call_stats.argtypes = [vp, C.POINTER(C.c_float), u32p, u32p]
    lib.smafa_last_call_kernels.argtypes = [vp, C.c_char_p, C.c_uint64]
    return lib


def census(lib, call):
    """every case of `call` on a fresh handle -> {case id: {"launches", "scans", "kernels"}}"""
    vp = C.c_void_p
    out = {}

    def ok(rc, allowed=()):
        if rc and rc not in allowed:
            raise RuntimeError("join_census: %s" % lib.smafa_last_error().decode())

    for cid, name, D, radius, knobs in cases(call):  # (neighbours: the cut in the radius' place)
        codes, alphabet = stores()[0][name]
        n = len(codes)
        saved = {k: os.environ.pop(k, None) for k in KNOBS}
        os.environ.update(knobs)  # (the knobs are read when the handle is created)
        h = vp()
        try:
            ok(lib.smafa_db_create(C.byref(h), 0, alphabet, codes.shape[1]))
        finally:
            for k in KNOBS:
                os.environ.pop(k, None)
                if saved[k] is not None:
                    os.environ[k] = saved[k]
        try:
            first = n // 2 if call == "components_update" else n  # the update: the labels of the first half, then the rest appended
            if first:
                ok(lib.smafa_db_append(h, codes.ctypes.data, first))
            labels = np.zeros(max((D + 1) * n if call == "levels" else n, 1), dtype=np.uint32)
            extra = np.zeros((2, max(n, 1)), dtype=np.uint32)
            counts = (C.c_uint64 * (D + 3))()
            if call == "pairs":  # no room for rows: the whole join runs and counts, SMAFA_ERR_CAPACITY (-3) where there are pairs
                ok(lib.smafa_db_self_hits(h, D, None, 0, counts), allowed=(-3,))
            elif call == "components":
                ok(lib.smafa_db_self_components(h, D, labels.ctypes.data, n, counts))
            elif call == "levels":
                ok(lib.smafa_db_self_levels(h, D, labels.ctypes.data, (D + 1) * n, counts))
            elif call == "density":
                ok(lib.smafa_db_self_density(h, D, 3, labels.ctypes.data, extra[0].ctypes.data, n, counts))
            elif call == "peaks":
                ok(lib.smafa_db_self_peaks(h, D, radius, labels.ctypes.data, extra[0].ctypes.data, extra[1].ctypes.data, n, counts))
            elif call == "neighbours":  # the capacity protocol: the degrees alone, then the call sized by them — the census is the last call's
                offsets = np.zeros(n + 1, dtype=np.uint64)
                rc = lib.smafa_db_self_neighbours(h, D, radius, offsets.ctypes.data, None, None, 0, counts)
                if rc == -3:
                    lists = np.zeros((2, counts[0]), dtype=np.uint32)
                    rc = lib.smafa_db_self_neighbours(h, D, radius, offsets.ctypes.data, lists[0].ctypes.data, lists[1].ctypes.data, counts[0], counts)
                ok(rc)
            elif call == "forest":
                edges = np.zeros((max(n, 2) - 1, 3), dtype=np.uint32)
                ok(lib.smafa_db_self_forest(h, D, edges.ctypes.data, len(edges), counts))
            elif call == "reach_forest":  # min_pts 3, as the density call's; the cores too
                edges = np.zeros((max(n, 2) - 1, 3), dtype=np.uint32)
                ok(lib.smafa_db_self_reach_forest(h, D, 3, edges.ctypes.data, len(edges), counts, extra[0].ctypes.data))
            elif call == "stable":  # min_pts 3, min_cluster_size 2; neither the joined levels nor the cores
                ok(lib.smafa_db_self_stable(h, D, 3, 2, labels.ctypes.data, None, None, n, counts))
            elif call == "chimeras":  # counted weights at the peaks call's radius, fold 2, the flags alone
                ok(lib.smafa_db_self_chimeras(h, D, radius, 2, None, labels.ctypes.data, None, None, None, None, None, n, counts))
            elif call == "pairs_since":  # no room for rows, as pairs
                ok(lib.smafa_db_self_hits_since(h, n // 2, D, None, 0, counts), allowed=(-3,))
            else:
                ok(lib.smafa_db_self_components(h, D, labels.ctypes.data, first, counts))
                if n - first:
                    ok(lib.smafa_db_append(h, codes[first:].ctypes.data, n - first))
                ok(lib.smafa_db_self_components_update(h, first, D, labels.ctypes.data, n, counts))
            ms, launches, scans = C.c_float(), C.c_uint32(), C.c_uint32()
            ok(lib.smafa_last_call_stats(h, C.byref(ms), C.byref(launches), C.byref(scans)))
            names = C.create_string_buffer(1 << 16)
            ok(lib.smafa_last_call_kernels(h, names, len(names)))
            out[cid] = {"launches": launches.value, "scans": scans.value, "kernels": [k for k in names.value.decode().split("\n") if k]}
        finally:
            lib.smafa_db_destroy(h)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", required=True)
    ap.add_argument("--calls", help="comma-separated: record only these and merge them into the file at --out")
    args = ap.parse_args()
    path = os.environ.get("SMAFA_AMD_LIB") or os.path.join(ROOT, "smafa_amd", "lib", "libsmafa_amd.so")
    lib = load(path)
    build = lib.smafa_build_id().decode()
    named = args.calls.split(",") if args.calls else CALLS
    unknown = sorted(set(named) - set(EVERY_CALL))
    if unknown:
        raise SystemExit("join_census: no such call: %s (there are: %s)" % (", ".join(unknown), ", ".join(EVERY_CALL)))
    if args.calls:
        if not os.path.exists(args.out):
            raise SystemExit("join_census: --calls merges into %s, which is not there; record the whole table first" % args.out)
        with open(args.out) as f:
            table = json.load(f)
        if table["repeats"] != args.repeat:
            raise SystemExit("join_census: %s was recorded with %d repeats, not %d" % (args.out, table["repeats"], args.repeat))
        # "build" is the build of the calls recorded with the whole table; "builds" names every call's own
        builds = table.setdefault("builds", {})
        for call in table["calls"]:
            builds.setdefault(call, table["build"])
        builds.update({call: build for call in named})
    else:
        table = {"build": build, "repeats": args.repeat, "calls": {}}
    for call in named:
        runs = [census(lib, call) for _ in range(args.repeat)]
        merged = runs[0]
        for cid, rec in merged.items():
            for other in runs[1:]:
                assert other[cid]["scans"] == rec["scans"] and other[cid]["kernels"] == rec["kernels"], (call, cid)
            seen = sorted({r[cid]["launches"] for r in runs})
            if len(seen) > 1:  # the jump rounds differed between the repeats: not pinned
                rec["launches"] = None
                rec["launches_seen"] = seen
        table["calls"][call] = merged
    with open(args.out, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print("join_census: build %s, %d cases of %s -> %s" % (build, sum(len(table["calls"][c]) for c in named), ", ".join(named), args.out))


if __name__ == "__main__":
    main()
