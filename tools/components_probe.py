"""Timing of the single-linkage components (smafa_db_self_components_launch) — profiles/r08_components.txt.

  --part join   one library (SMAFA_AMD_LIB, or this tree's) through ctypes alone, so that a build of the PARENT commit runs
                the very same script: the bench's 10M x 60 stores (amino acids at bound 5, nucleotides at bound 3;
                smafa_amd.synth.subjects), count-only smafa_db_self_launch (cap = 0) and — where the library has it — the
                components call, alternated, 3 runs each after a warm-up, wall clock around call + smafa_sync; one JSON
                line per store appended to --json.
  --part pairs  (b) a store where pairs dominate, synth.related_subjects(families, 100, div 0..0.08) at bound 5: the
                components call against the route a user had before — self_pairs to the host (grow and retry included), then a
                union-find there (numpy; scipy.sparse.csgraph.connected_components where scipy is installed) — with the bytes
                each moves over PCIe; (c) the dense 4 000-row store of the tests at bound 3: link-stage ms and rows per second.
  --part report --json FILE...  -> the text of profiles/r08_components.txt from the JSON lines of the runs above.
The library's per-stage milliseconds come from its level-2 trace line."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
NONE = 0xFFFFFFFF


def traced(lib, fn):
    """fn() with the library's level-2 stderr lines captured -> (fn's result, lines)"""
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        lib.smafa_set_verbosity(2)
        try:
            out = fn()
        finally:
            lib.smafa_set_verbosity(0)
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return out, [ln.strip() for ln in tmp.read().decode(errors="replace").splitlines()]


def stage_ms(lines, what):
    """{"records": ms, "scans": ms, ...} of the last "self-join of" / "components of" line"""
    for ln in reversed(lines):
        if what in ln:
            return {k: float(v) for k, v in re.findall(r"(records|scans|filter|link|flatten) ([0-9.]+) ms", ln)}
    return {}


def part_join(args):
    import torch

    torch.cuda.init()
    from smafa_amd import synth  # (host-side generator only: no library call)

    path = os.environ.get("SMAFA_AMD_LIB") or os.path.join(ROOT, "smafa_amd", "lib", "libsmafa_amd.so")
    lib = C.CDLL(path)
    vp = C.c_void_p
    lib.smafa_build_id.restype = C.c_char_p
    lib.smafa_last_error.restype = C.c_char_p
    lib.smafa_set_verbosity.restype = None
    lib.smafa_db_destroy.restype = None
    lib.smafa_db_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_uint32]
    lib.smafa_db_append.argtypes = [vp, vp, C.c_uint64]
    lib.smafa_db_self_launch.argtypes = [vp, C.c_uint32, vp, C.c_uint64, vp]
    lib.smafa_set_index.argtypes = [vp, C.c_int]
    lib.smafa_sync.argtypes = [vp]
    lib.smafa_db_destroy.argtypes = [vp]
    has_cc = hasattr(lib, "smafa_db_self_components_launch")
    if has_cc:
        lib.smafa_db_self_components_launch.argtypes = [vp, C.c_uint32, vp, vp]

    def ok(rc):
        if rc:
            raise SystemExit("components_probe: %s" % lib.smafa_last_error().decode())

    for label, alphabet, D in (("aa", 1, 5), ("nt", 0, 3)):
        codes = synth.subjects(args.rows, 60, alphabet)
        db = vp()
        ok(lib.smafa_db_create(C.byref(db), 0, alphabet, 60))
        ok(lib.smafa_db_append(db, codes.ctypes.data, len(codes)))
        ok(lib.smafa_set_index(db, 0))
        d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_labels = torch.zeros(len(codes), dtype=torch.int32, device="cuda")

        def join():
            t0 = time.perf_counter()
            ok(lib.smafa_db_self_launch(db, D, None, 0, d_count.data_ptr()))
            ok(lib.smafa_sync(db))
            return (time.perf_counter() - t0) * 1e3

        def components():
            t0 = time.perf_counter()
            ok(lib.smafa_db_self_components_launch(db, D, d_labels.data_ptr(), d_count.data_ptr()))
            ok(lib.smafa_sync(db))
            return (time.perf_counter() - t0) * 1e3

        join()
        pairs = int(d_count.item())
        if has_cc:
            components()
        j, c = [], []
        for _ in range(3):
            j.append(join())
            if has_cc:
                c.append(components())
        rec = {"part": "join", "lib": args.label, "build": lib.smafa_build_id().decode(), "store": label, "rows": len(codes), "bound": D,
               "pairs": pairs, "join_ms": j, "join_stages": stage_ms(traced(lib, join)[1], "self-join of")}
        if has_cc:
            rec["components_ms"] = c
            rec["components_stages"] = stage_ms(traced(lib, components)[1], "components of")
            rec["n_components"] = int(d_count.item())
            lab = d_labels.cpu().numpy().view(np.uint32)
            rec["labels_are_roots"] = bool((lab[lab] == lab).all() and (lab <= np.arange(len(lab))).all())
            rec["n_components_from_labels"] = int((lab == np.arange(len(lab))).sum())
        lib.smafa_db_destroy(db)
        with open(args.json, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec))


def part_pairs(args):
    import smafa_amd
    from smafa_amd import _lib, synth
    from components_cases import dense_store, labels_from_pairs_numpy

    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        connected_components = None
    lib = _lib.lib()
    D = 5
    codes = synth.related_subjects(args.families, 100, div_lo=0.0, div_hi=0.08)
    n = len(codes)
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    store.push(codes)
    store.self_components(D)  # warm-up of both routes' scans
    new, old, host, host_scipy = [], [], [], []
    for _ in range(3):
        t0 = time.perf_counter()
        labels, count = store.self_components(D)
        new.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        pairs = store.self_pairs(D)  # (first buffer of 65 536 rows: the call says how many, and the retry scans again)
        old.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ref = labels_from_pairs_numpy(n, pairs)
        host.append((time.perf_counter() - t0) * 1e3)
        assert ref.tobytes() == labels.tobytes() and count == int((ref == np.arange(n)).sum())
        if connected_components:
            t0 = time.perf_counter()
            g = coo_matrix((np.ones(len(pairs), dtype=np.uint8), (pairs["query"], pairs["subject"])), shape=(n, n))
            k, _ = connected_components(g, directed=False)
            host_scipy.append((time.perf_counter() - t0) * 1e3)
            assert k == count
    stages = stage_ms(traced(lib, lambda: store.self_components(D))[1], "components of")
    rec = {"part": "pairs", "build": smafa_amd.build_id(), "rows": n, "bound": D, "pairs": int(len(pairs)), "n_components": count,
           "components_ms": new, "components_stages": stages, "self_pairs_ms": old, "numpy_union_find_ms": host,
           "scipy_connected_components_ms": host_scipy, "components_bytes": 4 * n + 8, "pairs_bytes": 12 * int(len(pairs)) + 16}
    store.close()
    with open(args.json, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))
    # (c) the dense store: 4 000 x 4 000 rows in the one block's list, every one of them a hook or an early-out
    codes, _ = dense_store()
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_NT)
    store.push(codes)
    store.self_components(3)
    link, wall = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        (labels, count), lines = traced(lib, lambda: store.self_components(3))
        wall.append((time.perf_counter() - t0) * 1e3)
        link.append(stage_ms(lines, "components of"))
        assert count == 1 and not labels.any()
    rec = {"part": "dense", "build": smafa_amd.build_id(), "rows": len(codes), "bound": 3, "rows_linked": len(codes) ** 2,
           "components_ms": wall, "stages": link}
    store.close()
    with open(args.json, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


def part_report(args):
    recs = []
    for path in args.json.split(","):
        with open(path) as f:
            recs += [json.loads(ln) for ln in f if ln.strip()]
    med = statistics.median
    fmt = lambda xs: ", ".join("%.1f" % x for x in xs)  # noqa: E731
    stages = lambda d: ", ".join("%s %.3f ms" % kv for kv in d.items())  # noqa: E731
    this = [r for r in recs if r["part"] == "join" and r["lib"] == "this"]
    out = ["components probe — one MI355X, build id %s (parent commit's library: build id %s)" % (
        this[0]["build"] if this else "?", next((r["build"] for r in recs if r.get("lib") == "parent"), "?")),
        "wall clock around call + smafa_sync, medians of 3 runs; the two libraries ran in alternated processes", ""]
    for store in ("aa", "nt"):
        a1 = [r for r in recs if r["part"] == "join" and r["lib"] == "parent" and r["store"] == store]
        a2 = [r for r in this if r["store"] == store]
        if not a1 or not a2:
            continue
        m1, m2 = med([med(r["join_ms"]) for r in a1]), med([med(r["join_ms"]) for r in a2])
        m3 = med([med(r["components_ms"]) for r in a2])
        r = a2[-1]
        out += ["(a) %s: n = %d, L = 60, bound %d: %d pairs, %d components (labels are roots: %s)" % (
                    store, r["rows"], r["bound"], r["pairs"], r["n_components"], r["labels_are_roots"]),
                "  (a1) parent commit, smafa_db_self_launch cap = 0 : median %.1f ms (per process: %s)" % (
                    m1, "; ".join(fmt(x["join_ms"]) for x in a1)),
                "  (a2) this commit, the same call                 : median %.1f ms (per process: %s)   (a2) / (a1) = %.3f" % (
                    m2, "; ".join(fmt(x["join_ms"]) for x in a2), m2 / m1),
                "       stages: %s" % stages(r["join_stages"]),
                "  (a3) this commit, components                    : median %.1f ms (per process: %s)   (a3) / (a1) = %.3f" % (
                    m3, "; ".join(fmt(x["components_ms"]) for x in a2), m3 / m1),
                "       stages: %s" % stages(r["components_stages"]), ""]
    for r in recs:
        if r["part"] == "pairs":
            out += ["(b) related_subjects: n = %d (families of 100, divergence 0..0.08), bound %d: %d pairs, %d components" % (
                        r["rows"], r["bound"], r["pairs"], r["n_components"]),
                    "  components call                     : median %.1f ms (runs %s); %d bytes to the host" % (
                        med(r["components_ms"]), fmt(r["components_ms"]), r["components_bytes"]),
                    "       stages: %s" % stages(r["components_stages"]),
                    "  self_pairs to the host (grow + retry): median %.1f ms (runs %s); %d bytes to the host" % (
                        med(r["self_pairs_ms"]), fmt(r["self_pairs_ms"]), r["pairs_bytes"]),
                    "  + numpy union-find on the host        : median %.1f ms (runs %s)" % (
                        med(r["numpy_union_find_ms"]), fmt(r["numpy_union_find_ms"]))]
            if r["scipy_connected_components_ms"]:
                out += ["  (or scipy connected_components        : median %.1f ms (runs %s))" % (
                    med(r["scipy_connected_components_ms"]), fmt(r["scipy_connected_components_ms"]))]
            best = med(r["numpy_union_find_ms"])
            if r["scipy_connected_components_ms"]:
                best = min(best, med(r["scipy_connected_components_ms"]))
            out += ["  old route / components = %.1f, bytes ratio %.0f" % (
                (med(r["self_pairs_ms"]) + best) / med(r["components_ms"]), r["pairs_bytes"] / r["components_bytes"]), ""]
        if r["part"] == "dense":
            link = med([s["link"] for s in r["stages"]])
            out += ["(c) dense store: %d rows, bound %d, %d rows linked (one block's list; every pair, mirror and self-pair)" % (
                        r["rows"], r["bound"], r["rows_linked"]),
                    "  components call median %.1f ms; stages of the runs: %s" % (
                        med(r["components_ms"]), " | ".join(stages(s) for s in r["stages"])),
                    "  link stage median %.3f ms = %.2f G rows/s — the contended-hook rate on this store; no ceiling is claimed" % (
                        link, r["rows_linked"] / link / 1e6), ""]
    text = "\n".join(out)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["join", "pairs", "report"], required=True)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--families", type=int, default=10_000)
    ap.add_argument("--label", default="this", help="join: which library this is (this / parent)")
    ap.add_argument("--json", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_components.txt"))
    args = ap.parse_args()
    {"join": part_join, "pairs": part_pairs, "report": part_report}[args.part](args)


if __name__ == "__main__":
    main()
