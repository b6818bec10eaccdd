"""Timing of the single-linkage levels (smafa_db_self_levels_launch) — profiles/r09_levels.txt.

  --part store  one library (SMAFA_AMD_LIB, or this tree's) through ctypes alone, so that a build of the PARENT commit runs
                the very same script: the bench's 10M x 60 stores (amino acids at bound 5, nucleotides at bound 3;
                smafa_amd.synth.subjects).  Per store, after a warm-up, 3 rounds of: the components call at D; the
                components calls at 0, 1, .. D (their sum is what the levels call replaces); and — where the library has
                it — the levels call.  Wall clock around call + smafa_sync; one JSON line per store appended to --json.
  --part pairs  (b) a store where pairs dominate, synth.related_subjects(families, 100, div 0..0.08) at bound 5: the stages
                of the levels call beside those of the components call at D; (c) the dense 4 000-row store of the tests at
                bound 3: link-stage ms and rows per second of both calls.  The package's library (SMAFA_AMD_LIB selects
                another build, e.g. one whose hook loop has no early stop, for an A/B); --label names it.
  --part report --json FILE,FILE...  -> the text of profiles/r09_levels.txt from the JSON lines of the runs above.
The library's per-stage milliseconds come from its level-2 trace line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from components_probe import stage_ms, traced  # noqa: E402


def part_store(args):
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
    lib.smafa_set_index.argtypes = [vp, C.c_int]
    lib.smafa_sync.argtypes = [vp]
    lib.smafa_db_destroy.argtypes = [vp]
    lib.smafa_db_self_components_launch.argtypes = [vp, C.c_uint32, vp, vp]
    has_lv = hasattr(lib, "smafa_db_self_levels_launch")
    if has_lv:
        lib.smafa_db_self_levels_launch.argtypes = [vp, C.c_uint32, vp, vp]

    def ok(rc):
        if rc:
            raise SystemExit("levels_probe: %s" % lib.smafa_last_error().decode())

    for label, alphabet, D in (("aa", 1, 5), ("nt", 0, 3)):
        codes = synth.subjects(args.rows, 60, alphabet)
        n = len(codes)
        db = vp()
        ok(lib.smafa_db_create(C.byref(db), 0, alphabet, 60))
        ok(lib.smafa_db_append(db, codes.ctypes.data, n))
        ok(lib.smafa_set_index(db, 0))
        d_counts = torch.zeros(D + 1, dtype=torch.int64, device="cuda")
        d_labels = torch.zeros((D + 1) * n, dtype=torch.int32, device="cuda")

        def components(t):
            t0 = time.perf_counter()
            ok(lib.smafa_db_self_components_launch(db, t, d_labels.data_ptr(), d_counts.data_ptr()))
            ok(lib.smafa_sync(db))
            return (time.perf_counter() - t0) * 1e3

        def levels():
            t0 = time.perf_counter()
            ok(lib.smafa_db_self_levels_launch(db, D, d_labels.data_ptr(), d_counts.data_ptr()))
            ok(lib.smafa_sync(db))
            return (time.perf_counter() - t0) * 1e3

        components(D)
        if has_lv:
            levels()
        at_d, each, lv = [], [], []
        for _ in range(3):
            at_d.append(components(D))
            each.append([components(t) for t in range(D + 1)])
            if has_lv:
                lv.append(levels())
        rec = {"part": "store", "lib": args.label, "build": lib.smafa_build_id().decode(), "store": label, "rows": n, "bound": D,
               "components_ms": at_d, "components_each_ms": each,
               "components_stages": stage_ms(traced(lib, lambda: components(D))[1], "components of")}
        per_bound = []
        for t in range(D + 1):
            components(t)
            per_bound.append(int(d_counts[0].item()))
        rec["n_components_per_bound"] = per_bound
        if has_lv:
            rec["levels_ms"] = lv
            rec["levels_stages"] = stage_ms(traced(lib, levels)[1], "levels 0..")
            rec["n_components"] = d_counts.tolist()
            lab = d_labels.cpu().numpy().view(np.uint32).reshape(D + 1, n)
            components(D)
            rec["row_D_is_the_components_call"] = bool(
                (d_labels[:n].cpu().numpy().view(np.uint32) == lab[D]).all() and rec["n_components"] == per_bound)
        lib.smafa_db_destroy(db)
        with open(args.json, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec))


def part_pairs(args):
    import smafa_amd
    from smafa_amd import _lib, synth
    from components_cases import dense_store

    lib = _lib.lib()
    D = 5
    codes = synth.related_subjects(args.families, 100, div_lo=0.0, div_hi=0.08)
    n = len(codes)
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    store.push(codes)
    store.self_components(D)
    store.self_component_levels(D)
    cc, lv = [], []
    for _ in range(3):
        (row, count), lines = traced(lib, lambda: store.self_components(D))
        cc.append(stage_ms(lines, "components of"))
        (labels, counts), lines = traced(lib, lambda: store.self_component_levels(D))
        lv.append(stage_ms(lines, "levels 0.."))
        assert labels[D].tobytes() == row.tobytes() and counts[D] == count
    rec = {"part": "pairs", "lib": args.label, "build": smafa_amd.build_id(), "rows": n, "bound": D, "n_components": counts,
           "components_stages": cc, "levels_stages": lv}
    store.close()
    with open(args.json, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))
    # (c) the dense store: 4 000 x 4 000 rows in the one block's list, every one of them a hook or an early stop
    codes, _ = dense_store()
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_NT)
    store.push(codes)
    store.self_components(3)
    store.self_component_levels(3)
    cc, lv = [], []
    for _ in range(3):
        (row, count), lines = traced(lib, lambda: store.self_components(3))
        cc.append(stage_ms(lines, "components of"))
        (labels, counts), lines = traced(lib, lambda: store.self_component_levels(3))
        lv.append(stage_ms(lines, "levels 0.."))
        assert counts == [2, 2, 2, 1] and count == 1
    rec = {"part": "dense", "lib": args.label, "build": smafa_amd.build_id(), "rows": len(codes), "bound": 3,
           "rows_linked": len(codes) ** 2, "components_stages": cc, "levels_stages": lv}
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
    stage_med = lambda runs, k: med([s[k] for s in runs])  # noqa: E731
    this = [r for r in recs if r["part"] == "store" and r["lib"] == "this"]
    out = ["levels probe — one MI355X, build id %s (parent commit's library: build id %s)" % (
        this[0]["build"] if this else "?", next((r["build"] for r in recs if r.get("lib") == "parent"), "?")),
        "wall clock around call + smafa_sync, medians of 3 runs per process; the two libraries ran in alternated processes", ""]
    for store in ("aa", "nt"):
        a1 = [r for r in recs if r["part"] == "store" and r["lib"] == "parent" and r["store"] == store]
        a2 = [r for r in this if r["store"] == store]
        if not a1 or not a2:
            continue
        sums = lambda r: [sum(x) for x in r["components_each_ms"]]  # noqa: E731
        p_d, p_sum = med([med(r["components_ms"]) for r in a1]), med([med(sums(r)) for r in a1])
        t_d, t_lv = med([med(r["components_ms"]) for r in a2]), med([med(r["levels_ms"]) for r in a2])
        r = a2[-1]
        out += ["(a) %s: n = %d, L = 60, bounds 0..%d: components per level %s (row D and the counts are the components calls': %s)" % (
                    store, r["rows"], r["bound"], r["n_components"], r["row_D_is_the_components_call"]),
                "  (a1) parent commit, components at D          : median %.1f ms (per process: %s)" % (
                    p_d, "; ".join(fmt(x["components_ms"]) for x in a1)),
                "       stages: %s" % stages(a1[-1]["components_stages"]),
                "  (a2) parent commit, components at 0..D, summed: median %.1f ms (per process: %s)" % (
                    p_sum, "; ".join(fmt(sums(x)) for x in a1)),
                "       per bound, last process: %s" % fmt([med([x[t] for x in a1[-1]["components_each_ms"]]) for t in range(r["bound"] + 1)]),
                "  (a3) this commit, components at D            : median %.1f ms (per process: %s)   (a3) / (a1) = %.3f" % (
                    t_d, "; ".join(fmt(x["components_ms"]) for x in a2), t_d / p_d),
                "       stages: %s" % stages(r["components_stages"]),
                "  (a4) this commit, levels 0..D                : median %.1f ms (per process: %s)   (a4) / (a1) = %.3f, (a2) / (a4) = %.2f" % (
                    t_lv, "; ".join(fmt(x["levels_ms"]) for x in a2), t_lv / p_d, p_sum / t_lv),
                "       stages: %s" % "; ".join(stages(x["levels_stages"]) for x in a2), ""]
    for r in recs:
        if r["part"] == "pairs":
            out += ["(b) [%s, build %s] related_subjects: n = %d (families of 100, divergence 0..0.08), bound %d: components per level %s" % (
                        r["lib"], r["build"], r["rows"], r["bound"], r["n_components"]),
                    "  components at D: link median %.3f ms, flatten median %.3f ms; runs: %s" % (
                        stage_med(r["components_stages"], "link"), stage_med(r["components_stages"], "flatten"),
                        " | ".join(stages(s) for s in r["components_stages"])),
                    "  levels 0..D    : link median %.3f ms, flatten median %.3f ms; runs: %s" % (
                        stage_med(r["levels_stages"], "link"), stage_med(r["levels_stages"], "flatten"),
                        " | ".join(stages(s) for s in r["levels_stages"])),
                    "  flatten of levels / ((D + 1) x flatten of components) = %.2f" % (
                        stage_med(r["levels_stages"], "flatten") / ((r["bound"] + 1) * stage_med(r["components_stages"], "flatten"))), ""]
        if r["part"] == "dense":
            l_cc, l_lv = stage_med(r["components_stages"], "link"), stage_med(r["levels_stages"], "link")
            out += ["(c) [%s, build %s] dense store: %d rows, bound %d, %d rows linked (one block's list; every pair, mirror and self-pair)" % (
                        r["lib"], r["build"], r["rows"], r["bound"], r["rows_linked"]),
                    "  components at D: link stage median %.3f ms = %.2f G rows/s (runs %s)" % (
                        l_cc, r["rows_linked"] / l_cc / 1e6, ", ".join("%.3f" % s["link"] for s in r["components_stages"])),
                    "  levels 0..D    : link stage median %.3f ms = %.2f G rows/s (runs %s), flatten %.3f ms" % (
                        l_lv, r["rows_linked"] / l_lv / 1e6, ", ".join("%.3f" % s["link"] for s in r["levels_stages"]),
                        stage_med(r["levels_stages"], "flatten")), ""]
    text = "\n".join(out)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["store", "pairs", "report"], required=True)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--families", type=int, default=10_000)
    ap.add_argument("--label", default="this", help="which library this is (store: this / parent; pairs: this / visit-all)")
    ap.add_argument("--json", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_levels.txt"))
    args = ap.parse_args()
    {"store": part_store, "pairs": part_pairs, "report": part_report}[args.part](args)


if __name__ == "__main__":
    main()
