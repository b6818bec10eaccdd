"""Timing of the abundance-peak clusters (smafa_db_self_peaks) beside the components and density calls —
profiles/r13_peaks.txt.

  --part run    one process, this tree's library.  Per store: the components call at the bound, the density call (min_pts
                20, every pair kept: its count/keep stage reserves room in the kept list once per WAVE), and the peaks call
                at r = D (the same adds as the density call) and at r = 0 (its weigh/keep stage reserves once per WORKGROUP
                and loop iteration), alternated, 3 runs each after a warm-up, wall clock around the host-form call; the
                library's per-stage milliseconds and the jump rounds come from its level-2 trace line.
                Stores: (a) the bench's 10M x 60 stores (amino acids at bound 5, nucleotides at bound 3;
                smafa_amd.synth.subjects), where pairs are rare and the scans are everything; (b)
                synth.related_subjects(families, 100, div 0..0.08) at bound 5, where pairs dominate; (c) the dense 4 000-row
                store of the tests at bound 3.
  --part old    one library (SMAFA_AMD_LIB, or this tree's) through ctypes alone, so that a build of the PARENT commit runs
                the very same script: the components, levels and density calls on stores (b) and (c), 3 runs each after a
                warm-up.  Run in alternated processes, parent and this tree; --label names the library.
  --part report --json FILE,FILE  -> the text of profiles/r13_peaks.txt from the JSON lines of the runs above."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from components_probe import traced  # noqa: E402

STAGES = r"(records|scans|count/keep|weigh/keep|link|climb|flatten|settle\+jump) ([0-9.]+) ms"


def stage_ms(lines, what):
    for ln in reversed(lines):
        if what in ln:
            d = {k: float(v) for k, v in re.findall(STAGES, ln)}
            m = re.search(r"in (\d) join", ln)
            if m:
                d["joins"] = int(m.group(1))
            m = re.search(r"in (\d+) jump round", ln)
            if m:
                d["jump_rounds"] = int(m.group(1))
            return d
    return {}


def stores(args):
    from smafa_amd import synth
    from components_cases import dense_store

    if "a" in args.stores:
        yield "(a) aa: synth.subjects", synth.subjects(args.rows, 60, 1), 1, 5
        yield "(a) nt: synth.subjects", synth.subjects(args.rows, 60, 0), 0, 3
    if "b" in args.stores:
        yield ("(b) related_subjects, families of 100, divergence 0..0.08",
               synth.related_subjects(args.families, 100, div_lo=0.0, div_hi=0.08), 1, 5)
    if "c" in args.stores:
        yield "(c) dense store: 2 000 + 2 000 copies at distance 3", dense_store()[0], 0, 3


def part_run(args):
    import smafa_amd
    from smafa_amd import _lib

    lib = _lib.lib()
    for name, codes, alphabet, D in stores(args):
        store = smafa_amd.SubjectStore(codes.shape[1], alphabet)
        store.push(codes)
        store.set_index(0)
        calls = {"components": lambda: store.self_components(D), "density": lambda: store.self_density(D, args.min_pts),
                 "peaks, r = D": lambda: store.self_peaks(D, D), "peaks, r = 0": lambda: store.self_peaks(D, 0)}
        what = {"components": "components of", "density": "density of", "peaks, r = D": "peaks of", "peaks, r = 0": "peaks of"}
        for fn in calls.values():
            fn()  # warm-up
        wall, stages = {k: [] for k in calls}, {k: [] for k in calls}
        for _ in range(3):
            for k, fn in calls.items():
                t0 = time.perf_counter()
                res, lines = traced(lib, fn)
                wall[k].append((time.perf_counter() - t0) * 1e3)
                stages[k].append(stage_ms(lines, what[k]))
        dens, ball, copies = store.self_density(D, args.min_pts), store.self_peaks(D, D), store.self_peaks(D, 0)
        assert ball[2].tobytes() == (dens[1] + 1).astype(np.uint32).tobytes()
        for labels, parents, weights, n_peaks in (ball, copies):
            assert (labels[labels] == labels).all() and n_peaks == int((parents == np.arange(len(codes))).sum())
        rec = {"part": "run", "store": name, "build": smafa_amd.build_id(), "rows": len(codes), "bound": D, "min_pts": args.min_pts,
               "pairs": int(dens[1].astype(np.int64).sum()) // 2, "components": store.self_components(D)[1],
               "peaks": {"r = D": ball[3], "r = 0": copies[3]}, "wall_ms": wall, "stages": stages}
        store.close()
        with open(args.json, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec))


def part_old(args):
    path = os.environ.get("SMAFA_AMD_LIB") or os.path.join(ROOT, "smafa_amd", "lib", "libsmafa_amd.so")
    lib = C.CDLL(path)
    vp, u64p = C.c_void_p, C.POINTER(C.c_uint64)
    lib.smafa_build_id.restype = C.c_char_p
    lib.smafa_last_error.restype = C.c_char_p
    lib.smafa_set_verbosity.restype = None
    lib.smafa_db_destroy.restype = None
    lib.smafa_db_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_uint32]
    lib.smafa_db_append.argtypes = [vp, vp, C.c_uint64]
    lib.smafa_set_index.argtypes = [vp, C.c_int]
    lib.smafa_db_destroy.argtypes = [vp]
    lib.smafa_db_self_components.argtypes = [vp, C.c_uint32, vp, C.c_uint64, u64p]
    lib.smafa_db_self_levels.argtypes = [vp, C.c_uint32, vp, C.c_uint64, u64p]
    lib.smafa_db_self_density.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64, u64p]

    def ok(rc):
        if rc:
            raise SystemExit("peaks_probe: %s" % lib.smafa_last_error().decode())

    for name, codes, alphabet, D in stores(args):
        n = len(codes)
        h = vp()
        ok(lib.smafa_db_create(C.byref(h), 0, alphabet, codes.shape[1]))
        ok(lib.smafa_db_append(h, codes.ctypes.data, n))
        ok(lib.smafa_set_index(h, 0))
        labels = np.zeros((D + 1) * n, dtype=np.uint32)
        degrees = np.zeros(n, dtype=np.uint32)
        counts = (C.c_uint64 * (D + 3))()
        calls = {"components": lambda: ok(lib.smafa_db_self_components(h, D, labels.ctypes.data, n, counts)),
                 "levels": lambda: ok(lib.smafa_db_self_levels(h, D, labels.ctypes.data, (D + 1) * n, counts)),
                 "density": lambda: ok(lib.smafa_db_self_density(h, D, args.min_pts, labels.ctypes.data, degrees.ctypes.data, n, counts))}
        for fn in calls.values():
            fn()  # warm-up
        wall = {k: [] for k in calls}
        for _ in range(3):
            for k, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                wall[k].append((time.perf_counter() - t0) * 1e3)
        lib.smafa_db_destroy(h)
        rec = {"part": "old", "label": args.label, "store": name, "build": lib.smafa_build_id().decode(), "rows": n, "bound": D,
               "wall_ms": wall}
        with open(args.json, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec))


def part_report(args):
    recs = []
    for path in args.json.split(","):
        with open(path) as f:
            recs += [json.loads(ln) for ln in f if ln.strip()]
    med = statistics.median
    runs = [r for r in recs if r["part"] == "run"]
    out = ["peaks probe — one MI355X, build id %s" % (runs[0]["build"] if runs else "?"),
           "wall clock around the host-form call, medians of 3 alternated runs after a warm-up; per-stage ms from the level-2 trace", ""]
    for r in runs:
        out.append("%s: n = %d, bound %d: %d pairs, %d components; peaks %s" % (
            r["store"], r["rows"], r["bound"], r["pairs"], r["components"], r["peaks"]))
        st = {}
        for k in ("components", "density", "peaks, r = D", "peaks, r = 0"):
            keys = [s for s in ("records", "scans", "count/keep", "weigh/keep", "link", "climb", "flatten", "settle+jump")
                    if s in r["stages"][k][0]]
            st[k] = {s: med([x[s] for x in r["stages"][k]]) for s in keys}
            line = "  %-14s wall %9.1f ms (runs %s); %s" % (k, med(r["wall_ms"][k]), ", ".join("%.1f" % x for x in r["wall_ms"][k]),
                                                          ", ".join("%s %.3f ms" % kv for kv in st[k].items()))
            if k != "components":
                line += "; joins %s; scans / components' scans = %.3f" % (r["stages"][k][0].get("joins"),
                                                                          st[k]["scans"] / st["components"]["scans"])
            if k.startswith("peaks"):
                line += "; jump rounds %s" % r["stages"][k][0].get("jump_rounds")
                if st["density"].get("count/keep"):
                    line += "; weigh/keep (per workgroup) / density's count/keep (per wave) = %.3f" % (
                        st[k]["weigh/keep"] / st["density"]["count/keep"])
            out.append(line)
        out.append("")
    old = [r for r in recs if r["part"] == "old"]
    if old:
        out.append("the existing calls, this commit's library against the parent commit's, alternated processes (medians of 3 per process):")
        for store in sorted({r["store"] for r in old}):
            for call in ("components", "levels", "density"):
                per = {}
                for r in old:
                    if r["store"] == store:
                        per.setdefault((r["label"], r["build"]), []).append(med(r["wall_ms"][call]))
                line = "  %s, %s:" % (store, call)
                meds = {}
                for (label, build), v in sorted(per.items()):
                    meds[label] = med(v)
                    line += " %s (build %s) %.1f ms (per process: %s);" % (label, build, med(v), ", ".join("%.1f" % x for x in v))
                if "this" in meds and "parent" in meds:
                    line += " this / parent = %.3f" % (meds["this"] / meds["parent"])
                out.append(line)
        out.append("")
    text = "\n".join(out)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["run", "old", "report"], required=True)
    ap.add_argument("--stores", default="abc")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--families", type=int, default=10_000)
    ap.add_argument("--min-pts", type=int, default=20)
    ap.add_argument("--label", default="this")
    ap.add_argument("--json", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_peaks.txt"))
    args = ap.parse_args()
    {"run": part_run, "old": part_old, "report": part_report}[args.part](args)


if __name__ == "__main__":
    main()
