"""Timing of the abundance peaks with given weights (smafa_db_self_peaks_weighted) — profiles/r31_peaks_weighted.txt.

  --part ab      one library (SMAFA_AMD_LIB, or this tree's) through ctypes alone, so that a build of the PARENT commit runs the very
                 same script: smafa_db_self_peaks (r = 0 and r = D) and smafa_db_self_chimeras — the two calls that launch
                 smafa_pk::init_peaks_kernel and smafa_pk::weigh_keep_kernel, which gained arguments — 3 runs each after a warm-up,
                 wall clock around the host-form call, device time from smafa_last_call_stats, the weigh/keep stage from the
                 library's level-2 line.  Stores: (s) synth.subjects(--rows, 60 aa) at bound 5, where pairs are rare; (r)
                 synth.related_subjects(--families, 100) at bound 5, where the weigh/keep pass has work.  Run in alternated
                 processes, parent and this tree; --label names the library.
  --part sizes   this tree's library: a raw store of --raw rows drawn with repeats from --families x 100 related rows, sizes skewed
                 so that one sequence holds 1 % of the rows.  smafa_db_self_peaks on the raw store at bound 5, r = 0, beside np.unique
                 on the host + a fresh store of the distinct rows + smafa_db_self_peaks_weighted on it; the pairs at divergence 0
                 the raw side keeps (sum of c(c-1)/2, from the sizes), and the identity checked.
  --part report --json FILE,FILE  -> the text of the profile from the JSON lines of the runs above."""
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


def med(xs):
    return statistics.median(xs)


def stage(lines, what, name):
    for ln in reversed(lines):
        if what in ln:
            m = re.search(re.escape(name) + r" ([0-9.]+) ms", ln)
            return float(m.group(1)) if m else None
    return None


def part_ab(args):
    from smafa_amd import synth

    path = os.environ.get("SMAFA_AMD_LIB") or os.path.join(ROOT, "smafa_amd", "lib", "libsmafa_amd.so")
    l = C.CDLL(path)
    vp, u32 = C.c_void_p, C.c_uint32
    l.smafa_build_id.restype = C.c_char_p
    l.smafa_last_error.restype = C.c_char_p
    l.smafa_set_verbosity.argtypes = [C.c_int]
    l.smafa_db_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, u32]
    l.smafa_db_append.argtypes = [vp, vp, C.c_uint64]
    l.smafa_db_destroy.argtypes = [vp]
    l.smafa_db_self_peaks.argtypes = [vp, u32, u32, vp, vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    l.smafa_db_self_chimeras.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    l.smafa_last_call_stats.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(u32), C.POINTER(u32)]
    out = {"part": "ab", "label": args.label, "build_id": l.smafa_build_id().decode(), "cases": {}}
    for name, codes in (("(s) subjects %d x 60 aa" % args.rows, synth.subjects(args.rows, 60, 1)),
                        ("(r) related %d x 100, 60 aa" % args.families, synth.related_subjects(args.families, 100, div_lo=0.0, div_hi=0.08))):
        codes = np.ascontiguousarray(codes)
        n = len(codes)
        h = vp()
        assert l.smafa_db_create(C.byref(h), 0, 1, 60) == 0 and l.smafa_db_append(h, codes.ctypes.data, n) == 0, l.smafa_last_error()
        arrays = [np.zeros(n, dtype=np.uint32) for _ in range(6)]
        count = C.c_uint64(0)
        calls = {"peaks r=0": (lambda: l.smafa_db_self_peaks(h, 5, 0, *(a.ctypes.data for a in arrays[:3]), n, C.byref(count)), "peaks of", "weigh/keep"),
                 "peaks r=D": (lambda: l.smafa_db_self_peaks(h, 5, 5, *(a.ctypes.data for a in arrays[:3]), n, C.byref(count)), "peaks of", "weigh/keep"),
                 "chimeras": (lambda: l.smafa_db_self_chimeras(h, 5, 0, 2, None, *(a.ctypes.data for a in arrays), n, C.byref(count)), "chimeras of", "weigh/keep")}
        for call, (fn, what, stage_name) in calls.items():
            assert fn() == 0, l.smafa_last_error()  # warm-up
            wall, dev, st = [], [], []
            for _ in range(3):
                t0 = time.perf_counter()
                rc, lines = traced(l, fn)
                wall.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0
                ms = C.c_float(0)
                l.smafa_last_call_stats(h, C.byref(ms), None, None)
                dev.append(ms.value)
                st.append(stage(lines, what, stage_name))
            out["cases"]["%s: %s" % (name, call)] = {"wall_ms": wall, "device_ms": dev, "weigh_keep_ms": st, "answer": int(count.value)}
        l.smafa_db_destroy(h)
    print(json.dumps(out), flush=True)


def part_sizes(args):
    import smafa_amd
    from smafa_amd import _lib, synth
    from peaks_weighted_cases import expected_derep, lifted

    rng = np.random.default_rng(5)
    pool = synth.related_subjects(args.families, 100, div_lo=0.0, div_hi=0.08)
    u = len(pool)
    p = 1.0 / (1.0 + np.arange(u)) ** 0.5  # skewed sizes ...
    p[0] = 0.0
    p = p / p.sum() * 0.99
    p[0] = 0.01                            # ... and one sequence on 1 % of the rows
    codes = np.ascontiguousarray(pool[rng.choice(u, size=args.raw, p=p / p.sum())])
    D = 5
    out = {"part": "sizes", "build_id": smafa_amd.build_id(), "raw_rows": int(args.raw)}
    raw = smafa_amd.SubjectStore(60, 1)
    raw.push(codes)
    raw.self_peaks(D, 0)
    wall, dev = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        want = raw.self_peaks(D, 0)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(raw.last_call_stats()["kernel_ms"])
    out["raw"] = {"wall_ms": wall, "device_ms": dev, "n_peaks": want[3]}
    t0 = time.perf_counter()
    derep = expected_derep(codes)
    out["np_unique_ms"] = (time.perf_counter() - t0) * 1e3
    sizes = derep[2].astype(np.int64)
    out["distinct_rows"] = int(len(sizes))
    out["largest_size"] = int(sizes.max())
    out["raw_pairs_at_0"] = int((sizes * (sizes - 1) // 2).sum())
    t0 = time.perf_counter()
    uniques = smafa_amd.SubjectStore(60, 1)
    uniques.push(np.ascontiguousarray(codes[derep[1]]))
    out["push_ms"] = (time.perf_counter() - t0) * 1e3
    uniques.self_peaks(D, 0, weights_in=derep[2])
    wall, dev, kept = [], [], []
    for _ in range(3):
        t0 = time.perf_counter()
        got, lines = traced(_lib.lib(), lambda: uniques.self_peaks(D, 0, weights_in=derep[2]))
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(uniques.last_call_stats()["kernel_ms"])
        m = [re.search(r"(\d+) pairs kept", ln) for ln in lines if "weighted peaks of" in ln]
        kept.append(int(m[-1].group(1)) if m and m[-1] else None)
    out["uniques"] = {"wall_ms": wall, "device_ms": dev, "pairs_kept": kept, "n_peaks": got[3]}
    out["identity_holds"] = not lifted(want, derep, got)
    print(json.dumps(out), flush=True)


def part_report(args):
    recs = [json.loads(ln) for f in args.json.split(",") for ln in open(f) if ln.startswith("{")]
    ab = [r for r in recs if r["part"] == "ab"]
    print("peaks with given weights: the existing calls against the parent's build, and what the sizes buy\n")
    for label in sorted({r["label"] for r in ab}):
        print("build %s: %s, %d processes" % (label, sorted({r["build_id"] for r in ab if r["label"] == label}), sum(r["label"] == label for r in ab)))
    print()
    for case in (ab[0]["cases"] if ab else {}):
        print(case)
        by = {}
        for label in sorted({r["label"] for r in ab}):
            runs = [r["cases"][case] for r in ab if r["label"] == label]
            by[label] = {k: med([x for r in runs for x in r[k] if x is not None]) for k in ("wall_ms", "device_ms", "weigh_keep_ms")}
            per = [med(r["device_ms"]) for r in runs]
            print("  %-7s wall %9.3f ms, device %9.3f ms (per process %s), weigh/keep %7.3f ms" % (
                label, by[label]["wall_ms"], by[label]["device_ms"], ", ".join("%.3f" % x for x in per), by[label]["weigh_keep_ms"]))
        if len(by) == 2 and "parent" in by:
            other = next(k for k in by if k != "parent")
            print("  %s / parent: device %+.2f %%, weigh/keep %+.2f %%" % (other, 100 * (by[other]["device_ms"] / by["parent"]["device_ms"] - 1),
                                                                          100 * (by[other]["weigh_keep_ms"] / by["parent"]["weigh_keep_ms"] - 1)))
    for r in recs:
        if r["part"] == "sizes":
            print("\nsizes: %d raw rows, %d distinct, the largest on %d rows (build %s)" % (r["raw_rows"], r["distinct_rows"], r["largest_size"], r["build_id"]))
            print("  self_peaks on the raw rows, D = 5, r = 0: wall %.1f ms, device %.1f ms; pairs at divergence 0 alone: %d" % (
                med(r["raw"]["wall_ms"]), med(r["raw"]["device_ms"]), r["raw_pairs_at_0"]))
            print("  np.unique on the host %.1f ms + a fresh store of the distinct rows %.1f ms + weighted peaks: wall %.1f ms, device %.1f ms; pairs kept %s" % (
                r["np_unique_ms"], r["push_ms"], med(r["uniques"]["wall_ms"]), med(r["uniques"]["device_ms"]), r["uniques"]["pairs_kept"][-1]))
            print("  peaks %d and %d; the lifted identity holds: %s" % (r["raw"]["n_peaks"], r["uniques"]["n_peaks"], r["identity_holds"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=("ab", "sizes", "report"))
    ap.add_argument("--label", default="this")
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--families", type=int, default=2000)
    ap.add_argument("--raw", type=int, default=1_000_000)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    {"ab": part_ab, "sizes": part_sizes, "report": part_report}[a.part](a)
