"""Timing of the minimum spanning forest (smafa_db_self_forest_launch) — profiles/r19_forest.txt.

  --part run     one library (SMAFA_AMD_LIB, or this tree's) through ctypes alone, so that a build of the PARENT commit runs
                 the very same script.  Stores (--stores, comma separated): aa / nt — the bench's 10M x 60 stores
                 (smafa_amd.synth.subjects; amino acids at bound 5, nucleotides at bound 3); related —
                 synth.related_subjects(families, 100, div 0..0.08) at bound 5, where pairs dominate; dense — the 4 000-row
                 store of the tests at bound 3 (--bound: another bound, e.g. 60 on the dense store for the star stage).  Per store, after a warm-up, 3 rounds of: the components call at D, the
                 levels call (the yardstick: the same single join) and — where the library has it — the forest call, and
                 once the forest call of a handle made under SMAFA_DENSITY_KEEP_MAX=0 (the slow path: one more join per
                 class).  Wall clock around call + smafa_sync, and the stage times of the library's level-2 trace line; one
                 JSON line per store appended to --json.
  --part report  --json FILE,FILE...  -> the text of profiles/r19_forest.txt from the JSON lines of the runs above (run the two
                 libraries in alternated processes, --label parent / this)."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from components_probe import traced  # noqa: E402

STAGES = r"(records|scans|keep|span|star|link|flatten) ([0-9.]+) ms"


def stages(lines, what):
    for ln in reversed(lines):
        if what in ln:
            return {k: float(v) for k, v in re.findall(STAGES, ln)}
    return {}


def part_run(args):
    import torch

    torch.cuda.init()
    from smafa_amd import synth  # (host-side generators only: no library call)
    from components_cases import dense_store

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
    lib.smafa_db_self_levels_launch.argtypes = [vp, C.c_uint32, vp, vp]
    has_sf = hasattr(lib, "smafa_db_self_forest_launch")
    if has_sf:
        lib.smafa_db_self_forest_launch.argtypes = [vp, C.c_uint32, vp, vp]

    def ok(rc):
        if rc:
            raise SystemExit("forest_probe: %s" % lib.smafa_last_error().decode())

    def make(codes, alphabet):
        db = vp()
        ok(lib.smafa_db_create(C.byref(db), 0, alphabet, codes.shape[1]))
        ok(lib.smafa_db_append(db, codes.ctypes.data, len(codes)))
        ok(lib.smafa_set_index(db, 0))
        return db

    for label in args.stores.split(","):
        if label in ("aa", "nt"):
            alphabet, D = (1, 5) if label == "aa" else (0, 3)
            codes = synth.subjects(args.rows, 60, alphabet)
        elif label == "related":
            alphabet, D = 1, 5
            codes = synth.related_subjects(args.families, 100, div_lo=0.0, div_hi=0.08)
        else:
            alphabet, D = 0, 3
            codes = dense_store()[0]
        if args.bound is not None:  # (a bound >= the rows' length: the star stage)
            D = args.bound
        n = len(codes)
        db = make(codes, alphabet)
        d_counts = torch.zeros(D + 1, dtype=torch.int64, device="cuda")
        d_labels = torch.zeros((D + 1) * n, dtype=torch.int32, device="cuda")
        d_edges = torch.zeros(3 * max(n - 1, 1), dtype=torch.int32, device="cuda")
        d_ends = torch.zeros(D + 1, dtype=torch.int64, device="cuda")

        def timed(call):
            t0 = time.perf_counter()
            ok(call())
            ok(lib.smafa_sync(db))
            return (time.perf_counter() - t0) * 1e3

        components = lambda h=None: timed(lambda: lib.smafa_db_self_components_launch(h or db, D, d_labels.data_ptr(), d_counts.data_ptr()))  # noqa: E731
        levels = lambda h=None: timed(lambda: lib.smafa_db_self_levels_launch(h or db, D, d_labels.data_ptr(), d_counts.data_ptr()))  # noqa: E731
        forest = lambda h=None: timed(lambda: lib.smafa_db_self_forest_launch(h or db, D, d_edges.data_ptr(), d_ends.data_ptr()))  # noqa: E731
        components()
        levels()
        if has_sf:
            forest()
        cc, lv, sf = [], [], []
        for _ in range(3):
            cc.append(components())
            lv.append(levels())
            if has_sf:
                sf.append(forest())
        rec = {"part": "run", "lib": args.label, "build": lib.smafa_build_id().decode(), "store": label, "rows": n, "bound": D,
               "components_ms": cc, "levels_ms": lv,
               "components_stages": stages(traced(lib, components)[1], "components of"),
               "levels_stages": stages(traced(lib, levels)[1], "levels 0..")}
        levels()
        rec["n_components"] = d_counts.tolist()
        if has_sf:
            rec["forest_ms"] = sf
            rec["forest_stages"] = stages(traced(lib, forest)[1], "forest of")
            rec["level_ends"] = d_ends.tolist()
            rec["ends_are_n_minus_components"] = rec["level_ends"] == [n - c for c in rec["n_components"]]
            os.environ["SMAFA_DENSITY_KEEP_MAX"] = "0"
            slow = make(codes, alphabet)
            del os.environ["SMAFA_DENSITY_KEEP_MAX"]
            forest(slow)
            ms, lines = traced(lib, lambda: forest(slow))
            rec["forest_slow_ms"], rec["forest_slow_stages"] = ms, stages(lines, "forest of")
            rec["slow_ends_equal"] = d_ends.tolist() == rec["level_ends"]
            lib.smafa_db_destroy(slow)
        lib.smafa_db_destroy(db)
        del d_labels, d_edges
        with open(args.json, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)


def part_report(args):
    recs = []
    for path in args.json.split(","):
        with open(path) as f:
            recs += [json.loads(ln) for ln in f if ln.strip()]
    med = statistics.median
    fmt = lambda xs: ", ".join("%.1f" % x for x in xs)  # noqa: E731
    st = lambda d: ", ".join("%s %.3f ms" % kv for kv in d.items())  # noqa: E731
    builds = {r["lib"]: r["build"] for r in recs}
    out = ["forest probe — one MI355X, build id %s (parent commit's library: build id %s)" % (builds.get("this", "?"), builds.get("parent", "?")),
           "wall clock around call + smafa_sync, medians of 3 runs per process; the two libraries ran in alternated processes", ""]
    for store in dict.fromkeys(r["store"] for r in recs):
        par = [r for r in recs if r["store"] == store and r["lib"] == "parent"]
        this = [r for r in recs if r["store"] == store and r["lib"] == "this"]
        if not this:
            continue
        r = this[-1]
        out.append("%s: n = %d, bounds 0..%d: components per level %s, level ends %s (n - components: %s; the slow path's the same: %s)" % (
            store, r["rows"], r["bound"], r["n_components"], r["level_ends"], r["ends_are_n_minus_components"], r["slow_ends_equal"]))
        for name, key in (("components at D", "components_ms"), ("levels 0..D", "levels_ms")):
            t = med([med(x[key]) for x in this])
            line = "  this commit, %-16s: median %.1f ms (per process: %s)" % (name, t, "; ".join(fmt(x[key]) for x in this))
            if par:
                p = med([med(x[key]) for x in par])
                out.append("  parent commit, %-14s: median %.1f ms (per process: %s)" % (name, p, "; ".join(fmt(x[key]) for x in par)))
                line += "   this / parent = %.3f" % (t / p)
            out.append(line)
        f_ms = med([med(x["forest_ms"]) for x in this])
        yard = med([med(x["levels_ms"]) for x in (par or this)])
        out += ["  this commit, forest 0..D      : median %.1f ms (per process: %s)   forest / %s levels = %.3f" % (
                    f_ms, "; ".join(fmt(x["forest_ms"]) for x in this), "parent's" if par else "this commit's", f_ms / yard),
                "       forest stages: %s" % "; ".join(st(x["forest_stages"]) for x in this),
                "       levels stages: %s" % "; ".join(st(x["levels_stages"]) for x in (par or this)),
                "  slow path (SMAFA_DENSITY_KEEP_MAX=0): %s ms; stages: %s" % (
                    fmt([x["forest_slow_ms"] for x in this]), "; ".join(st(x["forest_slow_stages"]) for x in this)), ""]
    text = "\n".join(out)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["run", "report"], required=True)
    ap.add_argument("--stores", default="aa,nt,related,dense")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--families", type=int, default=10_000)
    ap.add_argument("--bound", type=int, help="this bound in place of the store's own")
    ap.add_argument("--label", default="this", help="which library this is: this / parent")
    ap.add_argument("--json", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_forest.txt"))
    args = ap.parse_args()
    {"run": part_run, "report": part_report}[args.part](args)


if __name__ == "__main__":
    main()
