"""Timing of the stable-cluster call (smafa_db_self_stable_launch) — profiles/r22_stable.txt.

  --part run     one library (SMAFA_AMD_LIB, or this tree's) through ctypes alone, so that a build of the PARENT commit runs
                 the very same script.  Stores (--stores, comma separated) as tools/reach_probe.py: aa / nt — the bench's
                 10M x 60 stores at bound 5 / 3; related — synth.related_subjects(families, 100, div 0..0.08) at bound 5;
                 dense — the 4 000-row store of the tests at bound 3.  Per store, after a warm-up, 3 rounds of: the reach
                 forest call at min_pts 4 (the yardstick: the same join, the same passes), the forest call, the density call
                 at min_pts 4 and — where the library has it — the stable call at min_pts 4, min_cluster_size 0.  Wall clock
                 around call + smafa_sync, and the stage times of the library's level-2 trace line; one JSON line per store
                 appended to --json.
  --part report  --json FILE,FILE...  -> the text of profiles/r22_stable.txt from the JSON lines of the runs above (run the two
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

STAGES = r"(records|scans|keep|tally|cores|span|star|select|count/keep|link|flatten) ([0-9.]+) ms"
M = 4


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
    lib.smafa_db_self_forest_launch.argtypes = [vp, C.c_uint32, vp, vp]
    lib.smafa_db_self_density_launch.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp]
    lib.smafa_db_self_reach_forest_launch.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp]
    has_st = hasattr(lib, "smafa_db_self_stable_launch")
    if has_st:
        lib.smafa_db_self_stable_launch.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.POINTER(C.c_uint64)]

    def ok(rc):
        if rc:
            raise SystemExit("stable_probe: %s" % lib.smafa_last_error().decode())

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
        n = len(codes)
        db = vp()
        ok(lib.smafa_db_create(C.byref(db), 0, alphabet, codes.shape[1]))
        ok(lib.smafa_db_append(db, codes.ctypes.data, n))
        ok(lib.smafa_set_index(db, 0))
        d_counts = torch.zeros(D + 1, dtype=torch.int64, device="cuda")
        d_labels = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_joined = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_edges = torch.zeros(3 * max(n - 1, 1), dtype=torch.int32, device="cuda")
        d_ends = torch.zeros(D + 1, dtype=torch.int64, device="cuda")
        d_cores = torch.zeros(n, dtype=torch.int32, device="cuda")
        count = C.c_uint64(0)

        def timed(call):
            t0 = time.perf_counter()
            ok(call(db))
            ok(lib.smafa_sync(db))
            return (time.perf_counter() - t0) * 1e3

        calls = {
            "reach": lambda h: lib.smafa_db_self_reach_forest_launch(h, D, M, d_edges.data_ptr(), d_ends.data_ptr(), d_cores.data_ptr()),
            "forest": lambda h: lib.smafa_db_self_forest_launch(h, D, d_edges.data_ptr(), d_ends.data_ptr()),
            "density": lambda h: lib.smafa_db_self_density_launch(h, D, M, d_labels.data_ptr(), None, d_counts.data_ptr()),
        }
        lines = {"reach": "reach forest of", "forest": "forest of", "density": "density of"}
        if has_st:
            calls["stable"] = lambda h: lib.smafa_db_self_stable_launch(h, D, M, 0, d_labels.data_ptr(), d_joined.data_ptr(),
                                                                        d_cores.data_ptr(), C.byref(count))
            lines["stable"] = "stable clusters of"
        for call in calls.values():
            timed(call)
        ms = {k: [] for k in calls}
        for _ in range(3):
            for k, call in calls.items():
                ms[k].append(timed(call))
        rec = {"part": "run", "lib": args.label, "build": lib.smafa_build_id().decode(), "store": label, "rows": n, "bound": D, "ms": ms,
               "stages": {k: stages(traced(lib, lambda: timed(call))[1], lines[k]) for k, call in calls.items()}}
        timed(calls["reach"])
        rec["reach_ends"] = d_ends.tolist()
        if has_st:
            timed(calls["stable"])
            rec["clusters"] = int(count.value)
            rec["noise"] = int((d_labels == -1).sum().item())
            rec["joined_levels"] = torch.bincount(d_joined[d_joined >= 0], minlength=D + 1).tolist()
        lib.smafa_db_destroy(db)
        del d_labels, d_edges, d_joined
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
    out = ["stable probe — one MI355X, build id %s (parent commit's library: build id %s)" % (builds.get("this", "?"), builds.get("parent", "?")),
           "wall clock around call + smafa_sync, medians of 3 runs per process; the two libraries ran in alternated processes;",
           "min_pts %d, min_cluster_size 0 (= min_pts)" % M, ""]
    for store in dict.fromkeys(r["store"] for r in recs):
        par = [r for r in recs if r["store"] == store and r["lib"] == "parent"]
        this = [r for r in recs if r["store"] == store and r["lib"] == "this"]
        if not this:
            continue
        r = this[-1]
        out.append("%s: n = %d, bounds 0..%d: reach level ends %s; %d clusters, %d noise rows, rows joined per level %s" % (
            store, r["rows"], r["bound"], r["reach_ends"], r["clusters"], r["noise"], r["joined_levels"]))
        for key in ("reach", "forest", "density"):
            t = med([med(x["ms"][key]) for x in this])
            line = "  this commit, %-8s: median %.1f ms (per process: %s)" % (key, t, "; ".join(fmt(x["ms"][key]) for x in this))
            if par:
                p = med([med(x["ms"][key]) for x in par])
                out.append("  parent commit, %-6s: median %.1f ms (per process: %s)" % (key, p, "; ".join(fmt(x["ms"][key]) for x in par)))
                line += "   this / parent = %.3f" % (t / p)
            out.append(line)
        yard = med([med(x["ms"]["reach"]) for x in (par or this)])
        t = med([med(x["ms"]["stable"]) for x in this])
        out += ["  this commit, stable  : median %.1f ms (per process: %s)   / %s reach = %.3f" % (
                    t, "; ".join(fmt(x["ms"]["stable"]) for x in this), "parent's" if par else "this commit's", t / yard),
                "       stages: %s" % "; ".join(st(x["stages"]["stable"]) for x in this),
                "       reach stages (%s): %s" % ("parent" if par else "this", "; ".join(st(x["stages"]["reach"]) for x in (par or this)))]
        for x in this:
            s, p = x["stages"]["stable"], (par[0] if par else x)["stages"]["reach"]
            out.append("       select %.3f ms against the reach call's span + tally %.3f ms" % (s.get("select", 0.0), p.get("span", 0.0) + p.get("tally", 0.0)))
        out.append("")
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
    ap.add_argument("--label", default="this", help="which library this is: this / parent")
    ap.add_argument("--json", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_stable.txt"))
    args = ap.parse_args()
    {"run": part_run, "report": part_report}[args.part](args)


if __name__ == "__main__":
    main()
