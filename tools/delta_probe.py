"""Timing of the delta self-join (smafa_db_self_since_launch) beside the full join (smafa_db_self_launch) of the same store, and
of the six older self-join calls on any build of the library — profiles/r17_delta_join.txt.

  --part run    one process, this tree's library.  Per store (the bench's 10M x 60 stores: amino acids at bound 5, nucleotides
                at bound 3; smafa_amd.synth.subjects) and per case — m = 10 000, 100 000 and 1 000 000 new rows in append order,
                and m = 100 000 new rows appended in SORTED order (the rows' own lexicographic order: their positions in the
                sorted store then run with their numbers) — the store is built from its first n - m rows and the m rows
                appended behind them.  The count-only delta call (cap = 0) and the count-only full call, without and with a
                built block index: after a warm-up, 3 alternated runs timed by the wall clock around the launch form and a
                sync, nothing else inside the timed region; then 3 alternated runs under the level-2 trace, untimed, for the
                gather / scans / filter milliseconds.  Checked per store: the delta call at first_row = 0 counts what the full
                call counts, and every run repeats its warm-up's count.  --stores related: synth.related_subjects(families,
                100, div 0..0.08) at bound 5 in their place, where pairs dominate and the filter stage has work.
  --part old    one library (SMAFA_AMD_LIB, or this tree's) through ctypes alone, so that a build of the PARENT commit runs
                the very same script: the six older calls — pairs (count only), components, levels, density, peaks,
                neighbours — in their launch forms on the ONE-APPEND bench stores, 3 alternated runs each after a warm-up.
                Run in alternated processes, parent and this tree; --label names the library.
  --part report --json FILE  -> the text of profiles/r17_delta_join.txt from the JSON lines of the runs above.
The ratio delta / full is printed twice — of the wall clocks and of the device-stage sums — beside the pair-test ratio 2m / n it
is expected to track (m x n tests against n x n / 2)."""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from components_probe import traced  # noqa: E402

STAGES = r"(gather|records|scans|filter) ([0-9.]+) ms"


def stage_ms(lines, what):
    for ln in reversed(lines):
        if what in ln:
            return {k: float(v) for k, v in re.findall(STAGES, ln)}
    return {}


def part_run(args):
    import torch

    torch.cuda.init()
    import smafa_amd
    from smafa_amd import _lib, synth

    lib = _lib.lib()
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    cases = [(int(m), False) for m in args.new.split(",")] + [(args.sorted_rows, True)]
    # related: synth.related_subjects(families, 100, div 0..0.08) at bound 5, where pairs dominate and the filter stage has work
    for name, alphabet, D in (("aa", 1, 5), ("nt", 0, 3), ("related", 1, 5)):
        if name not in args.stores.split(","):
            continue
        if name == "related":
            codes = synth.related_subjects(args.families, 100, div_lo=0.0, div_hi=0.08)
        else:
            codes = synth.subjects(args.rows, 60, alphabet)
        n = len(codes)
        for m, in_order in cases:
            if m <= 0 or m > n:
                continue
            new = codes[n - m:]
            if in_order:
                new = new[np.lexsort(new.T[::-1])]
            store = smafa_amd.SubjectStore(60, alphabet)
            store.push(codes[:n - m])
            store.push(new)
            n0 = n - m

            def delta():
                store.self_since_launch(n0, D, 0, 0, d_count.data_ptr())
                store.sync()

            def full():
                store.self_launch(D, 0, 0, d_count.data_ptr())
                store.sync()

            calls, what = {"delta": delta, "full": full}, {"delta": "delta self-join of", "full": "self-join of"}
            rec = {"part": "run", "store": name, "build": smafa_amd.build_id(), "rows": n, "new": m, "sorted_append": in_order, "bound": D}
            for indexed in (False, True):
                if indexed:
                    info = store.build_index(D)
                    store.set_index(1)
                    rec["index_serves"] = info["max_div_served"]
                else:
                    store.set_index(0)
                counts = {}
                for k, fn in calls.items():  # warm-up (and the re-sort, once)
                    fn()
                    counts[k] = int(d_count.item())
                if not indexed and m == cases[0][0]:
                    store.self_since_launch(0, D, 0, 0, d_count.data_ptr())
                    store.sync()
                    assert int(d_count.item()) == counts["full"], (int(d_count.item()), counts)
                wall, stages = {k: [] for k in calls}, {k: [] for k in calls}
                for _ in range(3):
                    for k, fn in calls.items():
                        t0 = time.perf_counter()
                        fn()
                        wall[k].append((time.perf_counter() - t0) * 1e3)
                        assert int(d_count.item()) == counts[k]  # (read back outside the timed region)
                for _ in range(3):
                    for k, fn in calls.items():
                        _, lines = traced(lib, fn)
                        stages[k].append(stage_ms(lines, what[k]))
                        assert int(d_count.item()) == counts[k]
                        kernels = store.last_call_kernels()
                        rec.setdefault("probed" if indexed else "scanned", {})[k] = any("index_probe" in x for x in kernels)
                key = "indexed" if indexed else "scan kernels"
                rec[key] = {"wall_ms": wall, "stages": stages, "pairs": counts, "scans": store.last_call_stats()["scans"]}
            store.close()
            with open(args.json, "a") as f:
                f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec), flush=True)


def part_old(args):
    import ctypes as C

    import torch

    torch.cuda.init()
    from smafa_amd import synth

    path = os.environ.get("SMAFA_AMD_LIB") or os.path.join(ROOT, "smafa_amd", "lib", "libsmafa_amd.so")
    lib = C.CDLL(path)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.smafa_build_id.restype = C.c_char_p
    lib.smafa_last_error.restype = C.c_char_p
    lib.smafa_db_destroy.restype = None
    lib.smafa_db_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, u32]
    lib.smafa_db_append.argtypes = [vp, vp, u64]
    lib.smafa_set_index.argtypes = [vp, C.c_int]
    lib.smafa_sync.argtypes = [vp]
    lib.smafa_db_destroy.argtypes = [vp]
    lib.smafa_db_self_launch.argtypes = [vp, u32, vp, u64, vp]
    lib.smafa_db_self_components_launch.argtypes = [vp, u32, vp, vp]
    lib.smafa_db_self_levels_launch.argtypes = [vp, u32, vp, vp]
    lib.smafa_db_self_density_launch.argtypes = [vp, u32, u32, vp, vp, vp]
    lib.smafa_db_self_peaks_launch.argtypes = [vp, u32, u32, vp, vp, vp, vp]
    lib.smafa_db_self_neighbours_launch.argtypes = [vp, u32, u32, vp, vp, vp, u64, vp]

    def ok(rc):
        if rc:
            raise SystemExit("delta_probe: %s" % lib.smafa_last_error().decode())

    for name, alphabet, D in (("aa", 1, 5), ("nt", 0, 3)):
        if name not in args.stores.split(","):
            continue
        codes = synth.subjects(args.rows, 60, alphabet)
        n = len(codes)
        h = vp()
        ok(lib.smafa_db_create(C.byref(h), 0, alphabet, 60))
        ok(lib.smafa_db_append(h, codes.ctypes.data, n))  # ONE append
        ok(lib.smafa_set_index(h, 0))
        cap = 1 << 22
        d_labels = torch.zeros((D + 1) * n, dtype=torch.int32, device="cuda")
        d_a, d_b = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
        d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_nb, d_ds = (torch.zeros(cap, dtype=torch.int32, device="cuda") for _ in range(2))
        d_counts = torch.zeros(D + 3, dtype=torch.int64, device="cuda")
        L, A, B, N = d_labels.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), d_counts.data_ptr()
        calls = {"pairs": lambda: lib.smafa_db_self_launch(h, D, None, 0, N),
                 "components": lambda: lib.smafa_db_self_components_launch(h, D, L, N),
                 "levels": lambda: lib.smafa_db_self_levels_launch(h, D, L, N),
                 "density": lambda: lib.smafa_db_self_density_launch(h, D, 20, L, A, N),
                 "peaks": lambda: lib.smafa_db_self_peaks_launch(h, D, 0, L, A, B, N),
                 "neighbours": lambda: lib.smafa_db_self_neighbours_launch(h, D, 0xffffffff, d_offsets.data_ptr(), d_nb.data_ptr(),
                                                                          d_ds.data_ptr(), cap, N)}

        def run(fn):
            ok(fn())
            ok(lib.smafa_sync(h))

        for fn in calls.values():
            run(fn)  # warm-up
        wall = {k: [] for k in calls}
        for _ in range(3):
            for k, fn in calls.items():
                t0 = time.perf_counter()
                run(fn)
                wall[k].append((time.perf_counter() - t0) * 1e3)
        lib.smafa_db_destroy(h)
        rec = {"part": "old", "label": args.label, "store": name, "build": lib.smafa_build_id().decode(), "rows": n, "bound": D,
               "wall_ms": wall}
        with open(args.json, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)


def med(xs):
    xs = [x for x in xs if x is not None]
    return statistics.median(xs) if xs else float("nan")


def part_report(args):
    recs = [json.loads(ln) for ln in open(args.json) if ln.strip()]
    print("delta self-join beside the full join (tools/delta_probe.py --part run; count-only launch forms, medians of 3 alternated runs in one "
          "process; wall = launch + sync and nothing else; stages from 3 further runs under the level-2 trace)")
    for r in recs:
        if r.get("part") != "run":
            continue
        print("\n%s: %d rows, %d new (%s), bound %d, build %s; expected ratio 2m/n = %.4f" % (
            r["store"], r["rows"], r["new"], "appended sorted" if r["sorted_append"] else "append order", r["bound"], r["build"],
            2.0 * r["new"] / r["rows"]))
        for key in ("scan kernels", "indexed"):
            if key not in r:
                continue
            x = r[key]
            g = lambda k, s: med([y.get(s) for y in x["stages"][k]])  # noqa: E731
            d, f = med(x["wall_ms"]["delta"]), med(x["wall_ms"]["full"])
            dd = g("delta", "gather") + g("delta", "scans") + g("delta", "filter")
            fd = g("full", "records") + g("full", "scans") + g("full", "filter")
            print("  %-12s delta: wall %.3f ms, device %.3f ms (gather %.3f, scans %.3f, filter %.3f), %d pairs | full: wall %.2f ms, device "
                  "%.2f ms (records %.3f, scans %.3f, filter %.3f), %d pairs | delta / full: wall %.4f, device %.4f" % (
                      key, d, dd, g("delta", "gather"), g("delta", "scans"), g("delta", "filter"), x["pairs"]["delta"], f, fd,
                      g("full", "records"), g("full", "scans"), g("full", "filter"), x["pairs"]["full"], d / f, dd / fd))
    olds = [r for r in recs if r.get("part") == "old"]
    if olds:
        print("\nthe six older calls, launch forms, on the ONE-APPEND bench stores (--part old; alternated processes, 3 alternated runs "
              "each after a warm-up; median over all runs of a library, and the per-process medians)")
        labels = sorted({r["label"] for r in olds})
        for store in sorted({r["store"] for r in olds}):
            for call in olds[0]["wall_ms"]:
                row = {}
                for lab in labels:
                    mine = [r for r in olds if r["label"] == lab and r["store"] == store]
                    row[lab] = (med([x for r in mine for x in r["wall_ms"][call]]), [med(r["wall_ms"][call]) for r in mine],
                                mine[0]["build"] if mine else "?")
                text = "; ".join("%s (%s) %.2f ms [%s]" % (lab, v[2], v[0], ", ".join("%.2f" % x for x in v[1])) for lab, v in row.items())
                ratio = " | this / parent = %.4f" % (row["this"][0] / row["parent"][0]) if "this" in row and "parent" in row else ""
                print("  %s %-10s %s%s" % (store, call, text, ratio))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["run", "old", "report"], required=True)
    ap.add_argument("--json", default="delta_probe.jsonl")
    ap.add_argument("--stores", default="aa,nt")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--families", type=int, default=10_000)
    ap.add_argument("--new", default="10000,100000,1000000")
    ap.add_argument("--sorted-rows", type=int, default=100_000)
    ap.add_argument("--label", default="this")
    args = ap.parse_args()
    {"run": part_run, "old": part_old, "report": part_report}[args.part](args)


if __name__ == "__main__":
    main()
