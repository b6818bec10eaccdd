#!/usr/bin/env python3
"""The k-nearest path (kth_plan.h, scan_host.hip.h) seen from outside: what each host-buffer call launches, finds and costs on
the bench's stores (10M x 60 aa, seed 1; 10M x 60 nt, seed 2), 10 000 planted queries.  Per store and call: the call's kernel
list, its launches and scans (smafa_last_call_stats), a hash of its rows, and the wall-clock median of --reps calls after a
warm-up.  One JSON line per process:
  k1 / k5 / k50   smafa_scan_hits without a bound (the ladder, the planner, the loose path)
  k5_d12          k = 5 under bound 12
  k1_64           64 queries, k = 1 (no ladder probe, no index)
  index3          a fresh handle in index mode 3, k = 1 without a bound, called until the index is bought (at most 8 calls):
                  per call the kernel list, launches, scans, row hash and blocks of the index; not timed
Run in alternated processes, SMAFA_AMD_LIB naming the parent commit's library or none for this tree's; --label says which.
    python3 tools/kth_plan_probe.py --label this|parent            one process
    python3 tools/kth_plan_probe.py --report lines.jsonl           the table of profiles/r18_kth_plan.txt"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS = ("k1", "k5", "k50", "k5_d12", "k1_64")
CAP = 1 << 22  # rows: 10 000 queries x (50 + ties)


def report(path):
    recs = [json.loads(ln) for ln in open(path) if ln.startswith("{")]
    print("this tree (build %s) against the parent commit's library (build %s), alternated processes; ms per call, each process's"
          % tuple(next(r["build"] for r in recs if r["label"] == lb) for lb in ("this", "parent")))
    print("median of %d; condition: the tree's median within the parent's min..max widened on both sides by that width" % recs[0]["reps"])
    for store in ("aa", "nt"):
        for call in CALLS:
            par = [r[store]["ms"][call] for r in recs if r["label"] == "parent"]
            new = [r[store]["ms"][call] for r in recs if r["label"] == "this"]
            lo, hi, med = min(par), max(par), statistics.median(new)
            ok = lo - (hi - lo) <= med <= hi + (hi - lo)
            print("  %s %-7s parent %s (median %.3f)  this %s (median %.3f)  ratio %.3f  allowed %.3f..%.3f  %s" % (
                store, call, " ".join("%.3f" % v for v in par), statistics.median(par), " ".join("%.3f" % v for v in new), med,
                med / statistics.median(par), lo - (hi - lo), hi + (hi - lo), "within" if ok else "OUTSIDE"))
    first = {lb: next(r for r in recs if r["label"] == lb) for lb in ("this", "parent")}
    for store in ("aa", "nt"):
        same = all(r[store]["seen"] == first["parent"][store]["seen"] for r in recs)
        print("  %s: kernel lists, launches, scans, row hashes and the index calls equal in every process of both sides: %s" % (store, same))
        for call, seen in first["this"][store]["seen"].items():
            print("    %-7s %s" % (call, json.dumps(seen)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this")
    ap.add_argument("--report", default=None)
    ap.add_argument("--db-rows", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    if a.report:
        return report(a.report)
    import numpy as np

    import smafa_amd
    from smafa_amd import _lib, synth

    out_rows = np.zeros(CAP, dtype=smafa_amd.HIT_DTYPE)

    def call(store, q, D, k):
        """one smafa_scan_hits with room for every row -> what the call was seen to do"""
        n_out = C.c_uint64(0)
        rc = _lib.lib().smafa_scan_hits(store._h, q.ctypes.data, len(q), _lib.NONE if D is None else D, k, out_rows.ctypes.data, CAP, C.byref(n_out))
        assert rc == 0, (rc, _lib.lib().smafa_last_error())
        return int(n_out.value)

    def seen(store, n):
        st = store.last_call_stats()
        return {"kernels": store.last_call_kernels(), "launches": st["launches"], "scans": st["scans"], "rows": n,
                "sha1": hashlib.sha1(out_rows[:n].tobytes()).hexdigest()}

    out = {"label": a.label, "build": smafa_amd.build_id(), "reps": a.reps, "db_rows": a.db_rows}
    for name, alphabet in (("aa", 1), ("nt", 0)):
        subj = synth.subjects(a.db_rows, 60, alphabet, seed=1 if alphabet else 2)
        q, _, _ = synth.queries(subj, a.queries, alphabet, seed=3, max_subs=10 if alphabet else 6)
        q = np.ascontiguousarray(q, dtype=np.uint8)
        store = smafa_amd.SubjectStore(60, alphabet, 0)
        store.push(subj)
        ms, what = {}, {}
        for label, qq, D, k in (("k1", q, None, 1), ("k5", q, None, 5), ("k50", q, None, 50), ("k5_d12", q, 12, 5), ("k1_64", q[:64], None, 1)):
            what[label] = seen(store, call(store, qq, D, k))  # (the warm-up)
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                call(store, qq, D, k)
                t.append((time.perf_counter() - t0) * 1e3)
            ms[label] = statistics.median(t)
        store.close()
        store = smafa_amd.SubjectStore(60, alphabet, 0)
        store.push(subj)
        store.set_index(3)
        calls = []
        for _ in range(8):
            s = seen(store, call(store, q, None, 1))
            s["blocks"] = store.index_info().get("blocks")
            calls.append(s)
            if s["blocks"]:
                break
        what["index3"] = calls
        store.close()
        out[name] = {"ms": ms, "seen": what}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
