#!/usr/bin/env python3
"""Host cost of choosing a scan launch's kernel (scan_plan.h), seen from outside: wall clock around call + synchronise on the
bench's headline store (10M x 60 aa, bound 5), medians of --reps runs after a warm-up, one JSON line per process:
  launch     one smafa_scan_launch of 10 000 planted queries (the headline launch)
  each_200   smafa_scan_each, 200 one-query passes enqueued by one call, no graph: 200 plans per call
  each_graph one one-query smafa_scan_each replayed from its captured graph
  hits_64    smafa_scan_hits of 64 queries through the host-buffer API
Run in alternated processes, SMAFA_AMD_LIB naming the parent commit's library or none for this tree's; --label says which.
    python3 tools/scan_plan_probe.py --label this|parent            one process
    python3 tools/scan_plan_probe.py --report lines.jsonl           the table of profiles/r16_scan_plan.txt"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def report(path):
    recs = [json.loads(ln) for ln in open(path) if ln.startswith("{")]
    print("this tree (build %s) against the parent commit's library (build %s), alternated processes; ms per call, each process's"
          % tuple(next(r["build"] for r in recs if r["label"] == lb) for lb in ("this", "parent")))
    print("median of %d; condition: the tree's median within the parent's min..max widened on both sides by that width" % recs[0]["reps"])
    for line in ("launch", "each_200", "each_graph", "hits_64"):
        par = [r[line] for r in recs if r["label"] == "parent"]
        new = [r[line] for r in recs if r["label"] == "this"]
        lo, hi, med = min(par), max(par), statistics.median(new)
        ok = lo - (hi - lo) <= med <= hi + (hi - lo)
        print("  %-10s parent %s (median %.4f)  this %s (median %.4f)  ratio %.3f  allowed %.4f..%.4f  %s" % (
            line, " ".join("%.4f" % v for v in par), statistics.median(par), " ".join("%.4f" % v for v in new), med,
            med / statistics.median(par), lo - (hi - lo), hi + (hi - lo), "within" if ok else "OUTSIDE"))
    kern = {r["label"]: r["kernels"] for r in recs}
    print("  kernels launched, this == parent: %s  %s" % (kern["this"] == kern["parent"], kern["this"]))
    rows = {r["label"]: r["rows"] for r in recs}
    print("  rows found, this == parent: %s  %s" % (rows["this"] == rows["parent"], rows["this"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this")
    ap.add_argument("--report", default=None)
    ap.add_argument("--db-rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    if a.report:
        return report(a.report)
    import torch

    import smafa_amd
    from smafa_amd import synth

    subj = synth.subjects(a.db_rows, 60, 1, seed=1)
    q, _, _ = synth.queries(subj, 10_000, 1, seed=3, max_subs=5)
    dev = torch.device("cuda", 0)
    store = smafa_amd.SubjectStore(60, 1, 0)
    store.push(subj)
    cap = 1 << 20
    hits = torch.zeros(cap * 3, dtype=torch.int32, device=dev)
    counts = torch.zeros(256, dtype=torch.int64, device=dev)
    big, many, one = smafa_amd.QuerySet(store, q), smafa_amd.QuerySet(store, q[:200]), smafa_amd.QuerySet(store, q[:1])
    kernels, rows = {}, {}

    def timed(name, fn, result):
        fn()  # warm-up (and, for the graph form, the capture)
        store.sync()
        kernels[name] = store.last_call_kernels()
        rows[name] = result()
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            store.sync()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms)

    out = {"label": a.label, "build": smafa_amd.build_id(), "reps": a.reps, "db_rows": a.db_rows}
    out["launch"] = timed("launch", lambda: store.scan_launch(big, 5, None, hits.data_ptr(), cap, counts.data_ptr()), lambda: int(counts[0]))
    out["each_200"] = timed("each_200", lambda: store.scan_each(many, 5, hits.data_ptr(), 256, counts.data_ptr(), False),
                            lambda: int(counts[:200].sum()))
    out["each_graph"] = timed("each_graph", lambda: store.scan_each(one, 5, hits.data_ptr(), 256, counts.data_ptr(), True), lambda: int(counts[0]))
    got = []
    out["hits_64"] = timed("hits_64", lambda: got.append(len(store.scan(q[:64], max_divergence=5))), lambda: got[-1])
    out["kernels"], out["rows"] = kernels, rows
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
