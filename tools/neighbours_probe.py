"""Timing of the neighbour lists (smafa_db_self_neighbours) beside the components call and beside the route a caller had before —
profiles/r15_neighbours.txt.

  --part run    one process, this tree's library.  Per store: the components call and the neighbours call (no cut) at the bound,
                alternated, 3 runs each after a warm-up, wall clock around the host-form call; the library's per-stage
                milliseconds, the entries and the growths come from its level-2 trace line.  Then the OLD ROUTE, 3 runs: self_pairs
                to the host, every edge mirrored, np.lexsort by (row, dist, neighbour), np.searchsorted for the row offsets — its
                result must equal the call's bytes — and the bytes each route moves over PCIe.
                Stores: (a) the bench's 10M x 60 stores (amino acids at bound 5, nucleotides at bound 3; smafa_amd.synth.subjects);
                (b) synth.related_subjects(families, 100, div 0..0.08) at bound 5; (c) the dense 4 000-row store of the tests at
                bound 3.
  The parent commit's library has no neighbours call; its components, levels and density calls are timed against this tree's
  with tools/peaks_probe.py --part old, which runs any library through ctypes, in alternated processes.
  --part report --json FILE  -> the text of profiles/r15_neighbours.txt from the JSON lines of the runs above."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from components_probe import traced  # noqa: E402
from peaks_probe import stores  # noqa: E402

STAGES = r"(records|scans|pack|sort|bounds|emit|link|flatten) ([0-9.]+) ms"


def stage_ms(lines, what):
    for ln in reversed(lines):
        if what in ln:
            d = {k: float(v) for k, v in re.findall(STAGES, ln)}
            for k, pat in (("entries", r"(\d+) entries"), ("growths", r"(\d+) growths"), ("sorts", r"\((\d) sorts?\)")):
                m = re.search(pat, ln)
                if m:
                    d[k] = int(m.group(1))
            return d
    return {}


def old_route(store, n, D):
    """-> (offsets, neighbours, dists, ms of the host part alone, bytes over PCIe)"""
    pairs = store.self_pairs(D, first_cap=1 << 24)
    t0 = time.perf_counter()
    row = np.concatenate([pairs["query"], pairs["subject"]])
    nb = np.concatenate([pairs["subject"], pairs["query"]])
    ds = np.concatenate([pairs["dist"], pairs["dist"]])
    order = np.lexsort((nb, ds, row))
    row, nb, ds = row[order], nb[order], ds[order]
    offsets = np.searchsorted(row, np.arange(n + 1, dtype=np.uint32), side="left").astype(np.uint64)
    return offsets, nb, ds, (time.perf_counter() - t0) * 1e3, pairs.nbytes


def part_run(args):
    import smafa_amd
    from smafa_amd import _lib

    lib = _lib.lib()
    for name, codes, alphabet, D in stores(args):
        n = len(codes)
        store = smafa_amd.SubjectStore(codes.shape[1], alphabet)
        store.push(codes)
        store.set_index(0)
        calls = {"components": lambda: store.self_components(D), "neighbours": lambda: store.self_neighbours(D, first_cap=args.cap)}
        what = {"components": "components of", "neighbours": "neighbours of"}
        for fn in calls.values():
            fn()  # warm-up
        wall, stages = {k: [] for k in calls}, {k: [] for k in calls}
        for _ in range(3):
            for k, fn in calls.items():
                t0 = time.perf_counter()
                res, lines = traced(lib, fn)
                wall[k].append((time.perf_counter() - t0) * 1e3)
                stages[k].append(stage_ms(lines, what[k]))
        offsets, nb, ds = store.self_neighbours(D, first_cap=args.cap)
        old_wall, old_host, old_bytes = [], [], 0
        for _ in range(3):
            t0 = time.perf_counter()
            o_offsets, o_nb, o_ds, host_ms, old_bytes = old_route(store, n, D)
            old_wall.append((time.perf_counter() - t0) * 1e3)
            old_host.append(host_ms)
        assert o_offsets.tobytes() == offsets.tobytes() and o_nb.tobytes() == nb.tobytes() and o_ds.tobytes() == ds.tobytes()
        rec = {"part": "run", "store": name, "build": smafa_amd.build_id(), "rows": n, "bound": D, "entries": int(len(nb)),
               "wall_ms": wall, "stages": stages, "old_route_wall_ms": old_wall, "old_route_host_ms": old_host,
               "pcie_bytes": {"neighbours": int(offsets.nbytes + nb.nbytes + ds.nbytes), "old route": int(old_bytes)}}
        store.close()
        with open(args.json, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec))


def med(xs):
    return statistics.median(xs) if xs else float("nan")


def part_report(args):
    recs = [json.loads(ln) for ln in open(args.json) if ln.strip()]
    print("neighbour lists beside the components call (tools/neighbours_probe.py; medians of 3, calls alternated in one process)")
    for r in recs:
        if r.get("part") != "run":
            continue
        nbs, cc = r["stages"]["neighbours"], r["stages"]["components"]
        g = lambda rows, k: med([x[k] for x in rows if k in x])  # noqa: E731
        print("\n%s: %d rows, bound %d, %d entries, build %s" % (r["store"], r["rows"], r["bound"], r["entries"], r["build"]))
        print("  components: wall %.1f ms, scans %.2f ms" % (med(r["wall_ms"]["components"]), g(cc, "scans")))
        print("  neighbours: wall %.1f ms, scans %.2f ms (x %.3f of the components call's), pack %.2f, sort %.2f (%d sort%s), bounds %.2f, "
              "emit %.2f ms, %d growths in the last run" % (med(r["wall_ms"]["neighbours"]), g(nbs, "scans"), g(nbs, "scans") / g(cc, "scans"),
                                                         g(nbs, "pack"), g(nbs, "sort"), nbs[-1].get("sorts", 0),
                                                         "" if nbs[-1].get("sorts", 0) == 1 else "s", g(nbs, "bounds"), g(nbs, "emit"),
                                                         nbs[-1].get("growths", 0)))
        print("  old route (self_pairs, mirror, lexsort, searchsorted): wall %.1f ms, of it on the host %.1f ms" % (
            med(r["old_route_wall_ms"]), med(r["old_route_host_ms"])))
        print("  over PCIe: neighbours %d B, old route %d B" % (r["pcie_bytes"]["neighbours"], r["pcie_bytes"]["old route"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["run", "report"], required=True)
    ap.add_argument("--json", default="neighbours_probe.jsonl")
    ap.add_argument("--stores", default="abc")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--families", type=int, default=10_000)
    ap.add_argument("--min-pts", type=int, default=20)
    ap.add_argument("--cap", type=int, default=1 << 25)
    args = ap.parse_args()
    {"run": part_run, "report": part_report}[args.part](args)


if __name__ == "__main__":
    main()
