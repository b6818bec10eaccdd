"""Timing of the density clusters (smafa_db_self_density) beside the components call — profiles/r11_density.txt.

One process, this tree's library.  Per store: the components call at the bound, the density call with every pair kept (one
join) and the density call of a handle made with SMAFA_DENSITY_KEEP_MAX=0 (two joins), alternated, 3 runs each after a
warm-up, wall clock around the host-form call; the library's per-stage milliseconds come from its level-2 trace line.
Stores: (a) the bench's 10M x 60 stores (amino acids at bound 5, nucleotides at bound 3; smafa_amd.synth.subjects), where
pairs are rare and the scans are everything; (b) synth.related_subjects(families, 100, div 0..0.08) at bound 5, where pairs
dominate; (c) the dense 4 000-row store of the tests at bound 3.  The three answers of a store are compared on the way.
  --part run --json FILE     one JSON line per store appended to FILE
  --part report --json FILE  -> the text of profiles/r11_density.txt"""
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

STAGES = r"(records|scans|count/keep|link|flatten) ([0-9.]+) ms"


def stage_ms(lines, what):
    for ln in reversed(lines):
        if what in ln:
            d = {k: float(v) for k, v in re.findall(STAGES, ln)}
            m = re.search(r"in (\d) join", ln)
            if m:
                d["joins"] = int(m.group(1))
            return d
    return {}


def measure(name, codes, alphabet, D, min_pts, out):
    import smafa_amd
    from smafa_amd import _lib

    lib = _lib.lib()
    os.environ.pop("SMAFA_DENSITY_KEEP_MAX", None)
    one = smafa_amd.SubjectStore(codes.shape[1], alphabet)
    os.environ["SMAFA_DENSITY_KEEP_MAX"] = "0"  # (read when the handle is made)
    two = smafa_amd.SubjectStore(codes.shape[1], alphabet)
    os.environ.pop("SMAFA_DENSITY_KEEP_MAX")
    for s in (one, two):
        s.push(codes)
        s.set_index(0)
    calls = {"components": lambda: one.self_components(D), "density, one join": lambda: one.self_density(D, min_pts),
             "density, two joins": lambda: two.self_density(D, min_pts)}
    what = {"components": "components of", "density, one join": "density of", "density, two joins": "density of"}
    for fn in calls.values():
        fn()  # warm-up
    wall, stages = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(3):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            res, lines = traced(lib, fn)
            wall[k].append((time.perf_counter() - t0) * 1e3)
            stages[k].append(stage_ms(lines, what[k]))
    a, b = one.self_density(D, min_pts), two.self_density(D, min_pts)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    row, count = one.self_components(D)
    base = one.self_density(D, 1)
    assert base[0].tobytes() == row.tobytes() and base[2]["clusters"] == count
    rec = {"store": name, "build": smafa_amd.build_id(), "rows": len(codes), "bound": D, "min_pts": min_pts,
           "pairs": int(a[1].astype(np.int64).sum()) // 2, "components": count, "counts": a[2], "wall_ms": wall, "stages": stages}
    one.close()
    two.close()
    with open(out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


def part_run(args):
    from smafa_amd import synth
    from components_cases import dense_store

    if "a" in args.stores:
        measure("(a) aa: synth.subjects", synth.subjects(args.rows, 60, 1), 1, 5, args.min_pts, args.json)
        measure("(a) nt: synth.subjects", synth.subjects(args.rows, 60, 0), 0, 3, args.min_pts, args.json)
    if "b" in args.stores:
        measure("(b) related_subjects, families of 100, divergence 0..0.08",
                synth.related_subjects(args.families, 100, div_lo=0.0, div_hi=0.08), 1, 5, args.min_pts, args.json)
    if "c" in args.stores:
        measure("(c) dense store: 2 000 + 2 000 copies at distance 3", dense_store()[0], 0, 3, args.min_pts, args.json)


def part_report(args):
    with open(args.json) as f:
        recs = [json.loads(ln) for ln in f if ln.strip()]
    med = statistics.median
    out = ["density probe — one MI355X, build id %s" % (recs[0]["build"] if recs else "?"),
           "wall clock around the host-form call, medians of 3 alternated runs after a warm-up; per-stage ms from the level-2 trace", ""]
    for r in recs:
        out.append("%s: n = %d, bound %d, min_pts %d: %d pairs, %d components; density %s" % (
            r["store"], r["rows"], r["bound"], r["min_pts"], r["pairs"], r["components"], r["counts"]))
        base = None
        for k in ("components", "density, one join", "density, two joins"):
            keys = [s for s in ("records", "scans", "count/keep", "link", "flatten") if s in r["stages"][k][0]]
            st = {s: med([x[s] for x in r["stages"][k]]) for s in keys}
            base = base or st
            line = "  %-20s wall %9.1f ms (runs %s); %s" % (k, med(r["wall_ms"][k]), ", ".join("%.1f" % x for x in r["wall_ms"][k]),
                                                          ", ".join("%s %.3f ms" % kv for kv in st.items()))
            if k != "components":
                line += "; joins %s; scans / components' scans = %.3f" % (r["stages"][k][0].get("joins"), st["scans"] / base["scans"])
                if st.get("count/keep"):
                    line += "; count/keep %.2f G pairs/s" % (r["pairs"] / st["count/keep"] / 1e6)
                if st.get("link"):
                    line += "; link %.2f G pairs/s" % (r["pairs"] / st["link"] / 1e6)
            out.append(line)
        out.append("")
    text = "\n".join(out)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["run", "report"], required=True)
    ap.add_argument("--stores", default="abc")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--families", type=int, default=10_000)
    ap.add_argument("--min-pts", type=int, default=20)
    ap.add_argument("--json", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_density.txt"))
    args = ap.parse_args()
    {"run": part_run, "report": part_report}[args.part](args)


if __name__ == "__main__":
    main()
