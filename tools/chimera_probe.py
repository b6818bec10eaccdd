"""Timing of the chimera check (smafa_db_self_chimeras_launch) beside the peaks call (smafa_db_self_peaks_launch) on the same
store and bound — profiles/r24_chimeras.txt.

One process, this tree's library, both calls in their _launch form on torch device buffers.  Per store: a warm-up of each call,
then `--rounds` alternated rounds (peaks, chimeras, peaks, ...), wall clock around launch + smafa_sync, the device time of
smafa_last_call_stats and the per-stage milliseconds of the library's level-2 trace line; medians are reported.  The join is
the same in the two calls (same bound, same radius 0, same weigh/keep kernel), so the difference is init_sides + offer_sides +
verdict against init + climb + settle + jump.
Stores: (a) the bench's 10M x 60 stores (amino acids at bound 5, nucleotides at bound 3; smafa_amd.synth.subjects), where pairs
are rare and the scans are everything; (p) planted families with heavy seeds — `--families` random seeds of 60 columns, each with
`--heavy` exact copies and `--light` single rows 1 - 3 substitutions from it, at bound 3: every light row has `--heavy` eligible
parents and its own family's light rows as ineligible pairs, so the gather of phase 2 runs for most kept pairs."""
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

STAGES = r"(records|scans|weigh/keep|climb|settle\+jump|offers|verdict) ([0-9.]+) ms"


def stage_ms(lines, what):
    for ln in reversed(lines):
        if what in ln:
            d = {k: float(v) for k, v in re.findall(STAGES, ln)}
            m = re.search(r"in (\d) join", ln)
            if m:
                d["joins"] = int(m.group(1))
            m = re.search(r"(\d+) pairs kept", ln)
            if m:
                d["pairs_kept"] = int(m.group(1))
            return d
    return {}


def heavy_families(families, heavy, light, seed=7, L=60):
    rng = np.random.default_rng(seed)
    seeds = rng.integers(0, 4, size=(families, L)).astype(np.uint8)
    members = np.repeat(seeds, light, axis=0)
    subs = rng.integers(1, 4, size=len(members))
    cols = np.argsort(rng.random(size=(len(members), L)), axis=1)[:, :3]
    for s in range(3):
        who = np.nonzero(subs > s)[0]
        members[who, cols[who, s]] = (members[who, cols[who, s]] + rng.integers(1, 4, size=len(who))) % 4
    codes = np.concatenate([np.repeat(seeds, heavy, axis=0), members])
    rng.shuffle(codes, axis=0)
    return np.ascontiguousarray(codes)


def stores(args):
    from smafa_amd import synth

    if "a" in args.stores:
        yield "(a) aa: synth.subjects", synth.subjects(args.rows, 60, 1), 1, 5
        yield "(a) nt: synth.subjects", synth.subjects(args.rows, 60, 0), 0, 3
    if "p" in args.stores:
        yield ("(p) planted families: %d seeds x (%d copies + %d rows 1 - 3 columns away)" % (args.families, args.heavy, args.light),
               heavy_families(args.families, args.heavy, args.light), 0, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stores", default="ap")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--families", type=int, default=20_000)
    ap.add_argument("--heavy", type=int, default=30)
    ap.add_argument("--light", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fold", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_chimeras.txt"))
    args = ap.parse_args()
    import torch

    torch.cuda.init()
    import smafa_amd
    from smafa_amd import _lib

    lib = _lib.lib()
    med = statistics.median
    out = ["chimera probe — one MI355X, build id %s" % smafa_amd.build_id(),
           "both calls in their _launch form, one process; wall clock around launch + sync, device ms from smafa_last_call_stats, "
           "per-stage ms from the level-2 trace; medians of %d alternated rounds after a warm-up" % args.rounds, ""]
    for name, codes, alphabet, D in stores(args):
        n = len(codes)
        store = smafa_amd.SubjectStore(codes.shape[1], alphabet)
        store.push(codes)
        store.set_index(0)
        bufs = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(6)]
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def peaks():
            store.self_peaks_launch(D, 0, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), count.data_ptr())
            store.sync()

        def chimeras():
            store.self_chimeras_launch(D, 0, args.fold, 0, *(b.data_ptr() for b in bufs), count.data_ptr())
            store.sync()

        calls = {"peaks": (peaks, "peaks of"), "chimeras": (chimeras, "chimeras of")}
        for fn, _ in calls.values():
            fn()  # warm-up
        wall, device, stages = ({k: [] for k in calls} for _ in range(3))
        for _ in range(args.rounds):
            for k, (fn, what) in calls.items():
                t0 = time.perf_counter()
                _, lines = traced(lib, fn)
                wall[k].append((time.perf_counter() - t0) * 1e3)
                device[k].append(store.last_call_stats()["kernel_ms"])
                stages[k].append(stage_ms(lines, what))
        flagged = int(count.item())
        with_parent = int((bufs[1] != -1).sum().item())
        rec = {"store": name, "rows": n, "bound": D, "fold": args.fold, "flagged": flagged, "rows_with_a_parent": with_parent,
               "wall_ms": wall, "device_ms": device, "stages": stages}
        print(json.dumps(rec))
        out.append("%s: n = %d, bound %d, radius 0, fold %d: %d pairs kept, %d rows with a parent, %d flagged" % (
            name, n, D, args.fold, stages["chimeras"][0].get("pairs_kept", -1), with_parent, flagged))
        st = {}
        for k in calls:
            keys = [s for s in ("records", "scans", "weigh/keep", "climb", "settle+jump", "offers", "verdict") if s in stages[k][0]]
            st[k] = {s: med([x[s] for x in stages[k]]) for s in keys}
            out.append("  %-9s wall %9.2f ms (rounds %s); device %9.2f ms; joins %s; %s" % (
                k, med(wall[k]), ", ".join("%.2f" % x for x in wall[k]), med(device[k]), stages[k][0].get("joins"),
                ", ".join("%s %.3f ms" % kv for kv in st[k].items())))
        own = {"peaks": st["peaks"].get("climb", 0.0) + st["peaks"].get("settle+jump", 0.0),
               "chimeras": st["chimeras"].get("offers", 0.0) + st["chimeras"].get("verdict", 0.0)}
        out.append("  behind the join: offers + verdict %.3f ms against climb + settle + jump %.3f ms; wall chimeras / peaks = %.3f" % (
            own["chimeras"], own["peaks"], med(wall["chimeras"]) / med(wall["peaks"])))
        out.append("")
        store.close()
        del bufs
        torch.cuda.empty_cache()
    text = "\n".join(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
