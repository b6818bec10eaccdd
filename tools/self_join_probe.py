"""Timing of the self-join (smafa_db_self_launch) against the only route to the same pairs without it.

Per store (10M x 60 amino acids at bound 5, 10M x 60 nucleotides at bound 3; smafa_amd.synth.subjects, the bench's store):
  (a) self_launch on the scan kernels            (b) self_launch with a built block index
  (a1) as (a) with SMAFA_JOIN_STRIDE=1 — blocks of consecutive positions instead of interleaved ones — with the time of
       every block's scan from the library's trace lines: what the interleaving is for
  (c) the store's own code rows as resident query sets of 65 536, smafa_scan_launch over all tiles, rows left on the
      device: every pair twice plus n self-pairs — the old route in its kindest form (sets packed beforehand, no PCIe, no
      host de-duplication)
Host clock around launch + synchronise, medians of 3 alternated runs after one warm-up each; the row counts of the three
must agree.  One more run of (a) at debug verbosity gives the per-stage device times.  Writes --out (a text file)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch.cuda.init()

import smafa_amd  # noqa: E402
from smafa_amd import _lib, synth  # noqa: E402


def traced_join(store, D, d_hits, cap, d_count, level):
    """one self_launch with the library's stderr lines captured -> (wall ms, lines)"""
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        _lib.lib().smafa_set_verbosity(level)
        try:
            t0 = time.perf_counter()
            store.self_launch(D, d_hits.data_ptr(), cap, d_count.data_ptr())
            store.sync()
            ms = (time.perf_counter() - t0) * 1e3
        finally:
            _lib.lib().smafa_set_verbosity(0)
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return ms, [ln.strip() for ln in tmp.read().decode(errors="replace").splitlines() if "self-join" in ln]


def block_times(trace):
    out = []
    for ln in trace:
        if ", scan " in ln and ln.endswith(" ms"):
            out.append(float(ln.rsplit(", scan ", 1)[1][:-3]))
    return out


def describe(ts):
    if not ts:
        return "no trace"
    k = max(1, len(ts) // 10)
    return "%d scans: first tenth %.2f ms each, last tenth %.2f ms each, min %.2f, median %.2f, max %.2f" % (
        len(ts), sum(ts[:k]) / k, sum(ts[-k:]) / k, min(ts), statistics.median(ts), max(ts))


def probe(label, alphabet, n, D, lines, batch=65536):
    codes = synth.subjects(n, 60, alphabet)
    store = smafa_amd.SubjectStore(60, alphabet)
    store.push(codes)
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    store.self_launch(D, 0, 0, d_count.data_ptr())
    store.sync()
    total = int(d_count.item())
    cap = total + 1024
    d_hits = torch.zeros(cap * 3, dtype=torch.int32, device="cuda")

    def run_join():
        t0 = time.perf_counter()
        store.self_launch(D, d_hits.data_ptr(), cap, d_count.data_ptr())
        store.sync()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, int(d_count.item()), store.last_call_stats()["kernel_ms"]

    qsets = [smafa_amd.QuerySet(store, codes[lo:lo + batch]) for lo in range(0, n, batch)]
    d_counts = torch.zeros(len(qsets), dtype=torch.int64, device="cuda")
    old_cap = 2 * total + n + 1024  # room for every row of the old route, were they kept side by side
    d_old = torch.zeros(min(old_cap, 1 << 26) * 3, dtype=torch.int32, device="cuda")

    def run_old():
        t0 = time.perf_counter()
        for i, qs in enumerate(qsets):  # each set's rows overwrite the last set's: only the counts are compared
            store.scan_launch(qs, D, None, d_old.data_ptr(), d_old.numel() // 3, d_counts.data_ptr() + 8 * i)
        store.sync()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, int(d_counts.sum().item())

    store.set_index(0)
    run_join(), run_old()  # warm-up
    a, c = [], []
    for _ in range(3):
        a.append(run_join())
        c.append(run_old())
    assert all(x[1] == total for x in a)
    assert all((x[1] - n) % 2 == 0 and (x[1] - n) // 2 == total for x in c), (c, total, n)
    kernels_a = store.last_call_kernels()
    # per-stage device times and every block's scan time of one more run, from the library's debug lines
    _, trace = traced_join(store, D, d_hits, cap, d_count, 3)
    stages = [ln for ln in trace if "self-join of" in ln]
    blocks_a = describe(block_times(trace))
    # the same join over blocks of consecutive positions: a second handle on the same rows
    os.environ["SMAFA_JOIN_STRIDE"] = "1"
    try:
        plain = smafa_amd.SubjectStore(60, alphabet)
    finally:
        del os.environ["SMAFA_JOIN_STRIDE"]
    plain.push(codes)
    plain.set_index(0)
    a1 = []
    for rep in range(4):
        t0 = time.perf_counter()
        plain.self_launch(D, d_hits.data_ptr(), cap, d_count.data_ptr())
        plain.sync()
        if rep:
            a1.append(((time.perf_counter() - t0) * 1e3, int(d_count.item())))
    assert all(x[1] == total for x in a1)
    _, trace1 = traced_join(plain, D, d_hits, cap, d_count, 3)
    blocks_a1 = describe(block_times(trace1))
    plain.close()
    store.set_index(1)
    info = store.build_index(D)
    b = []
    run_join()
    probes0 = store.index_info()["probe_launches"]
    for _ in range(3):
        b.append(run_join())
    used = store.index_info()["probe_launches"] > probes0
    assert all(x[1] == total for x in b)
    med = lambda xs: statistics.median(x[0] for x in xs)  # noqa: E731
    lines += [
        "%s: n = %d, L = 60, bound %d, blocks of %s rows, %s interleaved per span: %d pairs" % (
            label, n, D, os.environ.get("SMAFA_JOIN_BLOCK", "65536"), os.environ.get("SMAFA_JOIN_STRIDE", "16"), total),
        "  (a) self_launch, scan kernels     : median %.3f ms (runs %s), device time of its kernels %.1f ms" % (
            med(a), ", ".join("%.3f" % x[0] for x in a), statistics.median(x[2] for x in a)),
        "      kernels: %s" % "; ".join(kernels_a),
        "      stages : %s" % (stages[-1] if stages else "not captured"),
        "      blocks : %s" % blocks_a,
        "  (a1) the same, consecutive blocks : median %.3f ms (runs %s)" % (med(a1), ", ".join("%.3f" % x[0] for x in a1)),
        "      blocks : %s" % blocks_a1,
        "  (b) self_launch, block index      : median %.3f ms (runs %s); index max_div_served %s, probes used: %s" % (
            med(b), ", ".join("%.3f" % x[0] for x in b), info["max_div_served"], used),
        "  (c) %d x scan_launch of 65 536 rows : median %.3f ms (runs %s); %d rows before de-duplication" % (
            len(qsets), med(c), ", ".join("%.3f" % x[0] for x in c), c[0][1]),
        "  (a) / (c) = %.3f" % (med(a) / med(c)),
        "",
    ]
    for qs in qsets:
        qs.close()
    store.close()
    return med(a), med(c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_self_join.txt"))
    args = ap.parse_args()
    if smafa_amd.device_count() < 1:
        raise SystemExit("self_join_probe: no HIP device visible")
    lines = ["self-join probe — device %s, build id %s" % (torch.cuda.get_device_name(0), smafa_amd.build_id()), ""]
    ok = True
    for label, alphabet, D in (("amino acids", 1, 5), ("nucleotides", 0, 3)):
        a, c = probe(label, alphabet, args.rows, D, lines)
        ok = ok and a <= c
    lines.append("condition (a) <= (c): %s" % ("holds" if ok else "FAILS"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
