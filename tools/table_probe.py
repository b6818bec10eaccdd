"""The abundance table's overhead over the scan it is built on (profiles/r26_table.txt).

The project's standard store — 10M x 60 aa (smafa_amd.synth) — and 1M planted reads at bound 5.  (a) one smafa_db_assign_launch
with three samples and the labels of smafa_db_self_components at the same bound: device time of all its spans and its own
kernels (smafa_last_call_stats); (b) smafa_scan_launch(max_div = 5, max_num_hits = 1) over the same query set on the same build:
the scan that existed before (smafa_last_scan_ms).  Alternated rounds behind one warm-up each; medians.

    python tools/table_probe.py [--rows N] [--reads M] [--rounds R] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import smafa_amd  # noqa: E402
from smafa_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, m, D, n_samples = args.rows, args.reads, 5, 3
    subj = synth.subjects(n, 60, 1, seed=1)
    reads, _, _ = synth.queries(subj, m, 1, seed=3, max_subs=10)
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    store.push(subj)
    labels, n_components = store.self_components(D)
    qset = smafa_amd.QuerySet(store, reads)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(a.astype(np.int64)).to(dev).to(torch.int32)  # noqa: E731  (the uint32 bits)
    d_labels = up(labels)
    d_samples = up(np.random.default_rng(4).integers(0, n_samples, size=m).astype(np.uint32))
    d_subject, d_dist = torch.zeros(m, dtype=torch.int32, device=dev), torch.zeros(m, dtype=torch.int32, device=dev)
    d_entries, d_totals = torch.zeros(2 * m, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
    cap_rows = 1 << 22
    d_hits, d_count = torch.zeros(3 * cap_rows, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def table():
        store.assign_launch(qset, D, d_labels.data_ptr(), d_samples.data_ptr(), n_samples, 0, d_subject.data_ptr(), d_dist.data_ptr(), 0,
                            d_entries.data_ptr(), m, d_totals.data_ptr())
        store.sync()
        return store.last_call_stats()

    def scan():
        store.scan_launch(qset, D, 1, d_hits.data_ptr(), cap_rows, d_count.data_ptr())
        store.sync()
        return store.last_scan_ms()

    table(), scan()  # warm-up: buffers grown, kernels loaded
    t_ms, s_ms = [], []
    for _ in range(args.rounds):
        t_ms.append(table()["kernel_ms"])
        s_ms.append(scan()[0])
    stats = table()
    kernels = store.last_call_kernels()
    totals = d_totals.cpu().numpy().view(np.uint64)
    rows = int(d_count.cpu().numpy().view(np.uint64)[0])
    a, b = statistics.median(t_ms), statistics.median(s_ms)
    fmt = lambda xs: ", ".join("%.3f" % x for x in xs)  # noqa: E731
    lines = [
        "table probe — one MI355X, build id %s, %d rows x 60 aa, %d planted reads, bound %d, %d samples, labels = the %d components at "
        "bound %d, SMAFA_ASSIGN_SPAN and SMAFA_ASSIGN_ROWS_MAX at their defaults" % (smafa_amd.build_id(), n, m, D, n_samples, n_components, D),
        "device time: (a) smafa_last_call_stats behind smafa_db_assign_launch (all spans and the call's own kernels); (b) smafa_last_scan_ms "
        "behind smafa_scan_launch(max_div = %d, max_num_hits = 1) over the same query set; medians of %d alternated rounds behind one warm-up each"
        % (D, args.rounds),
        "",
        "  (a) table                 : %8.3f ms (rounds: %s); %d scans, %d launches" % (a, fmt(t_ms), stats["scans"], stats["launches"]),
        "  (b) best-hit scan alone   : %8.3f ms (rounds: %s); %d rows at the reads' minimum distances" % (b, fmt(s_ms), rows),
        "  (a) - (b)                 : %8.3f ms = %.1f %% of (b)" % (a - b, 100.0 * (a - b) / b),
        "  table: %d entries, weight %d assigned, %d unassigned" % (int(totals[0]), int(totals[1]), int(totals[2])),
        "  kernels of (a), in first-launch order:",
    ] + ["    " + k for k in kernels]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    qset.close()
    store.close()


if __name__ == "__main__":
    main()
