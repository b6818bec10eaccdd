"""The classification call beside the calls it is built on (profiles/r27_classify.txt).

The store and reads of §3.19's record — 10M x 60 aa (smafa_amd.synth), 1M planted reads, bound 5, three samples — and lineages of
R = 7 ranks derived from the store's families: the components at bound 5 are the species (rank 5 = the component's label, the
ranks above it the label divided by 8, 64, ...), rank 6 is the subject's own number (a strain), and every sixteenth subject's row
ends behind rank 3.  On one handle in one process, alternated rounds behind one warm-up each, medians:
  (a) smafa_db_classify_launch at slack 0 beside (b) smafa_db_assign_launch — the table call is unchanged and is the yardstick;
  (c) smafa_db_classify_launch at slack 2 beside (d) smafa_scan_launch(max_div = 5, max_num_hits = NONE) over the same set.
One more run of (a) and (c) with the library's level-2 line captured gives the split scan / best / agree / keys, sort and sums
and the number of rows classify::agree_kernel saw.

    python tools/classify_probe.py [--rows N] [--reads M] [--rounds R] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import smafa_amd  # noqa: E402
from smafa_amd import _lib, synth  # noqa: E402

NONE = 0xFFFFFFFF


def family_lineage(labels):
    n = len(labels)
    rows = np.zeros((n, 7), dtype=np.uint32)
    for r in range(6):
        rows[:, r] = labels // np.uint32(8 ** (5 - r))
    rows[:, 6] = np.arange(n, dtype=np.uint32)
    rows[::16, 4:] = NONE
    return rows


def traced(call):
    """one call with the library's level-2 stderr line captured -> the line"""
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        _lib.lib().smafa_set_verbosity(2)
        try:
            call()
        finally:
            _lib.lib().smafa_set_verbosity(0)
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        lines = [ln.strip() for ln in tmp.read().decode(errors="replace").splitlines() if "classification of" in ln]
        return lines[-1] if lines else "(no level-2 line)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, m, D, n_samples, E = args.rows, args.reads, 5, 3, 2
    subj = synth.subjects(n, 60, 1, seed=1)
    reads, _, _ = synth.queries(subj, m, 1, seed=3, max_subs=10)
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    store.push(subj)
    labels, n_components = store.self_components(D)
    lineage = family_lineage(labels)
    qset = smafa_amd.QuerySet(store, reads)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(a.astype(np.int64)).to(dev).to(torch.int32)  # noqa: E731  (the uint32 bits)
    d_labels, d_lineage = up(labels), up(lineage.reshape(-1))
    d_samples = up(np.random.default_rng(4).integers(0, n_samples, size=m).astype(np.uint32))
    per_read = [torch.zeros(m, dtype=torch.int32, device=dev) for _ in range(5)]
    d_entries = torch.zeros(2 * m, dtype=torch.int64, device=dev)
    d_totals4, d_totals6 = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(6, dtype=torch.int64, device=dev)
    cap_rows = 1 << 23
    d_hits, d_count = torch.zeros(3 * cap_rows, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def classify(slack):
        store.classify_launch(qset, D, slack, d_lineage.data_ptr(), 7, d_samples.data_ptr(), n_samples, 0, *[t.data_ptr() for t in per_read],
                              d_entries.data_ptr(), m, d_totals6.data_ptr())
        store.sync()
        return store.last_call_stats()

    def table():
        store.assign_launch(qset, D, d_labels.data_ptr(), d_samples.data_ptr(), n_samples, 0, per_read[0].data_ptr(), per_read[1].data_ptr(), 0,
                            d_entries.data_ptr(), m, d_totals4.data_ptr())
        store.sync()
        return store.last_call_stats()

    def scan_all():
        store.scan_launch(qset, D, None, d_hits.data_ptr(), cap_rows, d_count.data_ptr())
        store.sync()
        return store.last_scan_ms()

    classify(0), table(), classify(E), scan_all()  # warm-up: buffers grown, kernels loaded
    a_ms, b_ms, c_ms, d_ms = [], [], [], []
    for _ in range(args.rounds):
        a_ms.append(classify(0)["kernel_ms"])
        b_ms.append(table()["kernel_ms"])
        c_ms.append(classify(E)["kernel_ms"])
        d_ms.append(scan_all()[0])
    rows_all = int(d_count.cpu().numpy().view(np.uint64)[0])
    assert rows_all <= cap_rows, (rows_all, cap_rows)
    line0 = traced(lambda: classify(0))
    stats0, kernels0 = store.last_call_stats(), store.last_call_kernels()
    totals0 = d_totals6.cpu().numpy().view(np.uint64).copy()
    line2 = traced(lambda: classify(E))
    stats2 = store.last_call_stats()
    totals2 = d_totals6.cpu().numpy().view(np.uint64).copy()
    a, b, c, d = (statistics.median(x) for x in (a_ms, b_ms, c_ms, d_ms))
    fmt = lambda xs: ", ".join("%.3f" % x for x in xs)  # noqa: E731
    show = lambda t: "%d entries, weight %d assigned (%d on the root), %d unassigned, %d reads with ties" % (t[0], t[1], t[4], t[2], t[5])  # noqa: E731
    lines = [
        "classify probe — one MI355X, build id %s, %d rows x 60 aa, %d planted reads, bound %d, %d samples, R = 7 (species = the %d components at "
        "bound %d, rank 6 = the subject), SMAFA_ASSIGN_SPAN and SMAFA_ASSIGN_ROWS_MAX at their defaults" % (smafa_amd.build_id(), n, m, D, n_samples, n_components, D),
        "device time: smafa_last_call_stats behind the three calls, smafa_last_scan_ms behind the scan; one handle, one process; medians of %d "
        "alternated rounds (a, b, c, d) behind one warm-up each" % args.rounds,
        "",
        "  (a) classify, slack 0     : %8.3f ms (rounds: %s); %d scans, %d launches" % (a, fmt(a_ms), stats0["scans"], stats0["launches"]),
        "  (b) table (the yardstick) : %8.3f ms (rounds: %s)" % (b, fmt(b_ms)),
        "  (a) - (b)                 : %8.3f ms = %.1f %% of (b)" % (a - b, 100.0 * (a - b) / b),
        "  (c) classify, slack %d     : %8.3f ms (rounds: %s); %d scans, %d launches" % (E, c, fmt(c_ms), stats2["scans"], stats2["launches"]),
        "  (d) scan of every row <= %d: %8.3f ms (rounds: %s); %d rows" % (D, d, fmt(d_ms), rows_all),
        "  (c) - (d)                 : %8.3f ms = %.1f %% of (d)" % (c - d, 100.0 * (c - d) / d),
        "  slack 0: %s" % show(totals0),
        "  slack %d: %s" % (E, show(totals2)),
        "  the split of one more run each (the library's level-2 line):",
        "    " + line0,
        "    " + line2,
        "  kernels of (a), in first-launch order:",
    ] + ["    " + k for k in kernels0]
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
