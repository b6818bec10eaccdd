"""Timing of the consensus call (smafa_db_consensus_launch) — profiles/r23_consensus.txt.

The bench's stores (smafa_amd.synth.subjects, --rows x 60, amino acids and nucleotides) under three labellings: (a) the
components at bound 5 / 3, (b) all singletons, K = n, (c) one label for every row.  After a warm-up of each, --rounds alternated
rounds: wall clock around the launch form (it waits for its own work), the device time of smafa_last_scan_ms, and the stage
times and scratch bytes of the library's level-2 trace line.  Beside them the store's plane bytes over the tally-and-vote
stage as a share of the measured stream rate (6.7 TB/s, profiles/r04_stream_pmc.json), and the one baseline there is: the same
answer from the caller's code bytes in numpy on the host ((c) on all rows, (b) on the first --host-rows rows)."""
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

STREAM_TB_S = 6.7
STAGES = r"(groups|sort|tally and vote|measure) ([0-9.]+) ms"


def host_consensus(codes, labels):
    """the model of tests/consensus_cases.py without its loop over groups: per column one bincount over (group, code)"""
    ids, dense = np.unique(labels, return_inverse=True)
    K, (n, L) = len(ids), codes.shape
    cons = np.empty((K, L), dtype=np.uint8)
    for c in range(L):
        cons[:, c] = np.bincount(dense * 32 + codes[:, c], minlength=K * 32).reshape(K, 32).argmax(axis=1)
    div = (codes != cons[dense]).sum(axis=1)
    order = np.lexsort((np.arange(n), div, dense))
    nearest = order[np.r_[0, np.flatnonzero(np.diff(dense[order])) + 1]]
    return ids, np.bincount(dense, minlength=K), cons, nearest, div


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--host-rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--stores", default="aa,nt")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_consensus.txt"))
    args = ap.parse_args()
    import torch

    torch.cuda.init()
    import smafa_amd
    from smafa_amd import _lib, synth

    lib = _lib.lib()
    med = statistics.median
    out = ["consensus probe — one MI355X, build id %s, %d rows x 60, SMAFA_CONSENSUS_CHUNK at its default (4096)" % (smafa_amd.build_id(), args.rows),
           "wall: host clock around smafa_db_consensus_launch (which waits for its work); device: smafa_last_scan_ms; medians of %d "
           "alternated rounds behind one warm-up each" % args.rounds, ""]
    for label in args.stores.split(","):
        alphabet, D = (1, 5) if label == "aa" else (0, 3)
        codes = synth.subjects(args.rows, 60, alphabet)
        n, L = codes.shape
        store = smafa_amd.SubjectStore(L, alphabet)
        store.push(codes)
        info = store.info()
        components, n_components = store.self_components(D)
        labellings = {"(a) components at %d" % D: components, "(b) singletons": np.arange(n, dtype=np.uint32),
                      "(c) one label": np.zeros(n, dtype=np.uint32)}
        runs = {}
        for name, labels in labellings.items():
            d_labels = torch.from_numpy(labels.view(np.int32)).cuda()
            try:
                K = store.cluster_consensus_launch(d_labels.data_ptr(), 0, 0, 0)
            except smafa_amd.SmafaError as e:
                K = e.count
            bufs = [torch.empty(K, dtype=torch.int32, device="cuda") for _ in range(3)] + [torch.empty(K * L, dtype=torch.uint8, device="cuda"),
                                                                                           torch.empty(n, dtype=torch.int32, device="cuda")]
            ids, sizes, nearest, cons, div = bufs
            call = lambda a=d_labels, b=(ids, sizes, cons, nearest, div), k=K: store.cluster_consensus_launch(  # noqa: E731
                a.data_ptr(), *(t.data_ptr() for t in b), k)
            call()
            runs[name] = {"K": K, "call": call, "bufs": bufs, "labels": d_labels, "wall": [], "device": []}
        for _ in range(args.rounds):
            for r in runs.values():
                t0 = time.perf_counter()
                r["call"]()
                r["wall"].append((time.perf_counter() - t0) * 1e3)
                r["device"].append(store.last_scan_ms()[0])
        out.append("%s: n = %d, %d planes x %d words, plane bytes %d, %d components at bound %d" % (
            label, n, info.planes, info.words_per_plane, info.hbm_bytes, n_components, D))
        for name, r in runs.items():
            _, lines = traced(lib, r["call"])
            line = next(ln for ln in reversed(lines) if "consensus of" in ln)
            st = {k: float(v) for k, v in re.findall(STAGES, line)}
            scratch = int(re.search(r"scratch (\d+) B", line).group(1))
            K = r["K"]
            bound = 16 * ((n + 255) // 256 * 256) + 8 * (n + 1) + (12 + 4 * info.planes * info.words_per_plane) * K + \
                4096 * info.words_per_plane * ((n + 4095) // 4096)
            share = info.hbm_bytes / (st["tally and vote"] * 1e-3) / (STREAM_TB_S * 1e12)
            r.update(stages=st, scratch=scratch, bound=bound, share=share, wall_ms=med(r["wall"]), device_ms=med(r["device"]))
            out.append("  %-22s K = %8d: wall %8.2f ms, device %8.2f ms (rounds: %s); stages: %s; planes / tally-and-vote = %.3f of %.1f TB/s; "
                       "scratch %d B (bound without sort_tmp: %d B)" % (
                           name, K, r["wall_ms"], r["device_ms"], ", ".join("%.2f" % x for x in r["device"]),
                           ", ".join("%s %.3f" % kv for kv in st.items()), share, STREAM_TB_S, scratch, bound))
        a, c = runs["(a) components at %d" % D], runs["(c) one label"]
        out.append("  (c) / (a): device %.2f, wall %.2f" % (c["device_ms"] / a["device_ms"], c["wall_ms"] / a["wall_ms"]))
        # the device's bytes against the host's, then the host's time
        for name, rows in (("(c) one label", n), ("(b) singletons", min(n, args.host_rows))):
            labels = labellings[name][:rows]
            t0 = time.perf_counter()
            want = host_consensus(codes[:rows], labels)
            host_s = time.perf_counter() - t0
            same = "not compared (a slice)"
            if rows == n:
                ids, sizes, nearest, cons, div = (t.cpu().numpy() for t in runs[name]["bufs"])
                got = (ids.view(np.uint32), sizes.view(np.uint32), cons.reshape(-1, L), nearest.view(np.uint32), div.view(np.uint32))
                same = "device bytes equal: %s" % all((g == w).all() for g, w in zip(got, want))
            out.append("  host numpy, %-16s on %d rows: %.2f s (%s)" % (name, rows, host_s, same))
        out.append("")
        for r in runs.values():
            r.pop("call"), r.pop("bufs"), r.pop("labels")
        print(json.dumps({label: runs}), flush=True)
        store.close()
        del runs
        torch.cuda.empty_cache()
    text = "\n".join(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
