"""Timing of the subset and rows calls (smafa_db_subset, smafa_db_rows) — profiles/r29_subset.txt.

The bench's store (smafa_amd.synth.subjects, --rows x 60 amino acids) under random keep masks of 10 %, 50 % and 90 %:
  * the subset: device ms (smafa_last_call_stats on the source) and wall ms around SubjectStore.subset, beside the only route
    there was before it — a fresh SubjectStore and push(codes[keep]) from host memory, wall ms (the fancy-indexing copy on the
    host timed apart) — same process, alternated;
  * the call's effective bandwidth: plane bytes read (all n rows) plus written (k rows), and the order words, over its device
    ms, beside smafa_hbm_read_probe on the same device;
  * rows(): 1M listed rows and the whole store, ms and GB/s of code bytes delivered (device, and wall with the copy to the host);
  * the scan cost of the result: the headline launch (10 000 planted queries, bound 5) on the 50 % subset beside the same launch
    on the fresh store of the same rows, smafa_last_scan_ms of --launches launches each behind a warm-up, alternated, and the
    mean shared filter bits per tile of both stores (the zone_hist means, from the library's level-2 lines)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from components_probe import traced  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_subset.txt"))
    args = ap.parse_args()
    import smafa_amd
    from smafa_amd import synth

    med = statistics.median
    L, alphabet = 60, 1
    codes = synth.subjects(args.rows, L, alphabet)
    n = len(codes)
    store = smafa_amd.SubjectStore(L, alphabet)
    t0 = time.perf_counter()
    store.push(codes)
    load_ms = (time.perf_counter() - t0) * 1e3
    info = store.info()
    row_bytes = info.planes * info.words_per_plane * 4
    stream = smafa_amd.hbm_read_probe(0, 4 << 30)
    out = ["subset probe — one MI355X, build id %s, %d rows x %d aa (%d planes x %d words, %d B per row); the store itself: push from host "
           "memory %.1f ms wall" % (smafa_amd.build_id(), n, L, info.planes, info.words_per_plane, row_bytes, load_ms),
           "smafa_hbm_read_probe on this device: %.0f GB/s" % stream, ""]
    rng = np.random.default_rng(5)
    subsets = {}
    for share in (0.1, 0.5, 0.9):
        keep = rng.random(n) < share
        k = int(keep.sum())
        sub, old = store.subset(keep)  # warm-up, and the result is checked once
        assert len(sub) == k and (old == np.flatnonzero(keep)).all()
        sample = rng.integers(0, k, size=2000)
        assert (sub.rows(sample) == codes[old[sample]]).all()
        sub.close()
        dev, wall, fresh_wall, index_wall = [], [], [], []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            sub, _ = store.subset(keep)
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(store.last_call_stats()["kernel_ms"])
            sub.close()
            t0 = time.perf_counter()
            kept = codes[keep]
            index_wall.append((time.perf_counter() - t0) * 1e3)
            fresh = smafa_amd.SubjectStore(L, alphabet)
            fresh.push(kept)
            fresh_wall.append((time.perf_counter() - t0) * 1e3)
            fresh.close()
            del kept
        moved = n * row_bytes + k * row_bytes + 4 * (n + k) + 4 * 4 * (n + 1)  # planes read and written, order[] both ways, flags and sums
        out.append("keep %2.0f %% (k = %d): subset device %.2f ms (rounds: %s), wall %.1f ms; fresh store + push(codes[keep]) wall %.1f ms "
                   "(of which codes[keep] on the host %.1f ms): %.1f x; bytes moved %.0f MB over device ms = %.0f GB/s (%.2f of the read probe)"
                   % (100 * share, k, med(dev), ", ".join("%.2f" % x for x in dev), med(wall), med(fresh_wall), med(index_wall),
                      med(fresh_wall) / med(wall), moved / 1e6, moved / med(dev) / 1e6, moved / med(dev) / 1e6 / stream))
        subsets[share] = keep
    out.append("")
    # ---- rows()
    listed = rng.integers(0, n, size=min(1_000_000, n)).astype(np.uint32)
    for name, call, m, head in (("1M listed rows", lambda: store.rows(listed), len(listed), codes[listed[:1000]]),
                                ("the whole store", lambda: store.rows(), n, codes[:1000])):
        got = call()
        assert len(got) == m and (got[:1000] == head).all()
        dev, wall = [], []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(store.last_call_stats()["kernel_ms"])
        out.append("rows(), %s: device %.2f ms = %.0f GB/s of code bytes, wall with the copy to the host %.1f ms = %.1f GB/s (rounds, device: %s)"
                   % (name, med(dev), m * L / med(dev) / 1e6, med(wall), m * L / med(wall) / 1e6, ", ".join("%.2f" % x for x in dev)))
        del got
    out.append("")
    # ---- the scan cost of the result
    keep = subsets[0.5]
    from smafa_amd import _lib
    (sub, _), sub_lines = traced(_lib.lib(), lambda: store.subset(keep))
    kept = codes[keep]
    fresh = smafa_amd.SubjectStore(L, alphabet)
    _, fresh_lines = traced(_lib.lib(), lambda: fresh.push(kept))
    queries, _, _ = synth.queries(kept, args.queries, alphabet, seed=3)
    runs = {}
    for name, s in (("subset", sub), ("fresh", fresh)):
        qset = smafa_amd.QuerySet(s, queries)
        rows = s.scan(queries[:500], 5)
        runs[name] = {"store": s, "qset": qset, "ms": [], "rows": rows}
    assert runs["subset"]["rows"].tobytes() == runs["fresh"]["rows"].tobytes()
    import ctypes as C

    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    cap = 1 << 22
    d_hits, d_count = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_hits), cap * 12) == 0 and hip.hipMalloc(C.byref(d_count), 8) == 0
    for i in range(args.launches + 3):
        for r in runs.values():
            r["store"].scan_launch(r["qset"], 5, None, d_hits.value, cap, d_count.value)
            r["store"].sync()
            if i >= 3:
                r["ms"].append(r["store"].last_scan_ms()[0])
            r["kernel"] = r["store"].last_scan_kernel()
    for name, r in runs.items():
        ms = sorted(r["ms"])
        out.append("headline launch (%d planted queries, bound 5) on the %s store of %d rows: median %.3f ms, min %.3f, max %.3f, "
                   "quartiles %.3f / %.3f over %d launches; %s" % (args.queries, name, len(kept), med(ms), ms[0], ms[-1], ms[len(ms) // 4],
                                                                   ms[3 * len(ms) // 4], len(ms), r["kernel"]))
        out.append("    all launches, in order: %s" % ", ".join("%.3f" % x for x in r["ms"]))
    out.append("zone_hist means — subset: %s" % next((ln for ln in reversed(sub_lines) if "shared filter bits" in ln), "no line"))
    out.append("zone_hist means — fresh:  %s" % next((ln for ln in reversed(fresh_lines) if "shared filter bits" in ln), "no line"))
    text = "\n".join(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
