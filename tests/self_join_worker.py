"""Worker for tests/test_gpu_self_join.py::test_device_form_and_capacity.

smafa_db_self_launch leaves rows and count in HBM: with room for every pair the row SET is the brute-force one; without a
buffer the count alone is exact; with a third of the room the count is still exact and the stored rows are a repeat-free
subset.  torch supplies the device buffers (as bench.py does) and is imported first."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
torch.cuda.init()

import oracle  # noqa: E402
import smafa_amd  # noqa: E402
from self_join_cases import brute_pairs, check_against_oracle, planted_store, sort_rows  # noqa: E402


def main():
    oracle.build()
    for kind, alphabet, blocks in (("aa", 1, None), ("nt", 0, "4032")):
        if blocks:  # spans of 2 x 4 032 positions: they start between wave tiles (the cut rounds down), two blocks interleaved in each
            os.environ["SMAFA_JOIN_BLOCK"] = blocks
            os.environ["SMAFA_JOIN_STRIDE"] = "2"
        codes = planted_store(31, kind, 60, 2000)
        want = brute_pairs(codes, 5)
        check_against_oracle(codes, want, 5)
        assert len(want) > 0 and (want["dist"] == 0).sum() >= 1
        store = smafa_amd.SubjectStore(60, alphabet)
        os.environ.pop("SMAFA_JOIN_BLOCK", None)
        os.environ.pop("SMAFA_JOIN_STRIDE", None)
        store.push(codes)
        total = len(want)
        d_hits = torch.zeros((total + 64) * 3, dtype=torch.int32, device="cuda")
        d_count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        store.self_launch(5, d_hits.data_ptr(), total + 64, d_count.data_ptr())
        store.sync()
        assert int(d_count.item()) == total, (int(d_count.item()), total)
        assert sort_rows(d_hits[: 3 * total].cpu().numpy()).tobytes() == want.tobytes()
        # (records + scan + filter per block; 20 020 rows in spans of 8 064: two blocks, two blocks, one)
        assert store.last_call_stats()["launches"] >= (3 if not blocks else 3 + 2 * 5), store.last_call_stats()
        d_count.fill_(-1)
        store.self_launch(5, 0, 0, d_count.data_ptr())  # count only: no buffer at all
        store.sync()
        assert int(d_count.item()) == total
        cap = total // 3
        d_hits.zero_()
        d_count.fill_(-1)
        store.self_launch(5, d_hits.data_ptr(), cap, d_count.data_ptr())
        store.sync()
        assert int(d_count.item()) == total
        assert int(d_hits[3 * cap:].abs().sum().item()) == 0  # nothing past the capacity
        part = sort_rows(d_hits[: 3 * cap].cpu().numpy())
        key = lambda r: (r["query"].astype(np.int64) << 32) | r["subject"]  # noqa: E731
        assert len(np.unique(key(part))) == cap
        have = {(int(r["query"]), int(r["subject"]), int(r["dist"])) for r in want}
        assert all((int(r["query"]), int(r["subject"]), int(r["dist"])) in have for r in part)
        # smafa_scan_each after a join: smafa_last_scan_ms is that call's own figure, not the totals the join left on the handle
        join_ms, join_launches = store.last_scan_ms()
        assert join_launches >= 3 and abs(join_ms - store.last_call_stats()["kernel_ms"]) < 1e-3
        nq = 7
        qs = smafa_amd.QuerySet(store, codes[:nq])
        each_hits = torch.zeros(nq * 64 * 3, dtype=torch.int32, device="cuda")
        each_counts = torch.zeros(nq, dtype=torch.int64, device="cuda")
        store.scan_each(qs, 5, each_hits.data_ptr(), 64, each_counts.data_ptr())
        store.sync()
        ms, launches = store.last_scan_ms()
        assert launches == nq and 0 < ms < join_ms, (ms, launches, join_ms, join_launches)
        assert int(each_counts.sum().item()) >= nq  # every query is a store row: it finds itself
        qs.close()
        store.close()
    print("self-join device form ok")


if __name__ == "__main__":
    main()
