"""Worker for tests/test_gpu_reach_forest.py::test_device_form.

smafa_db_self_reach_forest_launch leaves the edges, the level ends and — where asked — the cores in HBM: they must pass
reach_cases.check_reach_forest (brute force on the code bytes) as they lie — ordered by weight, in any order inside a level —
and nothing may be written past them.  torch supplies the device buffers (as bench.py does) and is imported first."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
torch.cuda.init()

import smafa_amd  # noqa: E402
from forest_cases import as_edges  # noqa: E402
from reach_cases import check_reach_forest, expected_reach  # noqa: E402
from self_join_cases import planted_store  # noqa: E402


def main():
    D, M = 5, 4
    for kind, alphabet, blocks in (("aa", 1, None), ("nt", 0, "4032")):
        if blocks:  # spans of 2 x 4 032 positions, two blocks interleaved in each (as tests/self_join_worker.py)
            os.environ["SMAFA_JOIN_BLOCK"] = blocks
            os.environ["SMAFA_JOIN_STRIDE"] = "2"
        codes = planted_store(31, kind, 60, 2000)
        want_cores, _, counts = expected_reach(codes, D, M)
        n = len(codes)
        store = smafa_amd.SubjectStore(60, alphabet)
        os.environ.pop("SMAFA_JOIN_BLOCK", None)
        os.environ.pop("SMAFA_JOIN_STRIDE", None)
        store.push(codes)
        for with_cores in (True, False):
            d_edges = torch.full((3 * (n - 1) + 64,), -1, dtype=torch.int32, device="cuda")
            d_ends = torch.full((D + 2,), -1, dtype=torch.int64, device="cuda")
            d_cores = torch.full((n + 16,), 77, dtype=torch.int32, device="cuda")
            store.self_reach_forest_launch(D, M, d_edges.data_ptr(), d_ends.data_ptr(), d_cores.data_ptr() if with_cores else 0)
            store.sync()
            stats = store.last_call_stats()
            assert stats["launches"] > 0 and stats["kernel_ms"] > 0, stats
            ends = np.array(d_ends[:D + 1].tolist(), dtype=np.uint64)
            assert ends.tolist() == [n - c for c in counts], (ends.tolist(), counts)
            m = int(ends[-1])
            got = as_edges(d_edges[:3 * m].cpu().numpy().view(np.uint32))
            cores = d_cores[:n].cpu().numpy().view(np.uint32).copy() if with_cores else np.array(want_cores)
            if not with_cores:
                assert int((d_cores != 77).sum().item()) == 0  # no buffer given: none written
            check_reach_forest(codes, got, ends, cores, D, M)
            assert int((d_edges[3 * m:] != -1).sum().item()) == 0 and int(d_ends[D + 1].item()) == -1  # nothing past them
            assert int((d_cores[n:] != 77).sum().item()) == 0
        edges, host_ends, host_cores = store.self_reach_forest(D, M)  # the host form: the same counts, its own order, the same contract
        assert host_ends.tolist() == ends.tolist()
        check_reach_forest(codes, edges, host_ends, host_cores, D, M)
        for bad in ((0, d_ends.data_ptr()), (d_edges.data_ptr(), 0)):
            try:
                store.self_reach_forest_launch(D, M, *bad)
            except smafa_amd.SmafaError as e:
                assert e.code == smafa_amd._lib.ERR_INVALID and "NULL" in str(e)
            else:
                raise AssertionError("a NULL device buffer was accepted")
        store.close()
    print("reach forest device form ok")


if __name__ == "__main__":
    main()
