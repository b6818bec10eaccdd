"""Worker for tests/test_gpu_forest.py::test_device_form.

smafa_db_self_forest_launch leaves the edges and the level ends in HBM: they must pass forest_cases.check_forest (brute force
on the code bytes) as they lie — ordered by distance, in any order inside a level — and nothing may be written past them.
torch supplies the device buffers (as bench.py does) and is imported first."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
torch.cuda.init()

import smafa_amd  # noqa: E402
from forest_cases import as_edges, check_forest, expected_levels  # noqa: E402
from self_join_cases import planted_store  # noqa: E402


def main():
    D = 5
    for kind, alphabet, blocks in (("aa", 1, None), ("nt", 0, "4032")):
        if blocks:  # spans of 2 x 4 032 positions, two blocks interleaved in each (as tests/self_join_worker.py)
            os.environ["SMAFA_JOIN_BLOCK"] = blocks
            os.environ["SMAFA_JOIN_STRIDE"] = "2"
        codes = planted_store(31, kind, 60, 2000)
        counts = expected_levels(codes, D)[1]
        n = len(codes)
        store = smafa_amd.SubjectStore(60, alphabet)
        os.environ.pop("SMAFA_JOIN_BLOCK", None)
        os.environ.pop("SMAFA_JOIN_STRIDE", None)
        store.push(codes)
        d_edges = torch.full((3 * (n - 1) + 64,), -1, dtype=torch.int32, device="cuda")
        d_ends = torch.full((D + 2,), -1, dtype=torch.int64, device="cuda")
        store.self_forest_launch(D, d_edges.data_ptr(), d_ends.data_ptr())
        store.sync()
        stats = store.last_call_stats()
        assert stats["launches"] > 0 and stats["kernel_ms"] > 0, stats
        ends = np.array(d_ends[:D + 1].tolist(), dtype=np.uint64)
        assert ends.tolist() == [n - c for c in counts], (ends.tolist(), counts)
        m = int(ends[-1])
        got = as_edges(d_edges[:3 * m].cpu().numpy().view(np.uint32))
        check_forest(codes, got, ends, D)
        assert int((d_edges[3 * m:] != -1).sum().item()) == 0 and int(d_ends[D + 1].item()) == -1  # nothing past them
        edges, host_ends = store.self_forest(D)  # the host form: the same counts, its own order, the same contract
        assert host_ends.tolist() == ends.tolist()
        check_forest(codes, edges, host_ends, D)
        for bad in ((0, d_ends.data_ptr()), (d_edges.data_ptr(), 0)):
            try:
                store.self_forest_launch(D, *bad)
            except smafa_amd.SmafaError as e:
                assert e.code == smafa_amd._lib.ERR_INVALID and "NULL" in str(e)
            else:
                raise AssertionError("a NULL device buffer was accepted")
        store.close()
    print("forest device form ok")


if __name__ == "__main__":
    main()
