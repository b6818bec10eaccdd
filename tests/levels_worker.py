"""Worker for tests/test_gpu_levels.py::test_device_form.

smafa_db_self_levels_launch leaves the labels of every level and the numbers of components in HBM: both must equal the
host form's and the brute-force expectation.  torch supplies the device buffers (as bench.py does) and is imported first."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
torch.cuda.init()

import smafa_amd  # noqa: E402
from levels_cases import brute_levels  # noqa: E402
from self_join_cases import planted_store  # noqa: E402


def main():
    D = 5
    for kind, alphabet, blocks in (("aa", 1, None), ("nt", 0, "4032")):
        if blocks:  # spans of 2 x 4 032 positions, two blocks interleaved in each (as tests/self_join_worker.py)
            os.environ["SMAFA_JOIN_BLOCK"] = blocks
            os.environ["SMAFA_JOIN_STRIDE"] = "2"
        codes = planted_store(31, kind, 60, 2000)
        want, counts, _ = brute_levels(codes, D)
        n = len(codes)
        store = smafa_amd.SubjectStore(60, alphabet)
        os.environ.pop("SMAFA_JOIN_BLOCK", None)
        os.environ.pop("SMAFA_JOIN_STRIDE", None)
        store.push(codes)
        d_labels = torch.full(((D + 1) * n + 64,), -1, dtype=torch.int32, device="cuda")
        d_counts = torch.full((D + 2,), -1, dtype=torch.int64, device="cuda")
        store.self_component_levels_launch(D, d_labels.data_ptr(), d_counts.data_ptr())
        store.sync()
        stats = store.last_call_stats()
        assert stats["launches"] > 0 and stats["kernel_ms"] > 0, stats
        got = d_labels[:(D + 1) * n].cpu().numpy().view(np.uint32).reshape(D + 1, n)
        assert got.tobytes() == want.tobytes()
        assert d_counts[:D + 1].tolist() == counts
        assert int((d_labels[(D + 1) * n:] != -1).sum().item()) == 0 and int(d_counts[D + 1].item()) == -1  # nothing past them
        labels, host_counts = store.self_component_levels(D)
        assert labels.tobytes() == got.tobytes() and host_counts == counts
        for bad in ((0, d_counts.data_ptr()), (d_labels.data_ptr(), 0)):
            try:
                store.self_component_levels_launch(D, *bad)
            except smafa_amd.SmafaError as e:
                assert e.code == smafa_amd._lib.ERR_INVALID and "NULL" in str(e)
            else:
                raise AssertionError("a NULL device buffer was accepted")
        store.close()
    print("levels device form ok")


if __name__ == "__main__":
    main()
