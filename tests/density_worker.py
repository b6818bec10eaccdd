"""Worker for tests/test_gpu_density.py::test_device_form.

smafa_db_self_density_launch leaves the labels, the degrees and the three counters in HBM: they must equal the host form's
and the brute-force expectation, with and without a degree buffer, and the degrees must add up to twice the pair count of
smafa_db_self_launch with cap = 0.  torch supplies the device buffers (as bench.py does) and is imported first."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
torch.cuda.init()

import smafa_amd  # noqa: E402
from density_cases import brute_density  # noqa: E402
from self_join_cases import planted_store  # noqa: E402


def main():
    D, m = 5, 3
    for kind, alphabet, blocks in (("aa", 1, None), ("nt", 0, "4032")):
        if blocks:  # spans of 2 x 4 032 positions, two blocks interleaved in each (as tests/self_join_worker.py)
            os.environ["SMAFA_JOIN_BLOCK"] = blocks
            os.environ["SMAFA_JOIN_STRIDE"] = "2"
        codes = planted_store(31, kind, 60, 2000)
        labels, degrees, counts = brute_density(codes, D, m)
        want_counts = [counts["clusters"], counts["core"], counts["noise"]]
        n = len(codes)
        store = smafa_amd.SubjectStore(60, alphabet)
        os.environ.pop("SMAFA_JOIN_BLOCK", None)
        os.environ.pop("SMAFA_JOIN_STRIDE", None)
        store.push(codes)
        d_labels = torch.full((n + 64,), -2, dtype=torch.int32, device="cuda")
        d_degrees = torch.full((n + 64,), -2, dtype=torch.int32, device="cuda")
        d_counts = torch.full((4,), -2, dtype=torch.int64, device="cuda")
        for with_degrees in (True, False):
            d_labels.fill_(-2)
            d_degrees.fill_(-2)
            store.self_density_launch(D, m, d_labels.data_ptr(), d_degrees.data_ptr() if with_degrees else 0, d_counts.data_ptr())
            store.sync()
            stats = store.last_call_stats()
            assert stats["launches"] > 0 and stats["kernel_ms"] > 0, stats
            got = d_labels[:n].cpu().numpy().view(np.uint32)
            assert got.tobytes() == labels.tobytes()
            if with_degrees:
                assert d_degrees[:n].cpu().numpy().view(np.uint32).tobytes() == degrees.tobytes()
            else:
                assert int((d_degrees != -2).sum().item()) == 0
            assert d_counts[:3].tolist() == want_counts
            assert int((d_labels[n:] != -2).sum().item()) == 0 and int((d_degrees[n:] != -2).sum().item()) == 0  # nothing past them
            assert int(d_counts[3].item()) == -2
        d_pairs = torch.zeros((1,), dtype=torch.int64, device="cuda")
        store.self_launch(D, 0, 0, d_pairs.data_ptr())  # cap = 0 without a row buffer: counts only
        store.sync()
        assert int(degrees.astype(np.int64).sum()) == 2 * int(d_pairs.item()) and int(d_pairs.item()) > 0
        host = store.self_density(D, m)
        assert host[0].tobytes() == labels.tobytes() and host[1].tobytes() == degrees.tobytes() and host[2] == counts
        for bad in ((0, d_counts.data_ptr()), (d_labels.data_ptr(), 0)):
            try:
                store.self_density_launch(D, m, bad[0], d_degrees.data_ptr(), bad[1])
            except smafa_amd.SmafaError as e:
                assert e.code == smafa_amd._lib.ERR_INVALID and "NULL" in str(e)
            else:
                raise AssertionError("a NULL device buffer was accepted")
        store.close()
    print("density device form ok")


if __name__ == "__main__":
    main()
