"""Worker for tests/test_gpu_peaks.py::test_device_form.

smafa_db_self_peaks_launch leaves the labels, the parents, the weights and the peak count in HBM: they must equal the host
form's and the brute-force expectation, with and without the optional buffers, and nothing may be written past them.  torch
supplies the device buffers (as bench.py does) and is imported first."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
torch.cuda.init()

import smafa_amd  # noqa: E402
from peaks_cases import brute_peaks  # noqa: E402
from self_join_cases import planted_store  # noqa: E402


def main():
    D = 5
    for kind, alphabet, blocks, r in (("aa", 1, None, 0), ("nt", 0, "4032", D)):
        if blocks:  # spans of 2 x 4 032 positions, two blocks interleaved in each (as tests/self_join_worker.py)
            os.environ["SMAFA_JOIN_BLOCK"] = blocks
            os.environ["SMAFA_JOIN_STRIDE"] = "2"
        codes = planted_store(31, kind, 60, 2000)
        labels, parents, weights, n_peaks = brute_peaks(codes, D, r)
        n = len(codes)
        store = smafa_amd.SubjectStore(60, alphabet)
        os.environ.pop("SMAFA_JOIN_BLOCK", None)
        os.environ.pop("SMAFA_JOIN_STRIDE", None)
        store.push(codes)
        d_labels, d_parents, d_weights = (torch.full((n + 64,), -2, dtype=torch.int32, device="cuda") for _ in range(3))
        d_count = torch.full((2,), -2, dtype=torch.int64, device="cuda")
        for with_parents, with_weights in ((True, True), (False, False), (True, False)):
            for t in (d_labels, d_parents, d_weights):
                t.fill_(-2)
            store.self_peaks_launch(D, r, d_labels.data_ptr(), d_parents.data_ptr() if with_parents else 0,
                                    d_weights.data_ptr() if with_weights else 0, d_count.data_ptr())
            store.sync()
            stats = store.last_call_stats()
            assert stats["launches"] > 0 and stats["kernel_ms"] > 0, stats
            assert d_labels[:n].cpu().numpy().view(np.uint32).tobytes() == labels.tobytes()
            if with_parents:
                assert d_parents[:n].cpu().numpy().view(np.uint32).tobytes() == parents.tobytes()
            else:
                assert int((d_parents != -2).sum().item()) == 0
            if with_weights:
                assert d_weights[:n].cpu().numpy().view(np.uint32).tobytes() == weights.tobytes()
            else:
                assert int((d_weights != -2).sum().item()) == 0
            assert d_count.tolist() == [n_peaks, -2]
            for t in (d_labels, d_parents, d_weights):
                assert int((t[n:] != -2).sum().item()) == 0  # nothing past them
        host = store.self_peaks(D, r)
        assert host[0].tobytes() == labels.tobytes() and host[1].tobytes() == parents.tobytes()
        assert host[2].tobytes() == weights.tobytes() and host[3] == n_peaks
        for bad in ((0, d_count.data_ptr()), (d_labels.data_ptr(), 0)):
            try:
                store.self_peaks_launch(D, r, bad[0], d_parents.data_ptr(), d_weights.data_ptr(), bad[1])
            except smafa_amd.SmafaError as e:
                assert e.code == smafa_amd._lib.ERR_INVALID and "NULL" in str(e)
            else:
                raise AssertionError("a NULL device buffer was accepted")
        store.close()
    print("peaks device form ok")


if __name__ == "__main__":
    main()
