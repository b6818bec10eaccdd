"""Worker for tests/test_gpu_components.py::test_device_form.

smafa_db_self_components_launch leaves the labels and the number of components in HBM: both must equal the host form's and
the brute-force expectation.  torch supplies the device buffers (as bench.py does) and is imported first."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
torch.cuda.init()

import smafa_amd  # noqa: E402
from components_cases import brute_labels, n_components  # noqa: E402
from self_join_cases import planted_store  # noqa: E402


def main():
    for kind, alphabet, blocks in (("aa", 1, None), ("nt", 0, "4032")):
        if blocks:  # spans of 2 x 4 032 positions, two blocks interleaved in each (as tests/self_join_worker.py)
            os.environ["SMAFA_JOIN_BLOCK"] = blocks
            os.environ["SMAFA_JOIN_STRIDE"] = "2"
        codes = planted_store(31, kind, 60, 2000)
        want, _ = brute_labels(codes, 5)
        n = len(codes)
        store = smafa_amd.SubjectStore(60, alphabet)
        os.environ.pop("SMAFA_JOIN_BLOCK", None)
        os.environ.pop("SMAFA_JOIN_STRIDE", None)
        store.push(codes)
        d_labels = torch.full((n + 64,), -1, dtype=torch.int32, device="cuda")
        d_count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        store.self_components_launch(5, d_labels.data_ptr(), d_count.data_ptr())
        store.sync()
        stats = store.last_call_stats()
        assert stats["launches"] > 0 and stats["kernel_ms"] > 0, stats
        got = d_labels[:n].cpu().numpy().view(np.uint32)
        assert got.tobytes() == want.tobytes()
        assert int(d_count.item()) == n_components(want)
        assert int((d_labels[n:] != -1).sum().item()) == 0  # nothing past the n labels
        labels, count = store.self_components(5)
        assert labels.tobytes() == got.tobytes() and count == int(d_count.item())
        for bad in ((0, d_count.data_ptr()), (d_labels.data_ptr(), 0)):
            try:
                store.self_components_launch(5, *bad)
            except smafa_amd.SmafaError as e:
                assert e.code == smafa_amd._lib.ERR_INVALID and "NULL" in str(e)
            else:
                raise AssertionError("a NULL device buffer was accepted")
        store.close()
    print("components device form ok")


if __name__ == "__main__":
    main()
