"""Worker for tests/test_gpu_stable.py::test_device_form.

smafa_db_self_stable_launch leaves the labels and — where asked — the joined levels and the cores in HBM and returns the cluster
count: they must equal stable_cases.expected_stable (brute force on the code bytes and the definition) byte for byte, nothing may
be written past them, and a buffer that was not given is not written.  torch supplies the device buffers (as bench.py does) and
is imported first."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
torch.cuda.init()

import smafa_amd  # noqa: E402
from stable_cases import check_stable, expected_stable, planted_codes  # noqa: E402


def main():
    D, M, S = 5, 3, 4
    for kind, alphabet, blocks in (("aa", 1, None), ("ntn", 0, "128")):
        if blocks:  # spans of 2 x 128 positions, two blocks interleaved in each
            os.environ["SMAFA_JOIN_BLOCK"] = blocks
            os.environ["SMAFA_JOIN_STRIDE"] = "2"
        codes = planted_codes(kind)
        want, want_joined, want_count, want_cores = expected_stable(codes, D, M, S)
        n = len(codes)
        store = smafa_amd.SubjectStore(60, alphabet)
        os.environ.pop("SMAFA_JOIN_BLOCK", None)
        os.environ.pop("SMAFA_JOIN_STRIDE", None)
        store.push(codes)
        for with_joined, with_cores in ((True, True), (False, True), (True, False), (False, False)):
            d_labels, d_joined, d_cores = (torch.full((n + 16,), 77, dtype=torch.int32, device="cuda") for _ in range(3))
            count = store.self_stable_clusters_launch(D, M, S, d_labels.data_ptr(), d_joined.data_ptr() if with_joined else 0,
                                                      d_cores.data_ptr() if with_cores else 0)
            stats = store.last_call_stats()  # (the call has waited: no sync in front of the reads)
            assert stats["launches"] > 0 and stats["kernel_ms"] > 0, stats
            host = lambda d: d[:n].cpu().numpy().view(np.uint32).copy()  # noqa: E731
            for given, d in ((with_joined, d_joined), (with_cores, d_cores)):
                if not given:
                    assert int((d != 77).sum().item()) == 0  # no buffer given: none written
            check_stable(codes, (host(d_labels), count, host(d_joined) if with_joined else np.array(want_joined),
                                 host(d_cores) if with_cores else np.array(want_cores)), D, M, S)
            for d in (d_labels, d_joined, d_cores):
                assert int((d[n:] != 77).sum().item()) == 0  # nothing past them
        check_stable(codes, store.self_stable_clusters(D, M, S, joined=True, cores=True), D, M, S)  # the host form: the same bytes
        try:
            store.self_stable_clusters_launch(D, M, S, 0)
        except smafa_amd.SmafaError as e:
            assert e.code == smafa_amd._lib.ERR_INVALID and "NULL labels" in str(e)
        else:
            raise AssertionError("a NULL device buffer was accepted")
        store.close()
    print("stable clusters device form ok")


if __name__ == "__main__":
    main()
