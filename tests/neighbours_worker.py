"""Worker for tests/test_gpu_neighbours.py::test_device_form.

smafa_db_self_neighbours_launch leaves the offsets, the lists and the total in HBM: they must equal brute force, with and
without the distances and the cut; the capacity protocol must behave as the host form's — offsets and total exact at
cap = 0 and at total - 1, the lists untouched, success at exactly total — and nothing may be written past the buffers.
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
from neighbours_cases import brute_neighbours, cut_lists  # noqa: E402
from self_join_cases import planted_store  # noqa: E402


def main():
    D = 5
    for kind, alphabet, blocks in (("aa", 1, None), ("nt", 0, "2048")):
        if blocks:  # spans of 2 x 2 048 positions, two blocks interleaved in each (as tests/self_join_worker.py)
            os.environ["SMAFA_JOIN_BLOCK"] = blocks
            os.environ["SMAFA_JOIN_STRIDE"] = "2"
        codes = planted_store(31, kind, 60, 600)
        n = len(codes)
        store = smafa_amd.SubjectStore(60, alphabet)
        os.environ.pop("SMAFA_JOIN_BLOCK", None)
        os.environ.pop("SMAFA_JOIN_STRIDE", None)
        store.push(codes)
        d_offsets = torch.full((n + 1 + 8,), -2, dtype=torch.int64, device="cuda")
        d_total = torch.full((2,), -2, dtype=torch.int64, device="cuda")
        whole = brute_neighbours(codes, D)
        for k in (None, 3):
            offsets, nb, ds = cut_lists(whole, k)
            total = len(nb)
            assert total > n
            d_nb, d_ds = (torch.full((total + 64,), -2, dtype=torch.int32, device="cuda") for _ in range(2))

            def launch(cap, lists=True, dists=True):
                d_offsets.fill_(-2)
                d_total.fill_(-2)
                try:
                    store.self_neighbours_launch(D, k, d_offsets.data_ptr(), d_nb.data_ptr() if lists else 0,
                                                 d_ds.data_ptr() if lists and dists else 0, cap, d_total.data_ptr())
                    code = 0
                except smafa_amd.SmafaError as e:
                    code = e.code
                store.sync()
                assert d_offsets[: n + 1].cpu().numpy().view(np.uint64).tobytes() == offsets.tobytes()  # exact at any capacity
                assert int((d_offsets[n + 1:] != -2).sum().item()) == 0 and d_total.tolist() == [total, -2]
                return code

            def untouched():
                return int((d_nb != -2).sum().item()) == 0 and int((d_ds != -2).sum().item()) == 0

            assert launch(0, lists=False) == smafa_amd._lib.ERR_CAPACITY and untouched()
            assert launch(total - 1) == smafa_amd._lib.ERR_CAPACITY and untouched()
            assert launch(total) == 0
            stats = store.last_call_stats()
            assert stats["launches"] > 0 and stats["kernel_ms"] > 0, stats
            assert d_nb[:total].cpu().numpy().view(np.uint32).tobytes() == nb.tobytes()
            assert d_ds[:total].cpu().numpy().view(np.uint32).tobytes() == ds.tobytes()
            assert int((d_nb[total:] != -2).sum().item()) == 0 and int((d_ds[total:] != -2).sum().item()) == 0  # nothing past them
            d_nb.fill_(-2)
            d_ds.fill_(-2)
            assert launch(total + 64, dists=False) == 0
            assert d_nb[:total].cpu().numpy().view(np.uint32).tobytes() == nb.tobytes()
            assert int((d_nb[total:] != -2).sum().item()) == 0 and int((d_ds != -2).sum().item()) == 0
            host = store.self_neighbours(D, k)
            assert host[0].tobytes() == offsets.tobytes() and host[1].tobytes() == nb.tobytes() and host[2].tobytes() == ds.tobytes()
        for bad in ((0, d_nb.data_ptr(), d_total.data_ptr()), (d_offsets.data_ptr(), d_nb.data_ptr(), 0), (d_offsets.data_ptr(), 0, d_total.data_ptr())):
            try:
                store.self_neighbours_launch(D, None, bad[0], bad[1], 0, 16, bad[2])
            except smafa_amd.SmafaError as e:
                assert e.code == smafa_amd._lib.ERR_INVALID and "NULL" in str(e)
            else:
                raise AssertionError("a NULL device buffer was accepted")
        store.close()
    print("neighbours device form ok")


if __name__ == "__main__":
    main()
