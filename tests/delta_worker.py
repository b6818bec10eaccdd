"""Worker for tests/test_gpu_delta_join.py::test_device_forms.

smafa_db_self_since_launch leaves rows and count in HBM, smafa_db_self_components_update_launch takes and leaves its labels
there: both must equal the host forms and brute force.  torch supplies the device buffers (as bench.py does) and is imported
first."""
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
from delta_cases import since, store_case  # noqa: E402
from self_join_cases import sort_rows  # noqa: E402


def main():
    for name, alphabet in (("aa60", 1), ("nt60n", 0)):
        codes, want, D = store_case(name)
        n, n0 = len(codes), 2000
        expect = since(want, n0)
        total = len(expect)
        store = smafa_amd.SubjectStore(60, alphabet)
        store.push(codes[:n0])
        old_labels, _ = store.self_components(D)
        store.push(codes[n0:])
        # ---- pairs
        d_hits = torch.zeros((total + 64) * 3, dtype=torch.int32, device="cuda")
        d_count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()  # (torch fills on its own stream, the handle launches on another)
        store.self_since_launch(n0, D, d_hits.data_ptr(), total + 64, d_count.data_ptr())
        store.sync()
        assert int(d_count.item()) == total, (int(d_count.item()), total)
        assert sort_rows(d_hits[: 3 * total].cpu().numpy()).tobytes() == expect.tobytes()
        assert int(d_hits[3 * total:].abs().sum().item()) == 0
        stats = store.last_call_stats()
        assert stats["launches"] >= 4 and stats["kernel_ms"] > 0, stats
        assert store.self_pairs_since(n0, D).tobytes() == expect.tobytes()
        d_count.fill_(-1)
        torch.cuda.synchronize()  # (torch fills on its own stream, the handle launches on another)
        store.self_since_launch(n0, D, 0, 0, d_count.data_ptr())  # count only: no buffer at all
        store.sync()
        assert int(d_count.item()) == total
        cap = total // 3
        d_hits.zero_()
        d_count.fill_(-1)
        torch.cuda.synchronize()  # (torch fills on its own stream, the handle launches on another)
        store.self_since_launch(n0, D, d_hits.data_ptr(), cap, d_count.data_ptr())
        store.sync()
        assert int(d_count.item()) == total
        assert int(d_hits[3 * cap:].abs().sum().item()) == 0  # nothing past the capacity
        # ---- components
        full, _ = brute_labels(codes, D)
        given = np.full(n + 64, -1, dtype=np.int32)
        given[:n0] = old_labels.view(np.int32)
        d_labels = torch.from_numpy(given).cuda()
        d_count.fill_(-1)
        torch.cuda.synchronize()  # (torch fills on its own stream, the handle launches on another)
        store.self_components_update_launch(n0, D, d_labels.data_ptr(), d_count.data_ptr())
        store.sync()
        got = d_labels[:n].cpu().numpy().view(np.uint32)
        assert got.tobytes() == full.tobytes() and int(d_count.item()) == n_components(full)
        assert int((d_labels[n:] != -1).sum().item()) == 0  # nothing past the n labels
        labels, count = store.self_components_update(n0, D, old_labels)
        assert labels.tobytes() == got.tobytes() and count == int(d_count.item())
        # labels that are none: the device buffer is left as it was
        given[10] = 11
        d_labels = torch.from_numpy(given).cuda()
        torch.cuda.synchronize()
        try:
            store.self_components_update_launch(n0, D, d_labels.data_ptr(), d_count.data_ptr())
        except smafa_amd.SmafaError as e:
            assert e.code == smafa_amd._lib.ERR_INVALID and "labels" in str(e)
        else:
            raise AssertionError("a label above its row's number was accepted")
        store.sync()
        assert d_labels.cpu().numpy().tobytes() == given.tobytes()
        for bad in ((0, d_count.data_ptr()), (d_labels.data_ptr(), 0)):
            try:
                store.self_components_update_launch(n0, D, *bad)
            except smafa_amd.SmafaError as e:
                assert e.code == smafa_amd._lib.ERR_INVALID and "NULL" in str(e)
            else:
                raise AssertionError("a NULL device buffer was accepted")
        try:
            store.self_since_launch(n0, D, d_hits.data_ptr(), 8, 0)
        except smafa_amd.SmafaError as e:
            assert e.code == smafa_amd._lib.ERR_INVALID and "NULL" in str(e)
        else:
            raise AssertionError("a NULL count was accepted")
        store.close()
    print("delta device forms ok")


if __name__ == "__main__":
    main()
