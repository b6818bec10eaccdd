"""smafa_db_assign_launch on torch device buffers (run by tests/test_gpu_assign.py::test_device_form in a process of its own:
torch initialises HIP first).  The bytes must be the model's: every output at full capacity, the count alone at capacity 0 with
NULL entries, the first half of the table in table order at half the capacity, and a read whose sample number is out of range in
totals[3] and nowhere else."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import smafa_amd  # noqa: E402
from assign_cases import ASSIGN_KERNELS, TABLE_DTYPE, expected_assign, random_samples, random_weights, shape_reads  # noqa: E402
from consensus_cases import random_grouping  # noqa: E402


def main():
    codes, reads, _, _ = shape_reads("aa60", 150, 5, 4)
    n, m, D = len(codes), len(reads), 5
    labels, samples, weights = random_grouping(n, 3), random_samples(m, 3, 4), random_weights(m, 5)
    samples[[7, 100]] = [3, 0xFFFFFFFF]  # two reads of no sample: weights[7] and weights[100] count nowhere
    weights[[7, 100]] = [4, 5]
    want = expected_assign(codes, reads, D, labels, samples, 3, weights)
    clean = expected_assign(codes, np.delete(reads, [7, 100], axis=0), D, labels, np.delete(samples, [7, 100]), 3, np.delete(weights, [7, 100]))
    assert want[4].tolist() == clean[4].tolist()[:3] + [2] and want[0].tobytes() == clean[0].tobytes() and want[3].tobytes() == clean[3].tobytes()
    K = len(want[0])
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    store.push(codes)
    qset = smafa_amd.QuerySet(store, reads)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(a.astype(np.int64)).to(dev).to(torch.int32)  # noqa: E731  (the uint32 bits)
    d_labels, d_samples, d_weights = up(labels), up(samples), up(weights)
    fresh = lambda count, dtype=torch.int32: torch.full((count,), 5, dtype=dtype, device=dev)  # noqa: E731
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731

    def launch(cap, entries, per_read=True, counts=True):
        subject, dist, sc, totals = fresh(m), fresh(m), fresh(n, torch.int64), fresh(4, torch.int64)
        torch.cuda.synchronize()
        store.assign_launch(qset, D, d_labels.data_ptr(), d_samples.data_ptr(), 3, d_weights.data_ptr(), subject.data_ptr() if per_read else 0,
                            dist.data_ptr() if per_read else 0, sc.data_ptr() if counts else 0, entries.data_ptr() if entries is not None else 0,
                            cap, totals.data_ptr())
        store.sync()
        return subject, dist, sc, totals

    # every output, with room for two entries more than the table has: those are zeroed (the header says so), nothing behind them
    entries = fresh(2 * (K + 4), torch.int64)
    subject, dist, sc, totals = launch(K + 2, entries)
    got = entries.cpu().numpy().view(TABLE_DTYPE)
    assert got[:K].tobytes() == want[0].tobytes()
    assert (entries.cpu().numpy()[2 * K: 2 * (K + 2)] == 0).all() and (entries.cpu().numpy()[2 * (K + 2):] == 5).all()
    assert u32(subject).tobytes() == want[1].tobytes() and u32(dist).tobytes() == want[2].tobytes()
    assert u64(sc).tobytes() == want[3].tobytes() and u64(totals).tobytes() == want[4].tobytes()
    assert store.last_call_kernels()[-5:] == ASSIGN_KERNELS
    # cap = 0 with NULL entries: counted only; the optional outputs left out are not written
    subject, dist, sc, totals = launch(0, None, per_read=False, counts=False)
    assert u64(totals).tobytes() == want[4].tobytes()
    assert bool((subject == 5).all()) and bool((dist == 5).all()) and bool((sc == 5).all())
    # half the capacity: the first half in table order, the exact count, nothing behind it
    half = K // 2
    entries = fresh(2 * K, torch.int64)
    _, _, _, totals = launch(half, entries)
    assert int(u64(totals)[0]) == K and u64(totals).tobytes() == want[4].tobytes()
    assert entries.cpu().numpy().view(TABLE_DTYPE)[:half].tobytes() == want[0][:half].tobytes()
    assert (entries.cpu().numpy()[2 * half:] == 5).all()
    qset.close()
    store.close()
    print("table device form ok")


if __name__ == "__main__":
    main()
