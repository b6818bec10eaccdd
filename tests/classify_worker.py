"""smafa_db_classify_launch on torch device buffers (run by tests/test_gpu_classify.py::test_device_form in a process of its own:
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
from assign_cases import TABLE_DTYPE, random_samples, random_weights  # noqa: E402
from classify_cases import CLASSIFY_KERNELS, expected_classify, tie_case, tie_lineage  # noqa: E402

CASE = ("aa60", 150, 5, 4)


def main():
    codes, reads, dmat = tie_case(*CASE)
    m, D, R, slack = len(reads), 5, 7, 1
    lineage = tie_lineage(*CASE, R)
    samples, weights = random_samples(m, 3, 4), random_weights(m, 5)
    samples[[7, 100]] = [3, 0xFFFFFFFF]  # two reads of no sample: weights[7] and weights[100] count nowhere
    weights[[7, 100]] = [4, 5]
    want = expected_classify(codes, reads, D, lineage, slack, samples, 3, weights, dmat=dmat)
    keep = np.setdiff1d(np.arange(m), [7, 100])
    clean = expected_classify(codes, reads[keep], D, lineage, slack, samples[keep], 3, weights[keep], dmat=dmat[keep])
    assert want[0].tobytes() == clean[0].tobytes() and int(want[6][3]) == 2 and want[6][[0, 1, 2, 4]].tolist() == clean[6][[0, 1, 2, 4]].tolist()
    K = len(want[0])
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    store.push(codes)
    qset = smafa_amd.QuerySet(store, reads)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(a.astype(np.int64)).to(dev).to(torch.int32)  # noqa: E731  (the uint32 bits)
    d_lineage, d_samples, d_weights = up(lineage.reshape(-1)), up(samples), up(weights)
    fresh = lambda count, dtype=torch.int32: torch.full((count,), 5, dtype=dtype, device=dev)  # noqa: E731
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731

    def launch(cap, entries, per_read=True):
        outs = [fresh(m) for _ in range(5)]
        totals = fresh(6, torch.int64)
        torch.cuda.synchronize()
        store.classify_launch(qset, D, slack, d_lineage.data_ptr(), R, d_samples.data_ptr(), 3, d_weights.data_ptr(),
                              *[o.data_ptr() if per_read else 0 for o in outs], entries.data_ptr() if entries is not None else 0, cap,
                              totals.data_ptr())
        store.sync()
        return outs, totals

    # every output, with room for two entries more than the table has: those are zeroed (the header says so), nothing behind them
    entries = fresh(2 * (K + 4), torch.int64)
    outs, totals = launch(K + 2, entries)
    got = entries.cpu().numpy().view(TABLE_DTYPE)
    assert got[:K].tobytes() == want[0].tobytes()
    assert (entries.cpu().numpy()[2 * K: 2 * (K + 2)] == 0).all() and (entries.cpu().numpy()[2 * (K + 2):] == 5).all()
    for name, o, w in zip(("subject", "dist", "taxon", "depth", "ties"), outs, want[1:6]):
        assert u32(o).tobytes() == w.tobytes(), name
    assert u64(totals).tobytes() == want[6].tobytes()
    assert store.last_call_kernels()[-6:] == CLASSIFY_KERNELS
    # cap = 0 with NULL entries: counted only; the optional outputs left out are not written
    outs, totals = launch(0, None, per_read=False)
    assert u64(totals).tobytes() == want[6].tobytes()
    assert all(bool((o == 5).all()) for o in outs)
    # half the capacity: the first half in table order, the exact count, nothing behind it
    half = K // 2
    entries = fresh(2 * K, torch.int64)
    _, totals = launch(half, entries)
    assert int(u64(totals)[0]) == K and u64(totals).tobytes() == want[6].tobytes()
    assert entries.cpu().numpy().view(TABLE_DTYPE)[:half].tobytes() == want[0][:half].tobytes()
    assert (entries.cpu().numpy()[2 * half:] == 5).all()
    qset.close()
    store.close()
    print("classify device form ok")


if __name__ == "__main__":
    main()
