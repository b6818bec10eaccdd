"""smafa_db_consensus_launch on torch device buffers (run by tests/test_gpu_consensus.py::test_device_form and
tests/test_consensus_abi.py in a process of its own: torch initialises HIP first).  The bytes must be the host form's and the model's;
a capacity below K writes nothing and reports K."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import smafa_amd  # noqa: E402
from smafa_amd import _lib  # noqa: E402
from consensus_cases import check_consensus, chunk_case  # noqa: E402


def main():
    codes, labellings = chunk_case()
    labels = labellings["random"]
    n, L = codes.shape
    store = smafa_amd.SubjectStore(L, smafa_amd.ALPHABET_NT)
    store.push(codes)
    host = store.cluster_consensus(labels)
    K = check_consensus(codes, labels, host)
    dev = torch.device("cuda:0")
    d_labels = torch.from_numpy(labels.astype(np.int64)).to(dev).to(torch.int32)  # (the uint32 bits, NONE = -1)
    fresh = lambda count, dtype=torch.int32: torch.full((count,), 5, dtype=dtype, device=dev)  # noqa: E731
    ids, sizes, nearest, div, cons = fresh(K), fresh(K), fresh(K), fresh(n), fresh(K * L, torch.uint8)
    torch.cuda.synchronize()
    refused = ((ids.data_ptr(), sizes.data_ptr(), cons.data_ptr(), nearest.data_ptr(), div.data_ptr(), K - 1), (0, 0, 0, 0, 0, 0))
    for args in refused:  # a capacity below K, and the way to ask for K
        try:
            store.cluster_consensus_launch(d_labels.data_ptr(), *args)
            raise AssertionError("a capacity below K was accepted")
        except smafa_amd.SmafaError as e:
            assert e.code == _lib.ERR_CAPACITY and e.count == K, (e.code, str(e))
        for t in (ids, sizes, nearest, div, cons):
            assert bool((t == 5).all()), "a refused call wrote to an output"
    assert store.cluster_consensus_launch(d_labels.data_ptr(), ids.data_ptr(), sizes.data_ptr(), cons.data_ptr(), nearest.data_ptr(),
                                          div.data_ptr(), K) == K
    got = (ids.cpu().numpy().view(np.uint32), sizes.cpu().numpy().view(np.uint32), cons.cpu().numpy().reshape(K, L),
           nearest.cpu().numpy().view(np.uint32), div.cpu().numpy().view(np.uint32))
    assert all(g.tobytes() == h.tobytes() for g, h in zip(got, host))
    # the optional outputs left out
    ids2, sizes2, cons2 = fresh(K), fresh(K), fresh(K * L, torch.uint8)
    assert store.cluster_consensus_launch(d_labels.data_ptr(), ids2.data_ptr(), sizes2.data_ptr(), cons2.data_ptr(), 0, 0, K) == K
    assert torch.equal(ids2, ids) and torch.equal(sizes2, sizes) and torch.equal(cons2, cons)
    store.close()
    print("consensus device form ok")


if __name__ == "__main__":
    main()
