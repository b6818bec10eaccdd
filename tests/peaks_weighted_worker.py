"""Worker for tests/test_gpu_peaks_weighted.py::test_device_form.

smafa_db_self_peaks_weighted_launch on torch buffers: the weights are read from HBM and the labels, parents, weights and the peak
count stay there; everything must equal the model of tests/peaks_weighted_cases.py, the raw store's peaks must be the lifted
ones, and nothing may be written past the arrays.  torch supplies the device buffers (as bench.py does) and is imported first."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
torch.cuda.init()

import smafa_amd  # noqa: E402
from peaks_weighted_cases import brute_weighted_peaks, expected_derep, identity_store, lifted  # noqa: E402


def u32(t, count):
    return t[:count].cpu().numpy().view(np.uint32)


def main():
    D = 3
    for kind, alphabet in (("nt", 0), ("aa", 1)):
        codes = identity_store(kind)
        derep = expected_derep(codes)
        U = len(derep[1])
        raw = smafa_amd.SubjectStore(60, alphabet)
        raw.push(codes)
        uniques = smafa_amd.SubjectStore(60, alphabet)
        uniques.push(np.ascontiguousarray(codes[derep[1]]))
        d_sizes = torch.from_numpy(derep[2].view(np.int32).copy()).cuda()
        d_labels, d_parents, d_weights = (torch.full((U + 64,), -2, dtype=torch.int32, device="cuda") for _ in range(3))
        d_count = torch.full((2,), -2, dtype=torch.int64, device="cuda")
        model = brute_weighted_peaks(codes[derep[1]], D, 0, derep[2])
        for with_parents, with_weights in ((True, True), (False, False)):
            for t in (d_labels, d_parents, d_weights):
                t.fill_(-2)
            uniques.self_peaks_weighted_launch(D, 0, d_sizes.data_ptr(), d_labels.data_ptr(), d_parents.data_ptr() if with_parents else 0,
                                               d_weights.data_ptr() if with_weights else 0, d_count.data_ptr())
            uniques.sync()
            assert u32(d_labels, U).tobytes() == model[0].tobytes() and d_count.tolist() == [model[3], -2]
            if with_parents:
                assert u32(d_parents, U).tobytes() == model[1].tobytes() and u32(d_weights, U).tobytes() == model[2].tobytes()
            else:
                assert int((d_parents != -2).sum().item()) == 0 and int((d_weights != -2).sum().item()) == 0
            for t in (d_labels, d_parents, d_weights):
                assert int((t[U:] != -2).sum().item()) == 0  # nothing past them
        assert u32(d_sizes, U).tobytes() == derep[2].tobytes()  # the weights are read, not written
        assert not lifted(raw.self_peaks(D, 0), derep, (u32(d_labels, U), None, model[2], model[3]))
        # a missing argument is refused and nothing is written
        d_labels.fill_(-2)
        for bad in ((0, d_labels.data_ptr(), d_count.data_ptr()), (d_sizes.data_ptr(), 0, d_count.data_ptr()),
                    (d_sizes.data_ptr(), d_labels.data_ptr(), 0)):
            try:
                uniques.self_peaks_weighted_launch(D, 0, bad[0], bad[1], 0, 0, bad[2])
            except smafa_amd.SmafaError as e:
                assert e.code == -1 and "smafa_db_self_peaks_weighted_launch: NULL" in str(e), e
            else:
                raise AssertionError("a NULL argument was accepted")
        torch.cuda.synchronize()
        assert int((d_labels != -2).sum().item()) == 0
        uniques.close()
        raw.close()
    print("weighted peaks device form ok")


if __name__ == "__main__":
    main()
