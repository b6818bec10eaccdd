"""smafa_db_self_chimeras_launch on torch device buffers (run by tests/test_chimera_abi.py in a process of its own: torch
initialises HIP first).  The bytes must be the host form's and the model's, with counted weights and with weights given on the
device; optional outputs left out stay untouched."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import smafa_amd  # noqa: E402
from chimera_cases import STORES, brute_chimeras, expected, planted  # noqa: E402

FIELDS = ("flags", "left_parent", "left_len", "right_parent", "right_len", "weights")


def main():
    key, D, F = "nt60", 3, 2
    codes = planted(key)[0]
    n, L = codes.shape
    store = smafa_amd.SubjectStore(L, smafa_amd.ALPHABET_NT)
    store.push(codes)
    want = expected(key, D, 0, F)
    host = store.self_chimeras(D, F, 0)
    assert all(getattr(host, f).tobytes() == getattr(want, f).tobytes() for f in FIELDS) and host.n_chimeras == want.n_chimeras
    dev = torch.device("cuda:0")
    fresh = lambda: torch.full((n,), 5, dtype=torch.int32, device=dev)  # noqa: E731
    out = [fresh() for _ in range(6)]
    count = torch.full((1,), 9, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    store.self_chimeras_launch(D, 0, F, 0, *(t.data_ptr() for t in out), count.data_ptr())
    store.sync()
    assert int(count.item()) == want.n_chimeras
    for t, f in zip(out, FIELDS):
        assert t.cpu().numpy().view(np.uint32).tobytes() == getattr(want, f).tobytes(), f
    # weights given on the device, the optional outputs left out: flags and the count alone are written
    given = want.weights.copy()
    given[::3] = 0
    model = brute_chimeras(codes, D, 0, F, given)
    d_given = torch.from_numpy(given.astype(np.int64)).to(dev).to(torch.int32)
    flags, idle = fresh(), fresh()
    torch.cuda.synchronize()
    store.self_chimeras_launch(D, 0, F, d_given.data_ptr(), flags.data_ptr(), 0, 0, 0, 0, 0, count.data_ptr())
    store.sync()
    assert int(count.item()) == model.n_chimeras and flags.cpu().numpy().view(np.uint32).tobytes() == model.flags.tobytes()
    assert bool((idle == 5).all()) and d_given.cpu().numpy().view(np.uint32).tobytes() == given.tobytes()
    assert STORES[key][2] == L
    store.close()
    print("chimeras device form ok")


if __name__ == "__main__":
    main()
