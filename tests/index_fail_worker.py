"""An automatic build of the block index that fails (tests/test_gpu_index_auto.py runs this in a process of its own and reads
its stderr): `python index_fail_worker.py aa|nt2`.

SMAFA_INDEX_FAIL_BUILDS=1 makes the handle's next index_build fail where a store too big for the remaining HBM does — a
hipMalloc of its sort keys that returns out of memory.  That is not the scan's failure: the scan kernels answer with the
oracle's rows, nothing of the index stays allocated, the engine says "block index not built" once (verbosity 1) and does not
try again until the store changes.  Six cases, each on a handle of its own, each announced on stderr ("== case x") so that
the engine's lines can be counted per case; a case that fails is reported on stdout and the others still run."""
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import oracle
import smafa_amd
from self_join_cases import brute_pairs, planted_store
from smafa_amd import _lib
from test_gpu_layout import expected_with_k, queries_from

N, NQ, L, D = 20000, 300, 60, 3
TILE = 100  # mode 3: the batch is the NQ queries TILE times over, so that the rent reaches the build's price within a few calls


def make(kind, mode, fail, rows):
    env = {"SMAFA_INDEX": str(mode), "SMAFA_INDEX_MIN_ROWS": "1", "SMAFA_INDEX_MAX_RUN": "100000000", "SMAFA_INDEX_CAND": "100",
           "SMAFA_INDEX_FAIL_BUILDS": str(fail)}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)  # read when a handle is created
    try:
        store = smafa_amd.SubjectStore(rows.shape[1], 1 if kind == "aa" else 0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    store.push(rows)
    return store


def tiled(want, times, nq):
    out = np.tile(want, times)
    out["query"] += np.repeat(np.arange(times, dtype=np.uint32) * nq, len(want))
    return out


def main(kind):
    letters = 20 if kind == "aa" else 4
    planes_words = (5 if kind == "aa" else 2) * 2
    rng = np.random.default_rng(41 + letters)
    s = rng.integers(0, letters, size=(N, L), dtype=np.uint8)
    more = rng.integers(0, letters, size=(N // 4, L), dtype=np.uint8)
    s[100:104] = s[99]
    both = np.concatenate([s, more])
    q = queries_from(rng, both, NQ, letters, D + 2)
    want, want_both = oracle.scan_codes(s, q, D), oracle.scan_codes(both, q, D)
    assert len(want) > NQ // 4
    failed = []

    def case(name, fn):
        sys.stderr.write("== case %s\n" % name)
        sys.stderr.flush()
        try:
            fn()
            print("case %s ok" % name)
        except Exception as e:  # reported, and the next case still runs
            failed.append(name)
            print("case %s FAILED: %s: %s" % (name, type(e).__name__, e))
            traceback.print_exc(file=sys.stdout)
        sys.stdout.flush()
        sys.stderr.flush()

    def not_built(store):
        info = store.index_info()
        assert info["current"] == 0 and info["bytes"] == 0 and info["probe_launches"] == 0, info
        assert "index_probe" not in store.last_scan_kernel(), store.last_scan_kernel()

    held = {}

    def a():
        store = held["a"] = make(kind, 2, 1, s)
        for _ in range(3):  # the scan that was to build, then two more: no second attempt while the store is unchanged
            assert store.scan(q, max_divergence=D).tobytes() == want.tobytes()
            not_built(store)

    def b():
        store = held.pop("a")
        store.push(more)  # the store changed: the next eligible scan builds
        assert store.scan(q, max_divergence=D).tobytes() == want_both.tobytes()
        info = store.index_info()
        assert info["current"] == 1 and info["blocks"] == D + 1 and info["bytes"] > 0 and info["probe_launches"] == 1, info
        assert "index_probe" in store.last_scan_kernel(), store.last_scan_kernel()
        store.close()

    def c():
        store = make(kind, 3, 1, s)
        big, big_want = np.ascontiguousarray(np.tile(q, (TILE, 1))), tiled(want, TILE, NQ).tobytes()
        # rent or buy (kth_plan.h index_rent_charge / index_rent_due): 1.7e-12 ms per pair and stored vector against 0.3 ms + 1e-7 ms per block and subject
        due = int(np.ceil((0.3 + (D + 1) * N * 1.0e-7) / (NQ * TILE * N * planes_words * 1.7e-12)))
        assert 3 <= due < 200, due
        for call in range(due + 3):  # .. the call where the build comes due, and two more
            assert store.scan(big, max_divergence=D).tobytes() == big_want, call
            not_built(store)
        print("mode 3, fixed bound: build due at call %d" % due)
        store.close()

    def d():
        store = make(kind, 3, 1, s)
        full = oracle.scan_codes(s, q, L)
        best = expected_with_k(full, 1).tobytes()
        # (calls without a bound: 1.6e-11 ms per pair and stored vector against 0.3 ms + 1e-7 ms x 32 blocks at the most)
        due = int(np.ceil((0.3 + 32 * N * 1.0e-7) / (NQ * N * planes_words * 1.6e-11)))
        assert 3 <= due < 1000, due
        for call in range(due + 3):
            assert store.scan(q, max_num_hits=1).tobytes() == best, call
            assert store.index_info()["current"] == 0 and store.index_info()["bytes"] == 0 and store.index_info()["probe_launches"] == 0
        print("mode 3, no bound: build due by call %d" % due)
        store.close()

    def e():
        store = make(kind, 1, 1, s)
        try:
            store.build_index(D)
            raise AssertionError("build_index succeeded")
        except smafa_amd.SmafaError as err:
            print("build_index: SmafaError %d: %s" % (err.code, err))
        assert store.scan(q, max_divergence=D).tobytes() == want.tobytes()
        not_built(store)
        info = store.build_index(D)
        assert info["current"] == 1 and info["blocks"] == D + 1, info
        assert store.scan(q, max_divergence=D).tobytes() == want.tobytes()
        assert "index_probe" in store.last_scan_kernel()
        store.close()

    def f():
        codes = planted_store(7, "aa" if kind == "aa" else "nt", L, 300)
        store = make(kind, 2, 1, codes)
        assert store.self_pairs(D, first_cap=1 << 20).tobytes() == brute_pairs(codes, D).tobytes()
        info = store.index_info()
        assert info["current"] == 0 and info["bytes"] == 0 and info["probe_launches"] == 0, info
        store.close()

    for name, fn in (("a", a), ("b", b), ("c", c), ("d", d), ("e", e), ("f", f)):
        if name == "b" and "a" not in held:
            failed.append("b")
            print("case b FAILED: no handle from case a")
            continue
        case(name, fn)
    sys.stderr.write("== end\n")
    if failed:
        print("failed cases: %s" % " ".join(failed))
        return 1
    print("index fail worker ok: %s" % kind)
    return 0


if __name__ == "__main__":
    _lib.lib().smafa_set_verbosity(1)
    sys.exit(main(sys.argv[1]))
