"""The self-join of a resident store (smafa_db_self_hits / smafa_db_self_launch / `smafa pairs`): every unordered pair of
the store's own subjects within a bound, exactly once, rows {min, max, dist} ordered (query, dist, subject).

Expected rows are brute force on the code bytes (tests/self_join_cases.py), checked against oracle.scan_codes on a sample;
nothing here is expected from the code under test.  The file takes 38 s on an MI355X (25 s of it the 1M-row case)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib, synth
from self_join_cases import SHAPES, brute_pairs, check_against_oracle, planted_store

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def case(name, families):
    """-> (codes, expected rows, D) of a shape of SHAPES at `families` x 10 + 20 rows"""
    _, kind, L, D, n_frac = next(s for s in SHAPES if s[0] == name)
    codes = planted_store(11 + families + len(name), kind, L, families, n_frac)
    want = brute_pairs(codes, D)
    check_against_oracle(codes, want, D)
    assert len(want) > 0 and (want["dist"] == 0).sum() >= 1, (name, len(want))
    if D > 0:
        assert set(np.unique(want["dist"])) == set(range(D + 1)), (name, np.unique(want["dist"]))
    return codes, want, D


def make_store(codes, kind):
    store = smafa_amd.SubjectStore(codes.shape[1], smafa_amd.ALPHABET_AA if kind == "aa" else smafa_amd.ALPHABET_NT)
    store.push(codes)
    return store


def kind_of(name):
    return next(s for s in SHAPES if s[0] == name)[1]


@pytest.mark.parametrize("families", [300, 2000])  # 3 020 rows: append order kept; 20 020 rows in one piece: sorted store
@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_self_pairs_equal_brute_force(name, families):
    codes, want, D = case(name, families)
    store = make_store(codes, kind_of(name))
    assert store.info().planes == {"nt60": 2, "nt60n": 3, "nt9": 2, "nt130": 2}.get(name, 5)
    got = store.self_pairs(D)
    print("%s x %d rows, D = %d: %d pairs, kernels %s" % (name, len(codes), D, len(want), store.last_call_kernels()))
    assert got.tobytes() == want.tobytes()
    store.close()


def test_every_pair_at_the_full_length():
    """D = L: all n(n-1)/2 rows"""
    codes = planted_store(3, "nt", 60, 28)  # 300 rows
    assert len(codes) == 300
    want = brute_pairs(codes, 60)
    assert len(want) == 300 * 299 // 2 and (want["dist"] == 0).sum() >= 1
    store = make_store(codes, "nt")
    assert store.self_pairs(60).tobytes() == want.tobytes()
    assert store.self_pairs(1000).tobytes() == want.tobytes()  # a bound above seq_len is allowed
    store.close()


def test_small_stores_and_bad_bounds():
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_NT)
    assert len(store.self_pairs(5)) == 0
    row = np.zeros((1, 60), dtype=np.uint8)
    store.push(row)
    assert len(store.self_pairs(5)) == 0
    store.push(row)
    got = store.self_pairs(0)
    assert got.tolist() == [(0, 1, 0)]
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_pairs(None)
    assert e.value.code == _lib.ERR_INVALID
    store.close()


@pytest.mark.parametrize("name", ["aa60", "nt60"])
def test_every_engine_one_answer(name, monkeypatch):
    codes, want, D = case(name, 2000)
    kind = kind_of(name)
    store = make_store(codes, kind)
    assert store.self_pairs(D, first_cap=1 << 20).tobytes() == want.tobytes()  # (room at once: the kernel list is this call's)
    # (which scan kernel the default takes is the engine's measured rule, zone_pays in scan_plan.h: at 20 020 rows and bound 5 the tiles share
    # too few filter bits for the zone level to pay and the filter-plane-resident kernel runs; the zone kernel is asserted by
    # name below at zone level 2, and as the default's own choice in test_default_takes_the_zone_kernel_where_it_pays)
    assert store.last_call_kernels()[0].startswith("smafa::scan_"), store.last_call_kernels()
    assert [k for k in store.last_call_kernels() if k.startswith("smafa_join::")] == [
        "smafa_join::store_records_kernel", "smafa_join::inverse_order_kernel", "smafa_join::join_filter_kernel"]
    stats = store.last_call_stats()
    assert stats["kernel_ms"] > 0 and stats["launches"] >= 4 and store.last_scan_ms()[0] == pytest.approx(stats["kernel_ms"])
    store.set_prefilter(False)
    assert store.self_pairs(D).tobytes() == want.tobytes()
    store.set_prefilter(True)
    for level in (0, 2, 1):
        store.set_zone_level(level)
        assert store.self_pairs(D, first_cap=1 << 20).tobytes() == want.tobytes(), level
        if level == 2:
            assert any("scan_zone_kernel" in k for k in store.last_call_kernels()), store.last_call_kernels()
    store.close()
    # a current block index answers the blocks.  (Families of ten near-identical rows share most of their column blocks:
    # at 20 020 rows the engine would leave them to the scan kernels, so the limit on expected candidates is lifted the way
    # tests/test_gpu_index.py lifts it — the path under test has to run.)
    monkeypatch.setenv("SMAFA_INDEX_CAND", "100")
    monkeypatch.setenv("SMAFA_INDEX_MAX_RUN", "100000000")
    store = make_store(codes, kind)
    info = store.build_index(D)
    store.set_index(1)
    assert info["max_div_served"] is not None and info["max_div_served"] >= D, info
    before = store.index_info()["probe_launches"]
    assert store.self_pairs(D, first_cap=1 << 20).tobytes() == want.tobytes()
    assert store.index_info()["probe_launches"] > before
    assert any("index_probe_kernel" in k for k in store.last_call_kernels())
    store.close()
    monkeypatch.delenv("SMAFA_INDEX_CAND")
    monkeypatch.delenv("SMAFA_INDEX_MAX_RUN")
    # the same rows appended in 40 pieces: unsorted runs, then the automatic re-sort in front of the join (stores of this
    # size are below the engine's default re-sort threshold: lowered for this handle)
    monkeypatch.setenv("SMAFA_RESORT_MIN", "4096")
    grown = smafa_amd.SubjectStore(codes.shape[1], smafa_amd.ALPHABET_AA if kind == "aa" else smafa_amd.ALPHABET_NT)
    cuts = np.linspace(0, len(codes), 41).astype(int)
    for a, b in zip(cuts[:-1], cuts[1:]):
        grown.push(codes[a:b])
    assert grown.self_pairs(D).tobytes() == want.tobytes()
    print("grown store:", grown.last_call_kernels())
    grown.close()


def test_default_takes_the_zone_kernel_where_it_pays():
    """the sorted 20 020-row store at bound 0: the engine's own choice is the zone kernel, and the join runs it"""
    codes, want, D = case("aa60d0", 2000)
    store = make_store(codes, "aa")
    assert store.self_pairs(D, first_cap=1 << 20).tobytes() == want.tobytes()
    assert any("scan_zone_kernel" in k for k in store.last_call_kernels()), store.last_call_kernels()
    store.close()


def test_device_form_and_capacity():
    """smafa_db_self_launch, and smafa_scan_each after a join (smafa_last_scan_ms is then that call's, not the join's totals)
    — tests/self_join_worker.py, a process of its own: the device buffers come from torch, which has to initialise HIP before
    the library does"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "self_join_worker.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "self-join device form ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


@pytest.mark.parametrize("ceiling", [None, "1000000"])
def test_dense_store_grows_buffer_and_scratch(ceiling, monkeypatch):
    """(ceiling: the scratch list may not grow past a million rows — the 4 000-row block is halved down to 512-row pieces, each
    scanned within the list as it is, and the piece size stays reduced while the pieces stay dense.)
    2 000 copies of one row + 2 000 of a second row at distance 3, D = 3: every one of the 4000 x 3999 / 2 pairs
    qualifies.  The one block's scan reports 16M rows — four times the scratch list — and the caller's first buffer holds 1000."""
    rng = np.random.default_rng(9)
    a = rng.integers(0, 4, size=60).astype(np.uint8)
    b = a.copy()
    b[[3, 30, 59]] = (b[[3, 30, 59]] + 1) % 4
    group = rng.permutation(np.repeat([0, 1], 2000))
    codes = np.where(group[:, None] == 0, a[None, :], b[None, :]).astype(np.uint8)
    i, j = np.triu_indices(4000, 1)
    d = np.where(group[i] == group[j], 0, 3)
    order = np.lexsort((j, d, i))
    want = np.zeros(len(i), dtype=smafa_amd.HIT_DTYPE)
    want["query"], want["subject"], want["dist"] = i[order], j[order], d[order]
    assert len(want) == 7_998_000
    if ceiling:
        monkeypatch.setenv("SMAFA_JOIN_SCRATCH_MAX", ceiling)
    store = make_store(codes, "nt")
    got = store.self_pairs(3, first_cap=1000)
    assert len(got) == 7_998_000 and got.tobytes() == want.tobytes()
    store.close()


def test_a_chunk_that_cannot_fit_fails_with_its_row_count(monkeypatch):
    """70 000 equal rows at bound 0: 64 of them have 4 480 000 rows within the bound, more than the scratch list holds and more
    than it may grow to here — the one case the join gives up on, saying how many rows it needed"""
    monkeypatch.setenv("SMAFA_JOIN_SCRATCH_MAX", "4096")
    monkeypatch.setenv("SMAFA_JOIN_BLOCK", "128")  # (small first pieces: the halving ends after one step)
    codes = np.zeros((70_000, 60), dtype=np.uint8)
    store = make_store(codes, "nt")
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_pairs(0)
    assert e.value.code == _lib.ERR_NOMEM and "4480000 rows" in str(e.value), str(e.value)
    store.close()


def test_against_the_query_path_at_scale():
    """1M x 60 aa in 10 000 families of 100, D = 5: per sampled row the join's neighbours are those of `scan` — the path the
    rest of the suite holds against the oracle — and the total is (rows of `scan` over all rows - n) / 2."""
    D = 5
    codes = synth.related_subjects(10_000, 100, div_lo=0.0, div_hi=0.08)
    n = len(codes)
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    store.push(codes)
    pairs = store.self_pairs(D, first_cap=1 << 25)
    assert any("scan_zone_kernel" in k for k in store.last_call_kernels()), store.last_call_kernels()  # the default's own choice here
    assert (pairs["query"] < pairs["subject"]).all()
    total = 0
    for lo in range(0, n, 65536):
        total += len(store.scan(codes[lo:lo + 65536], max_divergence=D))
    assert (total - n) % 2 == 0 and len(pairs) == (total - n) // 2
    rng = np.random.default_rng(2)
    sample = np.sort(rng.choice(n, size=200, replace=False))
    by_q = np.argsort(pairs["query"], kind="stable")
    by_s = np.argsort(pairs["subject"], kind="stable")
    q_sorted, s_sorted = pairs["query"][by_q], pairs["subject"][by_s]
    neighbours = 0
    for i in sample:
        lo = pairs[by_q[np.searchsorted(q_sorted, i):np.searchsorted(q_sorted, i, side="right")]]
        hi = pairs[by_s[np.searchsorted(s_sorted, i):np.searchsorted(s_sorted, i, side="right")]]
        mine = sorted([(int(r["subject"]), int(r["dist"])) for r in lo] + [(int(r["query"]), int(r["dist"])) for r in hi])
        ref = store.scan(codes[i:i + 1], max_divergence=D)
        want = sorted((int(r["subject"]), int(r["dist"])) for r in ref if r["subject"] != i)
        assert mine == want, i
        neighbours += len(mine)
    print("%d rows: %d pairs, %d neighbours over 200 sampled rows" % (n, len(pairs), neighbours))
    assert neighbours >= 200
    store.close()


def test_stale_state_after_push():
    codes, want, D = case("aa60", 2000)
    more = planted_store(77, "aa", 60, 498)  # 5 000 rows
    assert len(more) == 5000
    store = make_store(codes, "aa")
    store.build_index(D)
    assert store.self_pairs(D).tobytes() == want.tobytes()
    store.push(more)
    both = np.concatenate([codes, more])
    want2 = brute_pairs(both, D)
    assert len(want2) > len(want)
    assert store.self_pairs(D, first_cap=1 << 20).tobytes() == want2.tobytes()
    assert "smafa_join::inverse_order_kernel" in store.last_call_kernels()  # built again for the grown store
    store.close()


@pytest.mark.parametrize("kind,L,D", [("nt", 60, 5), ("aa", 60, 5)])
def test_cli_pairs(tmp_path, kind, L, D):
    codes = planted_store(21, kind, L, 300)
    want = brute_pairs(codes, D)
    assert len(want) > 0
    text = b"".join(b"%d\t%d\t%d\n" % (r["query"], r["subject"], r["dist"]) for r in want)
    fa, db, packed = (str(tmp_path / n) for n in ("s.fa", "s.db", "s.packed"))
    alphabet = 1 if kind == "aa" else 0
    synth.write_fasta(fa, codes, alphabet)
    flags = ["--alphabet", kind]
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", db, *flags], capture_output=True).returncode == 0
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", packed, "--packed", *flags], capture_output=True).returncode == 0
    for path in (db, packed):
        r = subprocess.run([_lib.CLI_PATH, "pairs", "-d", path, "--max-divergence", str(D)], capture_output=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout == text, path
    out = str(tmp_path / "pairs.tsv")
    with open(out, "wb") as f:
        smafa_amd.pairs(db, D, out_fd=f.fileno())
    assert open(out, "rb").read() == text
