"""The subset of a resident store and its sequences back (smafa_db_subset, smafa_db_rows) against the numpy model of
tests/subset_cases.py: rows() returns the bytes push() was given, the subset under a mask holds codes[mask] and answers every call
as a fresh store of those rows does.  The expected rows of the scans come from the oracle's brute force."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import oracle
import smafa_amd
from smafa_amd import _lib
from self_join_cases import replaned_case
from kernel_namespaces import NAMESPACES
from subset_cases import (KINDS, LENGTHS, MASKS, PLANES, SIZES, SUBSET_CALL, DeviceArray, expected_subset, keep_mask, make_store,
                          random_codes, two_family_case)

SUBSET_KERNELS = NAMESPACES["subset::"]

pytestmark = pytest.mark.gpu


def check_subset(store, codes, keep, invert=False):
    """the subset under `keep` (a drop list where invert) equals the model; -> the subset"""
    want, old = expected_subset(codes, ~np.asarray(keep, dtype=bool) if invert else keep)
    sub, old_of_new = store.subset(keep, invert=invert)
    assert len(sub) == len(want) and old_of_new.tobytes() == old.tobytes()
    assert sub.info().planes == store.info().planes
    assert sub.rows().tobytes() == want.tobytes()
    return sub


# ---- rows round trip
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_rows_return_the_pushed_codes(kind, L):
    for n in SIZES:
        codes = random_codes(kind, L, n)
        store = make_store(kind, L, codes)
        assert store.info().planes == PLANES[kind]
        assert store.rows().tobytes() == codes.tobytes(), n
        store.close()


@pytest.mark.parametrize("kind", KINDS)
def test_rows_listed_ranged_and_none(kind):
    L, n = 33, 5000
    codes = random_codes(kind, L, n)
    store = make_store(kind, L, codes)
    rng = np.random.default_rng(4)
    listed = np.concatenate([np.arange(n - 1, n - 300, -1), rng.integers(0, n, size=200), [7, 7, 7, 0, n - 1]]).astype(np.uint32)  # descending, repeats
    assert store.rows(listed).tobytes() == codes[listed].tobytes()
    assert store.rows(first=300, count=1000).tobytes() == codes[300:1300].tobytes()  # a range that starts mid-tile
    assert store.rows(first=4999).tobytes() == codes[4999:].tobytes()
    assert store.rows(first=n).shape == (0, L) and store.rows(np.zeros(0, dtype=np.uint32)).shape == (0, L)  # m == 0
    before = store.last_call_kernels()
    assert _lib.lib().smafa_db_rows(store._h, None, 0, 0, None) == _lib.OK and store.last_call_kernels() == before  # ... touches nothing
    # the host form names the entry it refuses; a range past the end is refused
    bad = np.array([1, 2, n, 3], dtype=np.uint32)
    with pytest.raises(smafa_amd.SmafaError, match=r"smafa_db_rows: subjects\[2\] is 5000, the store has 5000 subjects"):
        store.rows(bad)
    with pytest.raises(smafa_amd.SmafaError, match="rows 4000 .. 5000, the store has 5000 subjects"):
        store.rows(first=4000, count=1001)
    # the launch form: one number out of range gives a row of 0xff, its neighbours stay intact, the guard bytes behind too
    d_list, d_out = DeviceArray(bad), DeviceArray(np.full((5, L), 0x55, dtype=np.uint8))
    store.rows_launch(d_list.ptr, 0, 4, d_out.ptr)
    got = d_out.get()
    assert got[:2].tobytes() == codes[[1, 2]].tobytes() and (got[2] == 0xff).all() and got[3].tobytes() == codes[3].tobytes() and (got[4] == 0x55).all()
    store.rows_launch(0, 4094, 4, d_out.ptr)  # the range form, across a tile edge
    assert d_out.get()[:4].tobytes() == codes[4094:4098].tobytes()
    d_list.free(), d_out.free()
    store.close()


# ---- the subset equals the model
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_subset_equals_the_model(kind, L):
    for n in SIZES:
        codes = random_codes(kind, L, n)
        store = make_store(kind, L, codes)
        for name in MASKS:
            check_subset(store, codes, keep_mask(name, n)).close()
        check_subset(store, codes, keep_mask("random10", n), invert=True).close()
        check_subset(store, codes, keep_mask("random90", n).astype(np.int64) * 7).close()  # integers: non-zero keeps
        store.close()


def test_subset_launch_form():
    kind, L, n = "aa", 60, 5000
    codes = random_codes(kind, L, n)
    store = make_store(kind, L, codes)
    keep = keep_mask("random90", n)
    want, old = expected_subset(codes, keep)
    d_keep, d_old = DeviceArray(keep.astype(np.uint32)), DeviceArray(np.full(n, 9, dtype=np.uint32))
    sub, k = store.subset_launch(d_keep.ptr, False, d_old.ptr)
    assert k == len(want) == len(sub) and sub.rows().tobytes() == want.tobytes()
    got = d_old.get()
    assert got[:k].tobytes() == old.tobytes() and (got[k:] == 9).all()
    sub.close()
    sub, k = store.subset_launch(d_keep.ptr, True)  # the same array as a drop list, old_of_new not wanted
    assert k == n - len(want) and sub.rows().tobytes() == codes[~keep].tobytes()
    sub.close()
    d_keep.free(), d_old.free()
    # the host form's capacity protocol: the count alone, no store
    l = _lib.lib()
    out, kept = C.c_void_p(5), C.c_uint64(0)
    k32, room = keep.astype(np.uint32), np.full(n, 9, dtype=np.uint32)
    assert l.smafa_db_subset(store._h, k32.ctypes.data, 0, C.byref(out), room.ctypes.data, len(want) - 1, C.byref(kept)) == _lib.ERR_CAPACITY
    assert out.value is None and kept.value == len(want) and (room == 9).all()
    assert b"old_of_new too small: %d rows kept, capacity %d" % (len(want), len(want) - 1) in l.smafa_last_error()
    assert store.scan(codes[:3], 0).tobytes() == oracle.scan_codes(codes, codes[:3], 0).tobytes()  # the source goes on as before
    store.close()


def test_empty_source_and_empty_result():
    store = smafa_amd.SubjectStore(60, smafa_amd.ALPHABET_AA)
    sub, old = store.subset(np.zeros(0, dtype=bool))  # n == 0: keep == NULL is accepted
    assert len(sub) == 0 and len(old) == 0 and sub.rows().shape == (0, 60)
    codes = random_codes("aa", 60, 257)
    sub.push(codes)
    assert sub.rows().tobytes() == codes.tobytes()
    none, old = sub.subset(np.zeros(257, dtype=bool))
    assert len(none) == 0 and len(old) == 0 and none.scan(codes[:2], 3).shape == (0,)
    none.push(codes[:100])  # the layout is the source's: rows pushed later unpack as they went in
    assert none.rows().tobytes() == codes[:100].tobytes() and none.scan(codes[:5], 0).tobytes() == oracle.scan_codes(codes[:100], codes[:5], 0).tobytes()
    for s in (store, sub, none):
        s.close()


# ---- the zone words are the subset's own
def test_zone_words_are_the_subsets_own():
    codes, family, queries = two_family_case()
    store = make_store("aa", 60, codes)
    every_second = keep_mask("every_second", len(codes))  # (the store is sorted: every new tile spans two old ones)
    first, _ = store.subset(every_second)
    kept = codes[every_second]
    for sub, rows in ((first, kept), (first.subset(family[every_second] != 0)[0], kept[family[every_second] != 0])):
        want = oracle.scan_codes(rows, queries, 3)
        assert len(want) >= 100
        sub.set_zone_level(2)
        zoned = sub.scan(queries, 3)
        assert sub.last_scan_kernel().startswith("smafa::scan_zone_kernel"), sub.last_scan_kernel()
        sub.set_zone_level(0)
        plain = sub.scan(queries, 3)
        assert "zone" not in sub.last_scan_kernel()
        sub.set_prefilter(False)
        unfiltered = sub.scan(queries, 3)
        assert zoned.tobytes() == plain.tobytes() == unfiltered.tobytes() == want.tobytes()
        sub.close()
    store.close()


# ---- the result behaves as a fresh store
def same_answers(sub, fresh, queries, D):
    for a in (lambda s: s.scan(queries, D), lambda s: s.scan(queries, max_num_hits=1), lambda s: s.scan(queries, D, max_num_hits=2),
              lambda s: s.get_distances(queries[0]), lambda s: s.self_pairs(D), lambda s: s.self_components(D)[0]):
        x, y = a(sub), a(fresh)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("kind,L", [("aa", 60), ("nt3", 130), ("nt2", 31)])
def test_the_result_behaves_as_a_fresh_store(kind, L):
    from self_join_cases import planted_store

    codes = planted_store(11, "aa" if kind == "aa" else "nt", L, 450, n_frac=0.01 if kind == "nt3" else 0.0)  # 4 520 rows: a sorted append
    keep = keep_mask("random90", len(codes))
    store = make_store(kind, L, codes)
    sub = check_subset(store, codes, keep)
    fresh = make_store(kind, L, codes[keep])
    same_answers(sub, fresh, codes[keep][::40], 3)
    for s in (store, sub, fresh):
        s.close()


# ---- store states
def test_a_source_of_several_appends(monkeypatch):
    monkeypatch.setenv("SMAFA_RESORT", "0")  # the patchwork stays one: runs of 100, 4096 (sorted), 900 (from mid-tile), 4
    codes = random_codes("aa", 60, 5100, seed=1)
    store = make_store("aa", 60, pieces=[codes[:100], codes[100:4196], codes[4196:5096], codes[5096:]])
    for name in ("every_second", "random10", "last_tile", "first"):
        keep = keep_mask(name, 5100)
        sub = check_subset(store, codes, keep)
        assert sub.scan(codes[:50], 2).tobytes() == oracle.scan_codes(codes[keep], codes[:50], 2).tobytes()
        sub.close()
    store.close()


def test_a_source_after_a_resort(monkeypatch):
    monkeypatch.setenv("SMAFA_RESORT_MIN", "64")
    codes = random_codes("nt3", 65, 5000, seed=2)
    store = make_store("nt3", 65, pieces=[codes[:3000], codes[3000:]])
    assert len(store.scan(codes[:4], 0)) >= 4  # the scan that sorts the store again
    keep = keep_mask("random90", 5000)
    sub = check_subset(store, codes, keep)
    assert sub.scan(codes[:50], 3).tobytes() == oracle.scan_codes(codes[keep], codes[:50], 3).tobytes()
    assert store.rows().tobytes() == codes.tobytes()
    sub.close(), store.close()


def test_an_unsorted_source(monkeypatch):
    monkeypatch.setenv("SMAFA_SORT", "0")
    codes = random_codes("aa", 64, 5000)
    store = make_store("aa", 64, codes)
    check_subset(store, codes, keep_mask("every_second", 5000)).close()
    store.close()


def test_a_replaned_source():
    pieces, _ = replaned_case()
    codes = np.concatenate(pieces)
    store = make_store("nt3", 330, pieces=pieces)
    assert store.info().planes == 3 and store.rows().tobytes() == codes.tobytes()
    check_subset(store, codes, keep_mask("random90", len(codes))).close()
    store.close()


def test_three_planes_stay_when_every_n_row_is_dropped():
    codes = random_codes("nt2", 60, 4096).copy()
    codes[::10, 7] = 4  # an N in every tenth row
    has_n = (codes == 4).any(axis=1)
    assert has_n.any() and not has_n.all()
    store = make_store("nt3", 60, codes)
    sub = check_subset(store, codes, has_n, invert=True)
    assert sub.info().planes == 3 and sub.rows().max() == 3
    assert sub.scan(codes[:50], 4).tobytes() == oracle.scan_codes(codes[~has_n], codes[:50], 4).tobytes()
    sub.close(), store.close()


# ---- life after
def test_life_after(monkeypatch, tmp_path):
    monkeypatch.setenv("SMAFA_RESORT_MIN", "64")
    codes = random_codes("aa", 60, 5000, seed=5)
    store = make_store("aa", 60, codes)
    keep = keep_mask("random90", 5000)
    sub = check_subset(store, codes, keep)
    rows = codes[keep]
    # a subset of a subset
    keep2 = keep_mask("every_second", len(rows))
    sub2 = check_subset(sub, rows, keep2)
    # push onto a subset, then scan: the rows pushed make up more than a quarter, so the scan sorts the store again
    more = random_codes("aa", 60, 4095, seed=6)
    sub2.push(more)
    both = np.concatenate([rows[keep2], more])
    assert sub2.scan(both[::50], 3).tobytes() == oracle.scan_codes(both, both[::50], 3).tobytes()
    assert sub2.rows().tobytes() == both.tobytes()
    # an index built on a subset answers as its scan kernels do
    queries = rows[::20]
    want = oracle.scan_codes(rows, queries, 3)
    assert sub.scan(queries, 3).tobytes() == want.tobytes()
    info = sub.build_index(3)
    assert info["current"] and sub.scan(queries, 3).tobytes() == want.tobytes()
    # save, load, rows
    path = str(tmp_path / "sub.db")
    sub.save(path)
    back = smafa_amd.SubjectStore.load(path)
    assert back.rows().tobytes() == rows.tobytes() and back.scan(queries, 3).tobytes() == want.tobytes()
    for s in (store, sub, sub2, back):
        s.close()


# ---- the source is untouched
def test_the_source_is_untouched(tmp_path):
    codes = random_codes("aa", 60, 5000, seed=7)
    store = make_store("aa", 60, codes)
    queries = codes[::25]
    info = store.build_index(3)
    assert info["current"]
    rows_before, scan_before = store.rows(), store.scan(queries, 3)
    keep = keep_mask("random90", 5000)
    files = []
    for name in ("a.db", "b.db"):
        sub, _ = store.subset(keep)
        files.append(str(tmp_path / name))
        sub.save(files[-1])
        sub.close()
    assert open(files[0], "rb").read() == open(files[1], "rb").read()  # the same mask twice: the same store, byte for byte
    after = store.index_info()
    assert after["current"] and after["blocks"] == info["blocks"]
    assert store.rows().tobytes() == rows_before.tobytes() == codes.tobytes()
    assert store.scan(queries, 3).tobytes() == scan_before.tobytes() == oracle.scan_codes(codes, queries, 3).tobytes()
    store.close()


# ---- kernels by name
def test_kernels_by_name():
    """subset::keep_flags_kernel, subset::run_ends_kernel, subset::move_rows_kernel and smafa::zone_kernel behind a subset;
    subset::unpack_rows_kernel<P> behind rows — with smafa_join::inverse_order_kernel in front of it the first time only"""
    seen = set()
    for kind in KINDS:
        codes = random_codes(kind, 60, 4096)
        store = make_store(kind, 60, codes)
        sub, _ = store.subset(keep_mask("every_second", 4096))
        assert store.last_call_kernels() == SUBSET_CALL
        stats = store.last_call_stats()
        assert stats["kernel_ms"] > 0 and stats["launches"] == 6 and store.last_scan_ms()[0] == pytest.approx(stats["kernel_ms"])
        unpack = "subset::unpack_rows_kernel<%d>" % PLANES[kind]
        store.rows()
        assert store.last_call_kernels() == ["smafa_join::inverse_order_kernel", unpack]
        store.rows(first=5, count=9)
        assert store.last_call_kernels() == [unpack] and store.last_call_stats()["launches"] == 1
        seen |= set(SUBSET_CALL[:3]) | {unpack}
        sub.close(), store.close()
    assert seen == set(SUBSET_KERNELS)


# ---- the verb
def run_cli(*args, stdin=None):
    return subprocess.run([_lib.CLI_PATH, *args], input=stdin, capture_output=True)


def test_the_verb(golden, tmp_path):
    fa = golden + "/subjects.fa"
    records = open(fa).read().split(">")[1:]
    n = len(records)
    drop = sorted({1, n - 1, n // 2})
    kept = [i for i in range(n) if i not in drop]
    kept_fa, db, sub_db, kept_db = (str(tmp_path / f) for f in ("kept.fa", "all.db", "sub.db", "kept.db"))
    open(kept_fa, "w").write("".join(">" + records[i] for i in kept))
    assert run_cli("makedb", "-i", fa, "-d", db).returncode == 0 and run_cli("makedb", "-i", kept_fa, "-d", kept_db).returncode == 0
    listed = "".join("%d\t1\tsome\tcolumns\n" % i for i in drop + drop[:1]).encode()  # further columns, a duplicate
    (tmp_path / "drop.tsv").write_bytes(listed)
    r = run_cli("subset", "-d", db, "--drop", str(tmp_path / "drop.tsv"), "--output", sub_db)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "".join("%d\t%d\n" % (new, old) for new, old in enumerate(kept)).encode()
    assert b"%d of %d sequences kept" % (len(kept), n) in r.stderr
    want = run_cli("query", "-d", kept_db, "-q", fa, "--max-divergence", "5")
    got = run_cli("query", "-d", sub_db, "-q", fa, "--max-divergence", "5")
    assert want.returncode == 0 and got.returncode == 0 and want.stdout and got.stdout == want.stdout
    # --keep - reads stdin; the result is the same store
    r = run_cli("subset", "-d", db, "--keep", "-", "--output", str(tmp_path / "keep.db"), stdin="".join("%d\n" % i for i in reversed(kept)).encode())
    assert r.returncode == 0 and r.stdout == "".join("%d\t%d\n" % (new, old) for new, old in enumerate(kept)).encode()
    assert (tmp_path / "keep.db").read_bytes() == (tmp_path / "sub.db").read_bytes()
    assert run_cli("pairs", "-d", sub_db, "--max-divergence", "2").returncode == 0  # another verb reads it
    # the refusals
    for args, stdin, code, text in (
            (("--keep", "-", "--drop", "x"), b"", 2, b"--keep and --drop exclude each other"),
            ((), b"", 2, b"subset needs --keep or --drop"),
            (("--keep", "-"), b"0\n%d\n" % n, 1, b"smafa_subset: list line 2: the database has no sequence of that number"),
            (("--keep", "-"), b"0\nx\n", 1, b"smafa_subset: list line 2: no sequence number"),
            (("--keep", "-"), b"0\n1x\n", 1, b"smafa_subset: list line 2: the sequence number is not a number"),
            (("--drop", str(tmp_path / "nothing")), b"", 1, b"cannot open list file")):
        r = run_cli("subset", "-d", db, *args, "--output", str(tmp_path / "refused.db"), stdin=stdin)
        assert r.returncode == code and text in r.stderr and r.stdout == b"", (args, r.stderr)
        assert not (tmp_path / "refused.db").exists()
    r = run_cli("subset", "-d", db, "--keep", "-")
    assert r.returncode == 2 and b"subset needs --database and --output" in r.stderr
