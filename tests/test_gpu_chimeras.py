"""Chimera check of a resident store (smafa_db_self_chimeras / smafa_db_self_chimeras_launch / `smafa chimeras`): per row the
heavier row within the bound that shares its longest prefix, the one that shares its longest suffix, and the flag where the two
lengths cover the row.

All seven outputs are compared byte for byte with tests/chimera_cases.py::brute_chimeras, which works from brute-force pairs on
the code bytes and never from the code under test; tests/test_chimera_model.py holds that model to hand-worked values and every
planted store used here to its classes."""
import subprocess

import numpy as np
import pytest

import smafa_amd
from smafa_amd import _lib, synth
from chimera_cases import HAND, NONE, STORES, brute_chimeras, expected, packed_perm, planted
from peaks_cases import brute_peaks
from self_join_cases import replaned_case

pytestmark = pytest.mark.gpu
FIELDS = ("flags", "left_parent", "left_len", "right_parent", "right_len", "weights")
WEIGHED = ["smafa_pk::init_peaks_kernel", "smafa_pk::weigh_keep_kernel"]
OURS = ["chimera::init_sides_kernel", "chimera::offer_sides_kernel", "chimera::verdict_kernel"]
FULL = WEIGHED + OURS  # a call whose join kept a pair


def make_store(codes, kind):
    store = smafa_amd.SubjectStore(codes.shape[1], smafa_amd.ALPHABET_AA if kind == "aa" else smafa_amd.ALPHABET_NT)
    store.push(codes)
    return store


def store_of(key):
    return make_store(planted(key)[0], STORES[key][1])


def check(got, want, what=""):
    for name in FIELDS:
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == np.uint32 and g.shape == w.shape, (what, name)
        assert g.tobytes() == w.tobytes(), (what, name, np.flatnonzero(g != w)[:8], g[g != w][:8], w[g != w][:8])
    assert got.n_chimeras == want.n_chimeras, (what, got.n_chimeras, want.n_chimeras)


def our_kernels(store):
    return [k for k in store.last_call_kernels() if k.startswith(("smafa_pk::", "chimera::"))]


@pytest.mark.parametrize("key", ["nt60", "ntn60", "aa60"])
def test_planted_store_equals_brute_force(key):
    """2, 3 and 5 planes; D in {0, 3, 6, L}, F in {1, 2, 3}, radius 0, 1 and D"""
    L = STORES[key][2]
    store = store_of(key)
    assert store.info().planes == {"nt60": 2, "ntn60": 3, "aa60": 5}[key]
    flagged = {}
    for D in (0, 3, 6, L):
        for r in sorted({0, min(1, D), D}):
            for F in (1, 2, 3):
                want = expected(key, D, r, F)
                check(store.self_chimeras(D, F, r), want, (key, D, r, F))
                flagged[D, r, F] = want.n_chimeras
    check(store.self_chimeras(3, 2, None), expected(key, 3, 3, 2))  # radius None (SMAFA_NONE): r = D
    print("%s x %d rows: flagged rows by (D, r, F): %s" % (key, len(planted(key)[0]), flagged))
    assert flagged[3, 0, 2] >= 4 and flagged[3, 0, 1] > flagged[3, 0, 2] and flagged[6, 0, 2] > flagged[3, 0, 2] and flagged[0, 0, 1] == 0
    store.close()


def test_hand_worked_store():
    """the eight rows of tests/test_chimera_model.py: at D >= 6 rows 3, 4 and 7 have a parent of last resort — a row that shares no
    column with them, at length 0 on both sides, the smaller number"""
    store = make_store(HAND, "nt")
    for D in (3, 4, 6, 9):
        for F in (1, 2, 3):
            for r in (0, None):
                check(store.self_chimeras(D, F, r), brute_chimeras(HAND, D, r, F), (D, F, r))
    got = store.self_chimeras(6, 1, 0)
    assert [(int(got.left_parent[q]), int(got.left_len[q]), int(got.right_parent[q]), int(got.right_len[q])) for q in (3, 7)] == [(0, 0, 0, 0)] * 2
    assert got.flags.tolist() == [0, 0, 0, 0, 0, 1, 0, 0] and store.self_chimeras(6, 2, 0).left_parent[3] == NONE
    store.close()


def test_every_length_and_the_packed_order(tmp_path):
    """L = 9, 31, 32, 33, 64, 65, 130 and aa250 (8 words per plane): breakpoints on both sides of every plane-word edge, the first
    and the last column.  The packed column order is not the identity on at least one of these stores (read from the packed
    store file, the one thing the API shows of it): without that the mapping back to source columns would go untested."""
    shuffled = {}
    for key in ("nt9", "nt31", "nt32", "nt33", "nt64", "nt65", "nt130", "aa250"):
        L = STORES[key][2]
        store = store_of(key)
        for D, F in ((3, 2), (3, 1), (6, 2), (L, 2)):
            check(store.self_chimeras(D, F, 0), expected(key, D, 0, F), (key, D, F))
        assert expected(key, 3, 0, 2).n_chimeras >= 3
        path = str(tmp_path / (key + ".packed"))
        store.save(path)
        perm = packed_perm(path, L)
        assert sorted(perm.tolist()) == list(range(L))
        shuffled[key] = int((perm != np.arange(L)).sum())
        store.close()
    print("packed columns away from their source column: %s" % shuffled)
    assert any(shuffled.values()), shuffled


def test_kernels_by_name_and_statistics():
    """chimera::init_sides_kernel, chimera::offer_sides_kernel and chimera::verdict_kernel behind the peaks call's
    smafa_pk::init_peaks_kernel and smafa_pk::weigh_keep_kernel, in launch order"""
    store = store_of("nt60")
    check(store.self_chimeras(3, 2, 0), expected("nt60", 3, 0, 2))
    kernels = store.last_call_kernels()
    assert kernels[-7:] == ["smafa_join::store_records_kernel", "smafa_join::inverse_order_kernel"] + FULL, kernels
    assert kernels[0].startswith("smafa::") and all(k.startswith("smafa::") for k in kernels[:-7]), kernels
    stats = store.last_call_stats()
    assert stats["kernel_ms"] > 0 and stats["launches"] >= 7 and stats["scans"] >= 1, stats
    assert store.last_scan_ms()[0] == pytest.approx(stats["kernel_ms"])
    check(store.self_chimeras(3, 2, 0), expected("nt60", 3, 0, 2))  # once more: the inverse order map is current
    assert store.last_call_kernels()[-6:] == ["smafa_join::store_records_kernel"] + FULL
    store.close()


def test_two_runs_give_identical_bytes():
    a, b = store_of("aa60"), store_of("aa60")
    first, again, other = a.self_chimeras(6, 1, 1), a.self_chimeras(6, 1, 1), b.self_chimeras(6, 1, 1)
    check(again, first)
    check(other, first)
    check(first, expected("aa60", 6, 1, 1))
    a.close()
    b.close()


def test_several_spans_off_the_tile_grid(monkeypatch):
    """SMAFA_JOIN_BLOCK=192 SMAFA_JOIN_STRIDE=3: 1 743 rows in spans of 576 positions, which begin inside wave tiles"""
    monkeypatch.setenv("SMAFA_JOIN_BLOCK", "192")
    monkeypatch.setenv("SMAFA_JOIN_STRIDE", "3")
    store = store_of("nt60big")  # (the knobs are read when the handle is made)
    monkeypatch.delenv("SMAFA_JOIN_BLOCK")
    monkeypatch.delenv("SMAFA_JOIN_STRIDE")
    n = len(planted("nt60big")[0])
    for D, r, F in ((3, 0, 2), (6, 1, 1)):
        check(store.self_chimeras(D, F, r), expected("nt60big", D, r, F), (D, r, F))
        assert store.last_call_stats()["scans"] >= -(-n // 192), store.last_call_stats()
        assert our_kernels(store) == FULL
    store.close()


def test_the_join_again_plan(monkeypatch):
    """SMAFA_DENSITY_KEEP_MAX below the pair count, and 0: the kept list cannot hold the pairs, the store is joined twice and
    chimera::offer_sides_kernel reads raw piece lists — self-pairs, mirror images and all.  The same bytes."""
    key, D, r, F = "nt60", 3, 0, 2
    want = expected(key, D, r, F)
    scans = {}
    for knob in (None, "0", "100"):
        if knob is None:
            monkeypatch.delenv("SMAFA_DENSITY_KEEP_MAX", raising=False)
        else:
            monkeypatch.setenv("SMAFA_DENSITY_KEEP_MAX", knob)  # (read when the handle is made)
        store = store_of(key)
        monkeypatch.delenv("SMAFA_DENSITY_KEEP_MAX", raising=False)
        check(store.self_chimeras(D, F, r), want, knob)
        assert "chimera::offer_sides_kernel" in store.last_call_kernels() and our_kernels(store) == FULL
        scans[knob] = store.last_call_stats()["scans"]
        check(store.self_chimeras(6, 1, 1), expected(key, 6, 1, 1), knob)
        store.close()
    print("scans per call: %s" % scans)
    assert scans[None] >= 1 and scans["0"] == 2 * scans[None] and scans["100"] == 2 * scans[None], scans


def test_with_a_block_index(monkeypatch):
    """a current block index answers the blocks: its repeats reach phase 2 (limits lifted as tests/test_gpu_peaks.py lifts them)"""
    key, D = "aa60", 3
    monkeypatch.setenv("SMAFA_INDEX_CAND", "100")
    monkeypatch.setenv("SMAFA_INDEX_MAX_RUN", "100000000")
    store = store_of(key)
    monkeypatch.delenv("SMAFA_INDEX_CAND")
    monkeypatch.delenv("SMAFA_INDEX_MAX_RUN")
    info = store.build_index(D)
    store.set_index(1)
    assert info["max_div_served"] is not None and info["max_div_served"] >= D, info
    before = store.index_info()["probe_launches"]
    check(store.self_chimeras(D, 2, 0), expected(key, D, 0, 2))
    assert store.index_info()["probe_launches"] > before
    assert any("index_probe_kernel" in k for k in store.last_call_kernels())
    check(store.self_chimeras(D, 1, 1), expected(key, D, 1, 1))
    store.close()


def test_store_states(monkeypatch):
    """a re-planed store (two planes, then three with the first N); a sorted store with an unsorted tail, and the same store after
    the scan that sorts it again"""
    pieces, _ = replaned_case()
    store = make_store(pieces[0], "nt")
    held = pieces[0]
    for piece, planes in ((None, 2), (pieces[1], 2), (pieces[2], 3)):
        if piece is not None:
            store.push(piece)
            held = np.concatenate([held, piece])
        assert store.info().planes == planes
        for D, F in ((5, 1), (3, 2)):
            check(store.self_chimeras(D, F, 0), brute_chimeras(held, D, 0, F), (len(held), D, F))
    assert (brute_chimeras(held, 5, 0, 1).left_parent != NONE).sum() > 100  # (the planted families: many parents, if few chimeras)
    store.close()

    monkeypatch.setenv("SMAFA_RESORT_MIN", "1000")  # (read when the handle is made)
    held = planted("nt60big")[0]
    store = make_store(held, "nt")
    monkeypatch.delenv("SMAFA_RESORT_MIN")
    rng = np.random.default_rng(31)
    check(store.self_chimeras(3, 2, 0), expected("nt60big", 3, 0, 2))
    for k in range(3):
        tail = held[rng.integers(0, len(held), size=100)].copy()
        tail[:, k] = (tail[:, k] + 1) % 4
        store.push(tail)
        held = np.concatenate([held, tail])
        check(store.self_chimeras(3, 1, 0), brute_chimeras(held, 3, 0, 1), "tail %d" % k)
    more = held[rng.integers(0, len(held), size=400)].copy()
    store.push(more)
    held = np.concatenate([held, more])
    want = brute_chimeras(held, 3, 0, 2)
    assert want.n_chimeras >= 4
    check(store.self_chimeras(3, 2, 0), want, "a quarter of the store unsorted")
    store.scan(held[:4], max_divergence=2)  # a quarter of the store has arrived since the sort: this scan sorts it again
    check(store.self_chimeras(3, 2, 0), want, "sorted again")
    store.close()


def test_weights_in():
    key, D, F = "nt60", 3, 2
    codes = planted(key)[0]
    n = len(codes)
    store = store_of(key)
    counted = expected(key, D, 0, F)
    # equal to the counted weights: the same answer, whatever radius is named beside them
    for r in (0, 2):
        check(store.self_chimeras(D, F, r, weights=counted.weights), counted, "counted weights given")
    assert our_kernels(store) == FULL
    # with zeros: those rows are neither flagged nor parents — every second parent of the flagged rows is taken out
    zeroed = counted.weights.copy()
    flagged = np.flatnonzero(counted.flags)
    zeroed[counted.left_parent[flagged[::2]]] = 0
    zeroed[flagged[1]] = 0
    want = brute_chimeras(codes, D, 0, F, zeroed)
    got = store.self_chimeras(D, F, 0, weights=zeroed)
    check(got, want, "weights with zeros")
    out = np.flatnonzero(zeroed == 0)
    assert not got.flags[out].any() and (got.left_parent[out] == NONE).all() and (got.right_parent[out] == NONE).all()
    assert not np.isin(got.left_parent, out).any() and not np.isin(got.right_parent, out).any()
    assert want.left_parent.tobytes() != counted.left_parent.tobytes() and got.weights.tobytes() == zeroed.tobytes()
    # the pipeline form: peaks' cluster sizes on the peaks, 0 elsewhere — the centres alone are checked, by sizes.  The peaks
    # are taken at bound 1: a bimera two columns from either parent is a centre of its own there, which is what the check is for
    labels, parents, _, n_peaks = store.self_peaks(1, 0)
    want_peaks = brute_peaks(codes, 1, 0)
    assert labels.tobytes() == want_peaks[0].tobytes()
    sizes = np.bincount(labels, minlength=n).astype(np.uint32)
    assert int((sizes > 0).sum()) == n_peaks and (sizes[labels != np.arange(n)] == 0).all()
    want = brute_chimeras(codes, D, 0, F, sizes)
    check(store.self_chimeras(D, F, 0, weights=sizes), want, "pipeline")
    print("pipeline form: %d peaks, %d of them flagged" % (n_peaks, want.n_chimeras))
    assert want.n_chimeras >= 1 and (sizes[np.flatnonzero(want.flags)] > 0).all()
    # weights as large as they get: the fold is taken in 64 bits
    big = np.where(counted.weights > 10, 0xFFFFFFFF, 0x80000000).astype(np.uint32)
    check(store.self_chimeras(D, 2, 0, weights=big), brute_chimeras(codes, D, 0, 2, big), "2^31 x 2")
    check(store.self_chimeras(D, 1, 0, weights=big), brute_chimeras(codes, D, 0, 1, big), "2^31 x 1")
    assert brute_chimeras(codes, D, 0, 2, big).n_chimeras == 0 and brute_chimeras(codes, D, 0, 1, big).n_chimeras >= 4
    with pytest.raises(ValueError):
        store.self_chimeras(D, F, 0, weights=sizes[:-1])
    store.close()


def test_between_the_other_calls_on_one_handle():
    """the same bytes after, and followed by, self_peaks, self_density, self_neighbours, self_stable_clusters and a query scan on
    one handle; theirs are unchanged behind it"""
    key, D = "aa60", 3
    codes = planted(key)[0]
    want = expected(key, D, 0, 2)
    store = store_of(key)
    others = {
        "peaks": lambda: store.self_peaks(D, 0),
        "density": lambda: store.self_density(D, 3),
        "neighbours": lambda: store.self_neighbours(D, 4),
        "stable": lambda: store.self_stable_clusters(D, 3),
        "scan": lambda: (store.scan(codes[:50], max_divergence=D),),
        "components": lambda: store.self_components(D),
    }

    def frozen(result):
        return [x.tobytes() if isinstance(x, np.ndarray) else x for x in result]

    before = {name: frozen(call()) for name, call in others.items()}
    check(store.self_chimeras(D, 2, 0), want, "behind all of them")
    for name, call in others.items():
        assert frozen(call()) == before[name], name + " behind the chimera check"
        check(store.self_chimeras(D, 2, 0), want, "behind " + name)
        check(store.self_chimeras(6, 1, 1), expected(key, 6, 1, 1), "behind " + name)
    store.close()


def test_edges():
    L = 60
    store = smafa_amd.SubjectStore(L, smafa_amd.ALPHABET_NT)
    got = store.self_chimeras(5)
    assert all(getattr(got, f).shape == (0,) for f in FIELDS) and got.n_chimeras == 0
    assert store.self_chimeras(5, weights=np.zeros(0, dtype=np.uint32)).n_chimeras == 0
    row = np.random.default_rng(4).integers(0, 4, size=(1, L)).astype(np.uint8)
    store.push(row)
    for D, r in ((5, 0), (5, 5), (L, 0), (L + 1, L + 1)):
        got = store.self_chimeras(D, 2, r)
        check(got, brute_chimeras(row, D, r, 2), (D, r))
        assert got.flags.tolist() == [0] and got.left_parent.tolist() == [NONE] and got.weights.tolist() == [1]
        assert not [k for k in store.last_call_kernels() if k.startswith(("smafa::", "smafa_join::"))], store.last_call_kernels()  # no scan
    assert store.self_chimeras(5, 2, 0, weights=np.array([7], dtype=np.uint32)).weights.tolist() == [7]
    store.close()
    # bounds no two rows can exceed: every other row is a candidate parent, the join runs at L; a radius as large: every weight
    # is n, no row has a parent and nothing is scanned
    key = "nt9"
    codes, L = planted(key)[0], 9
    store = store_of(key)
    for bound in (L, L + 3):
        for F in (1, 2):
            want = brute_chimeras(codes, bound, 0, F)
            check(store.self_chimeras(bound, F, 0), want, (bound, F))
        last_resort = (want.left_parent != NONE) & (want.left_len == 0) & (want.right_len == 0)
        assert our_kernels(store) == FULL and any(k.startswith("smafa::") for k in store.last_call_kernels())
        for r in (L, bound, None):
            got = store.self_chimeras(bound, 1, r)
            check(got, brute_chimeras(codes, bound, bound, 1), (bound, r))
            assert (got.weights == len(codes)).all() and got.n_chimeras == 0 and (got.left_parent == NONE).all()
            assert not [k for k in store.last_call_kernels() if k.startswith(("smafa::", "smafa_join::"))], store.last_call_kernels()
            assert our_kernels(store) == [WEIGHED[0], OURS[0], OURS[2]]
    print("rows whose only parents share no column with them at D = %d: %d" % (L + 3, int(last_resort.sum())))
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_chimeras(None)
    assert e.value.code == _lib.ERR_INVALID and "max_div" in str(e.value)
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_chimeras(2, 2, 3)
    assert e.value.code == _lib.ERR_INVALID and "radius 3" in str(e.value)
    with pytest.raises(smafa_amd.SmafaError) as e:
        store.self_chimeras(2, 0)
    assert e.value.code == _lib.ERR_INVALID and "min_fold" in str(e.value)
    store.close()


def text_of(answer):
    signed = lambda v: -1 if v == NONE else int(v)  # noqa: E731
    return "".join("%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (i, answer.flags[i], signed(answer.left_parent[i]), answer.left_len[i],
                                                   signed(answer.right_parent[i]), answer.right_len[i], answer.weights[i])
                   for i in range(len(answer.flags))).encode()


@pytest.mark.parametrize("key,D,flags", [("nt60", 3, []), ("aa60", 6, ["--min-fold", "1", "--radius", "1"])])
def test_cli_chimeras(tmp_path, key, D, flags):
    """the version-2 (nt) / version-3 (aa) file and the packed file; --min-fold and --radius defaulted (2, 0) and given; --weights
    from a file and from stdin, on both file formats"""
    codes, kind = planted(key)[0], STORES[key][1]
    n = len(codes)
    F, r = (1, 1) if flags else (2, 0)
    want = expected(key, D, r, F)
    assert want.n_chimeras >= 1 and (want.left_parent == NONE).any() and (want.left_parent != NONE).sum() >= 5
    fa, db, packed = (str(tmp_path / name) for name in ("s.fa", "s.db", "s.packed"))
    synth.write_fasta(fa, codes, 1 if kind == "aa" else 0)
    alphabet = ["--alphabet", kind]
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", db, *alphabet], capture_output=True).returncode == 0
    assert subprocess.run([_lib.CLI_PATH, "makedb", "-i", fa, "-d", packed, "--packed", *alphabet], capture_output=True).returncode == 0
    for path in (db, packed):
        p = subprocess.run([_lib.CLI_PATH, "chimeras", "-d", path, "--max-divergence", str(D), *flags], capture_output=True)
        assert p.returncode == 0, p.stderr
        assert p.stdout == text_of(want), path
    out = str(tmp_path / "chimeras.tsv")
    with open(out, "wb") as f:
        smafa_amd.chimeras(db, D, F, r, out_fd=f.fileno())
    assert open(out, "rb").read() == text_of(want)
    # --weights: lines in any order, further columns ignored, a missing row is weight 0
    given = want.weights.copy()
    given[::5] = 0
    rows = [i for i in np.random.default_rng(2).permutation(n) if given[i]]
    lines = "".join("%d\t%d\tignored\t7\n" % (i, given[i]) if i % 2 else "%d\t%d\n" % (i, given[i]) for i in rows)
    wpath = str(tmp_path / "weights.tsv")
    open(wpath, "w").write(lines)
    text = text_of(brute_chimeras(codes, D, r, F, given))
    assert text != text_of(want)
    base = [_lib.CLI_PATH, "chimeras", "-d", db, "--max-divergence", str(D), *flags, "--weights"]
    p = subprocess.run(base + [wpath], capture_output=True)
    assert p.returncode == 0 and p.stdout == text, p.stderr
    p = subprocess.run(base + ["-"], input=lines.encode(), capture_output=True)
    assert p.returncode == 0 and p.stdout == text, p.stderr
    p = subprocess.run(base[:-1] + ["--weights", wpath, "-d", packed], capture_output=True)
    assert p.returncode == 0 and p.stdout == text, p.stderr


def test_cli_errors_name_the_line(tmp_path):
    """a malformed line, a duplicate or an out-of-range row is SMAFA_ERR_INVALID naming the line, exit status 1, nothing printed; an
    empty DB prints nothing and exits 0 (the eight rows of the hand-worked store: each case is a process of its own)"""
    n = len(HAND)
    db = str(tmp_path / "hand.db")
    smafa_amd.write_db(db, HAND, smafa_amd.ALPHABET_NT)
    base = [_lib.CLI_PATH, "chimeras", "-d", db, "--max-divergence", "3", "--weights"]
    good = "5\t1\n0\t3\textra\n3\t2\n"
    p = subprocess.run(base + ["-"], input=good.encode(), capture_output=True)
    want = brute_chimeras(HAND, 3, 0, 2, np.array([3, 0, 0, 2, 0, 1, 0, 0], dtype=np.uint32))
    assert p.returncode == 0 and p.stdout == text_of(want) and want.n_chimeras == 1, p.stderr
    for bad, line, what in ((good + "5\t3\n", 4, b"second line"), ("0\t1\n%d\t1\n" % n, 2, b"sequence number"),
                            ("0\t1\n1 1\n", 2, b"no tab"), ("0\t1\n1\tx\n", 2, b"no weight"), ("0\t1\n\n", 2, b"no sequence number"),
                            ("0\t1\n1\t4294967296\n", 2, b"no weight"), ("0\t1x\n", 1, b"not a number")):
        p = subprocess.run(base + ["-"], input=bad.encode(), capture_output=True)
        assert p.returncode == 1 and p.stdout == b"", (bad[-20:], p.stderr)
        assert b"weights line %d:" % line in p.stderr and what in p.stderr, (bad[-20:], p.stderr)
    p = subprocess.run(base + [str(tmp_path / "missing.tsv")], capture_output=True)
    assert p.returncode == 1 and b"cannot open weights file" in p.stderr
    empty_db = str(tmp_path / "e.db")
    # (a version-3 file, amino acids: a version-2 file without rows is three bytes, which `smafa` refuses as the reference does)
    smafa_amd.write_db(empty_db, np.zeros((0, 60), dtype=np.uint8), smafa_amd.ALPHABET_AA)
    p = subprocess.run([_lib.CLI_PATH, "chimeras", "-d", empty_db, "--max-divergence", "2"], capture_output=True)
    assert p.returncode == 0 and p.stdout == b"", p.stderr
