"""GPU parity of the pigeonhole key test of scan_zone_kernel<.., DIRECT> (kernels.hip.h, zone_key_sets).

Sorted stores of 2^20 + 100 rows (4097 wave tiles, the last one partial: its tiles share about 12 filter bits) hold a family
of 1024 rows that agree on every column but four (eight of them on all).  The sort gathers the family into whole tiles,
whose shared columns are then nearly all of them.  Queries are the family's base with exactly the bound and one more substitutions in the
family-shared columns — where a substitution flips the filter bit it is counted by the zone level, and the key test only
keeps the family's tiles if the query's keys take the tile's own bits there — plus store rows a few substitutions away and
far rows.  Rows are compared byte for byte with the oracle, with the key test on every (chunk, tile) (SMAFA_ZONE_KEY_GATE=0),
and at 60 columns also with the default gate and with the test off, which must give the same rows.
"""
import os

import numpy as np
import pytest

import oracle
import smafa_amd

pytestmark = pytest.mark.gpu
BOUND = 5
LETTERS = {smafa_amd.ALPHABET_NT: b"ACGT", smafa_amd.ALPHABET_AA: b"ACDEFGHIKLMNPQRSTVWY"}


@pytest.fixture(scope="module", autouse=True)
def _built():
    smafa_amd.build()
    oracle.build()
    assert smafa_amd.device_count() >= 1


def make_case(alphabet, L, seed):
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(LETTERS[alphabet], dtype=np.uint8)
    nl = len(lut)
    n = (1 << 20) + 100
    s = rng.integers(0, nl, size=(n, L), dtype=np.uint8)
    base = rng.integers(0, nl, size=L, dtype=np.uint8)
    free = rng.choice(L, size=4, replace=False)
    fam = np.repeat(base[None, :], 1024, axis=0)
    fam[:, free] = rng.integers(0, nl, size=(1024, 4), dtype=np.uint8)
    fam[:8] = base  # (the planted queries' hits)
    s[rng.choice(n, size=1024, replace=False)] = fam
    shared = np.setdiff1d(np.arange(L), free)
    q = []
    for i in range(64):  # the family's base, exactly at the bound and one past it, in the shared columns
        r = base.copy()
        for c in rng.choice(shared, size=BOUND + (i & 1), replace=False):
            r[c] = (r[c] + rng.integers(1, nl)) % nl
        q.append(r)
    for i in range(48):  # store rows a few substitutions away
        r = s[rng.integers(0, n)].copy()
        for c in rng.choice(L, size=int(rng.integers(0, BOUND + 2)), replace=False):
            r[c] = (r[c] + rng.integers(1, nl)) % nl
        q.append(r)
    q += list(rng.integers(0, nl, size=(16, L), dtype=np.uint8))  # far rows
    q = np.array(q, dtype=np.uint8)
    return lut[s], lut[q]


def scan(alphabet, L, subj, qry, gate):
    old = os.environ.get("SMAFA_ZONE_KEY_GATE")
    os.environ["SMAFA_ZONE_KEY_GATE"] = gate  # read when the handle is created
    try:
        store = smafa_amd.SubjectStore(L, alphabet, 0)
    finally:
        if old is None:
            os.environ.pop("SMAFA_ZONE_KEY_GATE")
        else:
            os.environ["SMAFA_ZONE_KEY_GATE"] = old
    try:
        store.push(smafa_amd.encode_rows(subj, alphabet))
        store.set_zone_level(2)
        got = store.scan(smafa_amd.encode_rows(qry, alphabet), max_divergence=BOUND)
        kernel = store.last_scan_kernel()
    finally:
        store.close()
    assert kernel.startswith("smafa::scan_zone_kernel") and kernel.endswith("2, true, true>"), kernel
    return got


@pytest.mark.parametrize("alphabet,L", [(smafa_amd.ALPHABET_AA, L) for L in (33, 44, 56, 60, 64)] +
                         [(smafa_amd.ALPHABET_NT, L) for L in (33, 60)])
def test_zone_keys_match_oracle(alphabet, L):
    subj, qry = make_case(alphabet, L, 1000 * alphabet + L)
    want = oracle.scan_codes(oracle.codes_from_ascii(subj, alphabet), oracle.codes_from_ascii(qry, alphabet), BOUND)
    # the planted family queries: hits at the bound for every even one, none from the family for the odd ones
    assert len(np.unique(want["query"][want["query"] < 64])) >= 32
    got = scan(alphabet, L, subj, qry, "0")
    assert got.tobytes() == want.tobytes()
    if L == 60:
        for gate in ("3", "65"):  # the default gate, and the key test off
            assert scan(alphabet, L, subj, qry, gate).tobytes() == want.tobytes(), gate
