"""Host-side mirror of the reference crate's interface for the hot path.

``makedb`` / ``query`` / ``cluster`` / ``count`` take the arguments of the reference's public
functions (/root/reference/src/lib.rs:137,198,378; src/cluster.rs:13) — paths, and ``None`` for an
absent option — and produce the same bytes.  ``SubjectStore`` is the ``WindowSet`` of
src/lib.rs:54-135 living in HBM: ``push``/``get_distances``/``scan``.  Everything goes through the C
ABI of libsmafa_amd.so; nothing here computes distances on the CPU.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
from typing import Optional

import numpy as np

from . import _lib
from ._lib import ALPHABET_AA, ALPHABET_NT, NONE, Hit, SmafaError, SmafaPanic, check, lib

HIT_DTYPE = np.dtype([("query", "<u4"), ("subject", "<u4"), ("dist", "<u4")])
# what SubjectStore.self_chimeras returns: six uint32 arrays, one entry per subject, and the number of flagged rows
Chimeras = collections.namedtuple("Chimeras", "flags left_parent left_len right_parent right_len weights n_chimeras")
# one entry of the abundance table (smafa_table_entry), and what SubjectStore.assign returns: the entries in table order, per read
# its subject and distance (or None), per subject the weight assigned to it (or None), and the four totals
TABLE_DTYPE = np.dtype([("label", "<u4"), ("sample", "<u4"), ("count", "<u8")])
TableEntry = TABLE_DTYPE
Assigned = collections.namedtuple("Assigned", "entries subject dist subject_counts totals")
# what SubjectStore.classify returns: the (taxon, sample) entries in table order (TABLE_DTYPE, label = taxon), per read its anchor,
# distance, taxon, depth and ties, and the six totals.  TAXON_ROOT: the taxon of a read whose best hits share no rank
Classified = collections.namedtuple("Classified", "entries subject dist taxon depth ties totals")
TAXON_ROOT = 0xFFFFFFFE


def _opt(v: Optional[int]) -> int:
    return NONE if v is None else int(v)


# ---- what SubjectStore.assign and SubjectStore.classify share
def _given(a, count, what):
    """a side array as contiguous uint32 of `count` elements (None: not given)"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.uint32)
    if a.shape != (count,):
        raise ValueError(f"{what} has shape {a.shape}, expected ({count},)")
    return a


def _per_read(samples, weights, n_samples, m):
    """(samples, weights, n_samples) for m reads; n_samples None: the largest sample number + 1"""
    samples, weights = _given(samples, m, "samples"), _given(weights, m, "weights")
    if n_samples is None:
        n_samples = int(samples.max()) + 1 if samples is not None and m else 1
    return samples, weights, int(n_samples)


def _ptr(a, empty=False):
    """the address of an array, None where there is none — or, unless `empty`, nothing in it"""
    return a.ctypes.data if a is not None and (empty or a.size) else None


def _with_entries(m, totals, call):
    """the entries of call(entries address, capacity), which fills totals; an entry buffer that was too small (ERR_CAPACITY) is
    grown to totals[0], the number the call asks for, and the call made again"""
    cap = min(m, 1 << 16)
    while True:
        entries = np.zeros(cap, dtype=TABLE_DTYPE)
        rc = call(entries.ctypes.data if cap else None, cap)
        if rc != _lib.ERR_CAPACITY:
            check(rc)
            return entries[: int(totals[0])]
        cap = int(totals[0])


def device_count() -> int:
    return lib().smafa_device_count()


def build_id() -> str:
    return lib().smafa_build_id().decode()


def hbm_read_probe(device: int = 0, nbytes: int = 8 << 30) -> float:
    """Empirical HBM read-stream rate of the device in GB/s (a trivial sum kernel over `nbytes`)."""
    out = C.c_double(0.0)
    check(lib().smafa_hbm_read_probe(device, nbytes, C.byref(out)))
    return out.value


def encode(seq: bytes, alphabet: int = ALPHABET_NT) -> np.ndarray:
    """ASCII -> code bytes (create_lut / from_bytes, src/lib.rs:29-52,167-196)."""
    out = np.empty(len(seq), dtype=np.uint8)
    bad = C.c_uint64(0)
    check(lib().smafa_encode(alphabet, seq, len(seq), out.ctypes.data, C.byref(bad)))
    return out


def encode_rows(ascii_rows: np.ndarray, alphabet: int = ALPHABET_NT) -> np.ndarray:
    a = np.ascontiguousarray(ascii_rows, dtype=np.uint8)
    out = np.empty_like(a)
    bad = C.c_uint64(0)
    check(lib().smafa_encode(alphabet, a.ctypes.data, a.size, out.ctypes.data, C.byref(bad)))
    return out


def decode(codes: np.ndarray, alphabet: int = ALPHABET_NT) -> bytes:
    """code bytes -> subject string (get_as_string, src/lib.rs:113-135)."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    out = C.create_string_buffer(codes.size)
    check(lib().smafa_decode(alphabet, codes.ctypes.data, codes.size, out))
    return out.raw


class QuerySet:
    """A packed query batch resident in HBM."""

    def __init__(self, store: "SubjectStore", query_codes: np.ndarray):
        q = np.ascontiguousarray(query_codes, dtype=np.uint8)
        assert q.ndim == 2 and q.shape[1] == store.seq_len
        self.n = q.shape[0]
        self._h = C.c_void_p()
        self._store = store
        check(lib().smafa_qset_create(C.byref(self._h), store._h, q.ctypes.data, self.n))

    def close(self):
        if self._h:
            lib().smafa_qset_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SubjectStore:
    """WindowSet (src/lib.rs:54-135) resident in HBM as bit-planes."""

    def __init__(self, seq_len: int, alphabet: int = ALPHABET_NT, device: int = 0):
        self._h = C.c_void_p()
        self.seq_len = int(seq_len)
        self.alphabet = alphabet
        check(lib().smafa_db_create(C.byref(self._h), device, alphabet, self.seq_len))

    @classmethod
    def load(cls, path: str, device: int = 0) -> "SubjectStore":
        """a store from a packed store file (smafa_db_load): mmap + three host-to-device copies"""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        check(lib().smafa_db_load(C.byref(self._h), device, os.fsencode(path)))
        info = self.info()
        self.seq_len, self.alphabet = int(info.seq_len), int(info.alphabet)
        return self

    def save(self, path: str) -> None:
        check(lib().smafa_db_save(self._h, os.fsencode(path)))

    # push_encoding x n (src/lib.rs:91-111)
    def push(self, codes: np.ndarray) -> None:
        c = np.ascontiguousarray(codes, dtype=np.uint8)
        if c.ndim != 2 or c.shape[1] != self.seq_len:
            raise SmafaPanic(_lib.ERR_PANIC, "WindowSet seq length is %d, got a new sequence of length %d"
                             % (self.seq_len, c.shape[-1]))
        check(lib().smafa_db_append(self._h, c.ctypes.data, c.shape[0]))

    def __len__(self) -> int:
        return int(self.info().n_subjects)

    def info(self) -> _lib.DbInfo:
        info = _lib.DbInfo()
        check(lib().smafa_db_info(self._h, C.byref(info)))
        return info

    # get_distances (src/lib.rs:71-89)
    def get_distances(self, query_codes: np.ndarray) -> np.ndarray:
        q = np.ascontiguousarray(query_codes, dtype=np.uint8).reshape(-1)
        if q.size != self.seq_len:
            raise SmafaPanic(_lib.ERR_PANIC, "Cannot compute distances between seq of length %d and windows of lengths %d"
                             % (q.size, self.seq_len))
        out = np.zeros(len(self), dtype=np.uint32)
        check(lib().smafa_distances(self._h, q.ctypes.data, out.ctypes.data))
        return out

    def scan(self, query_codes: np.ndarray, max_divergence: Optional[int] = None,
             max_num_hits: Optional[int] = None) -> np.ndarray:
        """All (query, subject, dist) rows within the bounds, ordered (query, dist, subject)."""
        q = np.ascontiguousarray(query_codes, dtype=np.uint8)
        assert q.ndim == 2 and q.shape[1] == self.seq_len
        cap = 1 << 16
        while True:
            out = np.zeros(cap, dtype=HIT_DTYPE)
            n_out = C.c_uint64(0)
            rc = lib().smafa_scan_hits(self._h, q.ctypes.data, q.shape[0], _opt(max_divergence), _opt(max_num_hits),
                                       out.ctypes.data, cap, C.byref(n_out))
            if rc == _lib.ERR_CAPACITY:
                cap = int(n_out.value)
                continue
            check(rc)
            return out[: n_out.value]

    # ---- device-resident form -------------------------------------------------------------
    def set_stream(self, hip_stream: int) -> None:
        check(lib().smafa_db_set_stream(self._h, C.c_void_p(hip_stream)))

    def set_query_block(self, n: int) -> None:
        check(lib().smafa_set_query_block(self._h, n))

    def set_prefilter(self, enabled: bool) -> None:
        check(lib().smafa_set_prefilter(self._h, 1 if enabled else 0))

    def set_zone_level(self, mode: int) -> None:
        check(lib().smafa_set_zone_level(self._h, int(mode)))

    def build_index(self, max_divergence: int) -> dict:
        """the block index of the resident store (smafa_db_build_index): fixed bounds up to max_divergence are then answered
        by max_divergence + 1 probes per query wherever the store's blocks are selective enough"""
        check(lib().smafa_db_build_index(self._h, int(max_divergence)))
        return self.index_info()

    def drop_index(self) -> None:
        check(lib().smafa_db_drop_index(self._h))

    def set_index(self, mode: int) -> None:
        check(lib().smafa_set_index(self._h, int(mode)))

    def index_info(self) -> dict:
        info = _lib.IndexInfo()
        check(lib().smafa_index_info(self._h, C.byref(info)))
        d = {k: getattr(info, k) for k, _ in _lib.IndexInfo._fields_}
        d["max_div_served"] = None if d["max_div_served"] == _lib.NONE else d["max_div_served"]
        return d

    def scan_launch(self, qset: QuerySet, max_divergence: Optional[int], max_num_hits: Optional[int],
                    d_hits: int, cap: int, d_count: int) -> None:
        check(lib().smafa_scan_launch(self._h, qset._h, _opt(max_divergence), _opt(max_num_hits),
                                      C.c_void_p(d_hits), cap, C.c_void_p(d_count)))

    def scan_each(self, qset: QuerySet, max_divergence: Optional[int], d_hits: int, cap_per_query: int, d_counts: int,
                  use_graph: bool = False) -> None:
        """one store pass per query, enqueued back to back (smafa_scan_each)"""
        check(lib().smafa_scan_each(self._h, qset._h, _opt(max_divergence), C.c_void_p(d_hits), cap_per_query,
                                    C.c_void_p(d_counts), 1 if use_graph else 0))

    # ---- the self-join ---------------------------------------------------------------------
    def self_pairs(self, max_divergence: int, first_cap: int = 1 << 16) -> np.ndarray:
        """Every unordered pair of the store's own subjects within max_divergence, once, as rows (query = the smaller subject
        number, subject = the larger, dist), ordered (query, dist, subject) — smafa_db_self_hits; `first_cap` rows are offered
        first, and the buffer grows to what the call asks for."""
        cap = max(int(first_cap), 0)
        while True:
            out = np.zeros(max(cap, 1), dtype=HIT_DTYPE)
            n_out = C.c_uint64(0)
            rc = lib().smafa_db_self_hits(self._h, _opt(max_divergence), out.ctypes.data, cap, C.byref(n_out))
            if rc == _lib.ERR_CAPACITY:
                cap = int(n_out.value)
                continue
            check(rc)
            return out[: n_out.value]

    def self_launch(self, max_divergence: int, d_hits: int, cap: int, d_count: int) -> None:
        """device-resident self-join (smafa_db_self_launch): rows unordered in d_hits, the exact pair count in *d_count"""
        check(lib().smafa_db_self_launch(self._h, _opt(max_divergence), C.c_void_p(d_hits) if d_hits else None, cap,
                                         C.c_void_p(d_count) if d_count else None))

    # ---- single-linkage components ---------------------------------------------------------
    def self_components(self, max_divergence: int) -> tuple[np.ndarray, int]:
        """(labels, n_components): labels[i] = the smallest subject number in i's connected component of the graph whose edges
        are the store's pairs within max_divergence (uint32, one per subject) — smafa_db_self_components.  The pairs stay
        on the device."""
        n = self.info().n_subjects
        labels = np.zeros(max(n, 1), dtype=np.uint32)
        count = C.c_uint64(0)
        check(lib().smafa_db_self_components(self._h, _opt(max_divergence), labels.ctypes.data, n, C.byref(count)))
        return labels[:n], int(count.value)

    def self_components_launch(self, max_divergence: int, d_labels: int, d_n_components: int) -> None:
        """device-resident form (smafa_db_self_components_launch): n_subjects uint32 labels in d_labels, the number of
        components in *d_n_components (device uint64)"""
        check(lib().smafa_db_self_components_launch(self._h, _opt(max_divergence), C.c_void_p(d_labels) if d_labels else None,
                                                    C.c_void_p(d_n_components) if d_n_components else None))

    # ---- delta self-join: the rows appended since a mark ------------------------------------
    def self_pairs_since(self, first_row: int, max_divergence: int, first_cap: int = 1 << 16) -> np.ndarray:
        """Every unordered pair within max_divergence whose larger subject number is >= first_row — the pairs that the rows
        appended since the store had first_row rows have added — once, rows as self_pairs gives them, ordered (query, dist,
        subject) — smafa_db_self_hits_since.  self_pairs of the first first_row rows and these rows are disjoint and together
        self_pairs of the whole store."""
        cap = max(int(first_cap), 0)
        while True:
            out = np.zeros(max(cap, 1), dtype=HIT_DTYPE)
            n_out = C.c_uint64(0)
            rc = lib().smafa_db_self_hits_since(self._h, int(first_row), _opt(max_divergence), out.ctypes.data, cap, C.byref(n_out))
            if rc == _lib.ERR_CAPACITY:
                cap = int(n_out.value)
                continue
            check(rc)
            return out[: n_out.value]

    def self_since_launch(self, first_row: int, max_divergence: int, d_hits: int, cap: int, d_count: int) -> None:
        """device-resident form (smafa_db_self_since_launch): rows unordered in d_hits, the exact pair count in *d_count"""
        check(lib().smafa_db_self_since_launch(self._h, int(first_row), _opt(max_divergence), C.c_void_p(d_hits) if d_hits else None, cap,
                                               C.c_void_p(d_count) if d_count else None))

    def self_components_update(self, first_row: int, max_divergence: int, labels) -> tuple[np.ndarray, int]:
        """(labels, n_components) of the store as it is now, byte for byte those of self_components(max_divergence), from
        `labels`, whose first first_row entries are what self_components(max_divergence) gave when the store had first_row
        rows (entries behind them are ignored, and need not be there) — smafa_db_self_components_update: only the rows from
        first_row on are joined against the store.  `labels` itself is not written."""
        n = self.info().n_subjects
        given = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
        if len(given) < min(int(first_row), n):
            raise ValueError("labels holds %d entries, first_row is %d" % (len(given), first_row))
        out = np.zeros(max(n, 1), dtype=np.uint32)
        out[: min(len(given), n)] = given[:n]
        count = C.c_uint64(0)
        check(lib().smafa_db_self_components_update(self._h, int(first_row), _opt(max_divergence), out.ctypes.data, n, C.byref(count)))
        return out[:n], int(count.value)

    def self_components_update_launch(self, first_row: int, max_divergence: int, d_labels: int, d_n_components: int) -> None:
        """device-resident form (smafa_db_self_components_update_launch): n_subjects uint32 labels in d_labels, in and out,
        the number of components in *d_n_components (device uint64)"""
        check(lib().smafa_db_self_components_update_launch(self._h, int(first_row), _opt(max_divergence),
                                                           C.c_void_p(d_labels) if d_labels else None,
                                                           C.c_void_p(d_n_components) if d_n_components else None))

    # ---- single-linkage levels -------------------------------------------------------------
    def self_component_levels(self, max_divergence: int) -> tuple[np.ndarray, list[int]]:
        """(labels, counts): labels[t, i] = the label self_components(t) gives subject i, for every t = 0 .. max_divergence
        (uint32, shape (max_divergence + 1, n_subjects)), counts[t] = its number of components — smafa_db_self_levels: one
        join at the largest bound, one union-find per level.  The pairs stay on the device."""
        n = self.info().n_subjects
        levels = int(max_divergence) + 1 if max_divergence is not None and 0 <= int(max_divergence) < _lib.NONE else 1
        labels = np.zeros(max(levels * n, 1), dtype=np.uint32)
        counts = (C.c_uint64 * levels)()
        check(lib().smafa_db_self_levels(self._h, _opt(max_divergence), labels.ctypes.data, levels * n, counts))
        return labels[: levels * n].reshape(levels, n), [int(c) for c in counts]

    def self_component_levels_launch(self, max_divergence: int, d_labels: int, d_n_components: int) -> None:
        """device-resident form (smafa_db_self_levels_launch): (max_divergence + 1) x n_subjects uint32 labels in d_labels,
        max_divergence + 1 component counts in d_n_components (device uint64 each)"""
        check(lib().smafa_db_self_levels_launch(self._h, _opt(max_divergence), C.c_void_p(d_labels) if d_labels else None,
                                                C.c_void_p(d_n_components) if d_n_components else None))

    # ---- density clusters ------------------------------------------------------------------
    def self_density(self, max_divergence: int, min_pts: int, degrees: bool = True):
        """(labels, degrees, {"clusters", "core", "noise"}) — smafa_db_self_density: DBSCAN over the store's own rows with
        eps = max_divergence.  degrees[i] = the number of other subjects within the bound of subject i (None with
        degrees=False); a row is core iff degrees[i] + 1 >= min_pts; labels[i] = the smallest core subject number of i's
        cluster, for a border row the label of its smallest-numbered core neighbour, NONE (0xFFFFFFFF) for noise.  uint32,
        one per subject.  The pairs stay on the device."""
        n = self.info().n_subjects
        labels = np.zeros(max(n, 1), dtype=np.uint32)
        degs = np.zeros(max(n, 1), dtype=np.uint32) if degrees else None
        counts = (C.c_uint64 * 3)()
        check(lib().smafa_db_self_density(self._h, _opt(max_divergence), int(min_pts), labels.ctypes.data,
                                          degs.ctypes.data if degrees else None, n, counts))
        return labels[:n], (degs[:n] if degrees else None), {"clusters": int(counts[0]), "core": int(counts[1]), "noise": int(counts[2])}

    def self_density_launch(self, max_divergence: int, min_pts: int, d_labels: int, d_degrees: int, d_counts: int) -> None:
        """device-resident form (smafa_db_self_density_launch): n_subjects uint32 labels in d_labels, as many degrees in
        d_degrees (0: not wanted), {clusters, core rows, noise rows} in d_counts (3 device uint64)"""
        check(lib().smafa_db_self_density_launch(self._h, _opt(max_divergence), int(min_pts), C.c_void_p(d_labels) if d_labels else None,
                                                 C.c_void_p(d_degrees) if d_degrees else None,
                                                 C.c_void_p(d_counts) if d_counts else None))

    # ---- abundance-peak clusters -----------------------------------------------------------
    def self_peaks(self, max_divergence: int, radius: Optional[int] = 0, parents: bool = True, weights: bool = True, weights_in=None):
        """(labels, parents, weights, n_peaks) — smafa_db_self_peaks: weights[i] = 1 + the number of other subjects within
        `radius` of subject i (0: its exact copies; None: max_divergence), parents[i] = the subject of greatest (weight,
        smaller number) among i and the subjects within max_divergence of it — i itself makes i a peak — labels[i] = the peak
        reached from i along the parents.  uint32, one per subject; parents / weights are None where not wanted.  The pairs
        stay on the device.  weights_in (uint32, one per subject; smafa_db_self_peaks_weighted): weights[i] = weights_in[i] + the
        sum of weights_in over the other subjects within `radius` — the sizes of dereplicated sequences, on the store of the distinct ones:
        its peaks are then the peaks of the raw rows."""
        n = self.info().n_subjects
        labels = np.zeros(max(n, 1), dtype=np.uint32)
        par = np.zeros(max(n, 1), dtype=np.uint32) if parents else None
        wts = np.zeros(max(n, 1), dtype=np.uint32) if weights else None
        count = C.c_uint64(0)
        if weights_in is None:
            check(lib().smafa_db_self_peaks(self._h, _opt(max_divergence), _opt(radius), labels.ctypes.data,
                                            par.ctypes.data if parents else None, wts.ctypes.data if weights else None, n,
                                            C.byref(count)))
        else:
            given = _given(weights_in, n, "weights_in")
            check(lib().smafa_db_self_peaks_weighted(self._h, _opt(max_divergence), _opt(radius), _ptr(given), labels.ctypes.data,
                                                     par.ctypes.data if parents else None, wts.ctypes.data if weights else None, n,
                                                     C.byref(count)))
        return labels[:n], (par[:n] if parents else None), (wts[:n] if weights else None), int(count.value)

    def self_peaks_weighted_launch(self, max_divergence: int, radius: Optional[int], d_weights_in: int, d_labels: int, d_parents: int,
                                   d_weights: int, d_n_peaks: int) -> None:
        """device-resident form (smafa_db_self_peaks_weighted_launch): self_peaks_launch with n_subjects uint32 given weights in
        d_weights_in"""
        ptr = lambda a: C.c_void_p(a) if a else None  # noqa: E731
        check(lib().smafa_db_self_peaks_weighted_launch(self._h, _opt(max_divergence), _opt(radius), ptr(d_weights_in), ptr(d_labels),
                                                        ptr(d_parents), ptr(d_weights), ptr(d_n_peaks)))

    def self_peaks_launch(self, max_divergence: int, radius: Optional[int], d_labels: int, d_parents: int, d_weights: int,
                          d_n_peaks: int) -> None:
        """device-resident form (smafa_db_self_peaks_launch): n_subjects uint32 labels in d_labels, as many parents in
        d_parents and weights in d_weights (0: not wanted), the number of peaks in *d_n_peaks (device uint64)"""
        check(lib().smafa_db_self_peaks_launch(self._h, _opt(max_divergence), _opt(radius), C.c_void_p(d_labels) if d_labels else None,
                                               C.c_void_p(d_parents) if d_parents else None,
                                               C.c_void_p(d_weights) if d_weights else None,
                                               C.c_void_p(d_n_peaks) if d_n_peaks else None))

    # ---- chimera check -----------------------------------------------------------------------
    def self_chimeras(self, max_divergence: int, min_fold: int = 2, radius: Optional[int] = 0, weights=None) -> Chimeras:
        """Chimeras(flags, left_parent, left_len, right_parent, right_len, weights, n_chimeras) — smafa_db_self_chimeras: the
        two-parent bimeras of the store.  A parent of row q is a row within max_divergence of it whose weight is greater and at
        least min_fold times q's; left_parent[q] shares the longest prefix with q (left_len[q] columns), right_parent[q] the
        longest suffix, ties to the smaller number, NONE and 0 without a parent; flags[q] = 1 iff left_len[q] + right_len[q] >=
        seq_len: q is left_parent's head on right_parent's tail.  The weights are counted as self_peaks counts them at `radius`
        (0: exact copies; None: max_divergence), or taken from `weights` (uint32, one per subject; a row of weight 0 takes no
        part), and returned.  uint32, one per subject.  The pairs stay on the device."""
        n = self.info().n_subjects
        given = None
        if weights is not None:
            given = np.ascontiguousarray(weights, dtype=np.uint32)
            if given.shape != (n,):
                raise ValueError(f"weights has shape {given.shape}, the store has {n} subjects")
            if n == 0:
                given = np.zeros(1, dtype=np.uint32)
        out = [np.zeros(max(n, 1), dtype=np.uint32) for _ in range(6)]
        count = C.c_uint64(0)
        check(lib().smafa_db_self_chimeras(self._h, _opt(max_divergence), _opt(radius), int(min_fold),
                                           given.ctypes.data if given is not None else None, *(a.ctypes.data for a in out), n,
                                           C.byref(count)))
        return Chimeras(*(a[:n] for a in out), int(count.value))

    def self_chimeras_launch(self, max_divergence: int, radius: Optional[int], min_fold: int, d_weights_in: int, d_flags: int,
                             d_left_parent: int, d_left_len: int, d_right_parent: int, d_right_len: int, d_weights: int,
                             d_n_chimeras: int) -> None:
        """device-resident form (smafa_db_self_chimeras_launch): n_subjects uint32 weights in d_weights_in (0: counted at the
        radius), as many flags in d_flags and — each 0 where not wanted — parents, lengths and weights in the five buffers
        behind it, the number of flagged rows in *d_n_chimeras (device uint64)"""
        ptr = lambda a: C.c_void_p(a) if a else None  # noqa: E731
        check(lib().smafa_db_self_chimeras_launch(self._h, _opt(max_divergence), _opt(radius), int(min_fold), ptr(d_weights_in),
                                                  ptr(d_flags), ptr(d_left_parent), ptr(d_left_len), ptr(d_right_parent),
                                                  ptr(d_right_len), ptr(d_weights), ptr(d_n_chimeras)))

    # ---- neighbour lists ------------------------------------------------------------------
    def self_neighbours(self, max_divergence: int, k: Optional[int] = None, dists: bool = True, first_cap: int = 1 << 16):
        """(offsets uint64[n + 1], neighbours uint32, dists uint32 or None) — smafa_db_self_neighbours: the store's graph at
        max_divergence as per-row lists.  Row i's neighbours, every other subject within the bound, are
        neighbours[offsets[i]:offsets[i + 1]], ordered by (distance, number), with their distances beside them in `dists`;
        k cuts every list to its k nearest (ties to the smaller number).  `first_cap` entries are offered first, and the
        buffers grow to what the call asks for (it joins again).

        The three arrays are a CSR matrix as they are: scipy.sparse.csr_matrix((dists, neighbours, offsets), shape=(n, n))
        (distance 0, an exact copy, is a stored zero).  The k-distance of a row with at least k neighbours — the value a
        k-distance plot sorts to choose DBSCAN's eps — is dists[offsets[i] + k - 1]."""
        n = self.info().n_subjects
        cap = max(int(first_cap), 0)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        while True:
            nb = np.zeros(max(cap, 1), dtype=np.uint32)
            ds = np.zeros(max(cap, 1), dtype=np.uint32) if dists else None
            n_out = C.c_uint64(0)
            rc = lib().smafa_db_self_neighbours(self._h, _opt(max_divergence), _opt(k), offsets.ctypes.data, nb.ctypes.data,
                                                ds.ctypes.data if dists else None, cap, C.byref(n_out))
            if rc == _lib.ERR_CAPACITY:
                cap = int(n_out.value)
                continue
            check(rc)
            return offsets, nb[: n_out.value], (ds[: n_out.value] if dists else None)

    def self_neighbours_launch(self, max_divergence: int, k: Optional[int], d_offsets: int, d_neighbours: int, d_dists: int, cap: int,
                               d_total: int) -> None:
        """device-resident form (smafa_db_self_neighbours_launch): n_subjects + 1 uint64 offsets in d_offsets, up to `cap`
        uint32 neighbours in d_neighbours and distances in d_dists (0: not wanted), the number of entries in *d_total (device
        uint64); SmafaError with code ERR_CAPACITY where they do not fit (offsets and total are written all the same)"""
        check(lib().smafa_db_self_neighbours_launch(self._h, _opt(max_divergence), _opt(k), C.c_void_p(d_offsets) if d_offsets else None,
                                                    C.c_void_p(d_neighbours) if d_neighbours else None,
                                                    C.c_void_p(d_dists) if d_dists else None, cap,
                                                    C.c_void_p(d_total) if d_total else None))

    # ---- minimum spanning forest -----------------------------------------------------------
    def self_forest(self, max_divergence: int) -> tuple[np.ndarray, np.ndarray]:
        """(edges, level_ends) — smafa_db_self_forest: a minimum spanning forest of the graph whose edges are the store's pairs
        within max_divergence, weighted by distance: the merge tree of single linkage.  edges are rows as self_pairs gives them
        (query = a < subject = b, dist = their distance), ordered by (dist, query, subject); level_ends (uint64, max_divergence
        + 1) counts the edges with dist <= t.  The edges [0, level_ends[t]) are acyclic and connect exactly the components of
        self_components(t), so level_ends[t] = n_subjects - n_components[t].  Which of several pairs of equal distance is
        chosen may differ from run to run; the counts and the partitions do not.  forest_linkage makes a linkage matrix of
        them.  The pairs stay on the device."""
        n = self.info().n_subjects
        levels = int(max_divergence) + 1 if max_divergence is not None and 0 <= int(max_divergence) < _lib.NONE else 1
        edges = np.zeros(max(n - 1, 1), dtype=HIT_DTYPE)
        level_ends = np.zeros(levels, dtype=np.uint64)
        check(lib().smafa_db_self_forest(self._h, _opt(max_divergence), edges.ctypes.data, max(n - 1, 0),
                                         level_ends.ctypes.data_as(C.POINTER(C.c_uint64))))
        return edges[: int(level_ends[-1])], level_ends

    def self_forest_launch(self, max_divergence: int, d_edges: int, d_level_ends: int) -> None:
        """device-resident form (smafa_db_self_forest_launch): up to n_subjects - 1 rows of three uint32 in d_edges, ordered by
        distance, max_divergence + 1 level ends in d_level_ends (device uint64 each); the last of them is the number of rows"""
        check(lib().smafa_db_self_forest_launch(self._h, _opt(max_divergence), C.c_void_p(d_edges) if d_edges else None,
                                                C.c_void_p(d_level_ends) if d_level_ends else None))

    # ---- mutual-reachability forest ----------------------------------------------------------
    def self_reach_forest(self, max_divergence: int, min_pts: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(edges, level_ends, cores) — smafa_db_self_reach_forest: a minimum spanning forest under the mutual-reachability
        distance w = max(distance(a, b), core[a], core[b]), the tree HDBSCAN starts from.  cores (uint32, n_subjects) is the
        distance of every row to its (min_pts - 1)-th nearest other row, NONE where fewer are within max_divergence (the row
        is sparse and in no edge).  edges are rows as self_forest gives them with dist = w, ordered by (w, query, subject);
        level_ends (uint64, max_divergence + 1) counts the edges with w <= t.  The edges [0, level_ends[t]) are acyclic and
        connect, among the rows with core <= t, exactly the core rows' clusters of self_density(t, min_pts).  min_pts <= 1 is
        self_forest's contract.  forest_linkage takes the edges as they are."""
        n = self.info().n_subjects
        levels = int(max_divergence) + 1 if max_divergence is not None and 0 <= int(max_divergence) < _lib.NONE else 1
        edges = np.zeros(max(n - 1, 1), dtype=HIT_DTYPE)
        level_ends = np.zeros(levels, dtype=np.uint64)
        cores = np.zeros(n, dtype=np.uint32)
        check(lib().smafa_db_self_reach_forest(self._h, _opt(max_divergence), int(min_pts), edges.ctypes.data, max(n - 1, 0),
                                               level_ends.ctypes.data_as(C.POINTER(C.c_uint64)), cores.ctypes.data if n else None))
        return edges[: int(level_ends[-1])], level_ends, cores

    def self_reach_forest_launch(self, max_divergence: int, min_pts: int, d_edges: int, d_level_ends: int, d_cores: int = 0) -> None:
        """device-resident form (smafa_db_self_reach_forest_launch): up to n_subjects - 1 rows of three uint32 in d_edges, ordered
        by weight, max_divergence + 1 level ends in d_level_ends (device uint64 each), and n_subjects uint32 core distances in
        d_cores (0: not wanted)"""
        check(lib().smafa_db_self_reach_forest_launch(self._h, _opt(max_divergence), int(min_pts), C.c_void_p(d_edges) if d_edges else None,
                                                      C.c_void_p(d_level_ends) if d_level_ends else None,
                                                      C.c_void_p(d_cores) if d_cores else None))

    # ---- stable clusters ----------------------------------------------------------------------
    def self_stable_clusters(self, max_divergence: int, min_pts: int, min_cluster_size: int = 0, joined: bool = False, cores: bool = False):
        """(labels, n_clusters[, joined][, cores]) — smafa_db_self_stable: HDBSCAN's selection over the hierarchy of
        self_reach_forest(max_divergence, min_pts), counted in levels.  labels (uint32, n_subjects) is the smallest subject number
        of the row's chosen cluster, NONE for noise; a cluster holds at least min_cluster_size rows (0: min_pts) and is kept
        where its stability — its size summed over the levels it lives through — is at least what its children's best add up
        to.  joined (uint32) is the level at which the row joined its cluster, cores the reach forest's core distances.  Every
        output is a function of the store and the three parameters alone."""
        n = self.info().n_subjects
        labels = np.zeros(n, dtype=np.uint32)
        since = np.zeros(n, dtype=np.uint32) if joined else None
        core = np.zeros(n, dtype=np.uint32) if cores else None
        count = C.c_uint64(0)
        # (an empty store: a pointer all the same, the call takes no NULL labels)
        check(lib().smafa_db_self_stable(self._h, _opt(max_divergence), int(min_pts), int(min_cluster_size),
                                         labels.ctypes.data if n else C.cast(C.pointer(C.c_uint32(0)), C.c_void_p),
                                         since.ctypes.data if joined and n else None, core.ctypes.data if cores and n else None, n,
                                         C.byref(count)))
        return (labels, int(count.value)) + ((since,) if joined else ()) + ((core,) if cores else ())

    def self_stable_clusters_launch(self, max_divergence: int, min_pts: int, min_cluster_size: int, d_labels: int, d_joined: int = 0,
                                    d_cores: int = 0) -> int:
        """device-resident form (smafa_db_self_stable_launch): n_subjects uint32 labels in d_labels, and where given (0: not
        wanted) as many joined levels in d_joined and core distances in d_cores; -> n_clusters, the one value that crosses to the
        host (the call has waited for its work when it returns)"""
        count = C.c_uint64(0)
        check(lib().smafa_db_self_stable_launch(self._h, _opt(max_divergence), int(min_pts), int(min_cluster_size),
                                                C.c_void_p(d_labels) if d_labels else None, C.c_void_p(d_joined) if d_joined else None,
                                                C.c_void_p(d_cores) if d_cores else None, C.byref(count)))
        return int(count.value)

    # ---- consensus ----------------------------------------------------------------------------
    def cluster_consensus(self, labels, nearest: bool = True, div: bool = True):
        """(ids, sizes, codes[K, L] uint8, nearest, div) — smafa_db_consensus: what each cluster of `labels` looks like.  labels
        (uint32, n_subjects) is what self_components, self_density, self_peaks, self_stable_clusters and the others return: NONE
        or a value below n_subjects per row.  ids (uint32, K) are the distinct labels in ascending order, sizes their member
        counts, codes[k, c] the code most members of cluster k hold at column c (a tie to the smallest code), div[i] the number
        of columns where row i differs from its cluster's consensus (NONE for an unlabelled row), nearest[k] the member with the
        smallest (div, number).  nearest / div not wanted: None in their place.  Asks for K first, then allocates."""
        n, L = self.info().n_subjects, self.info().seq_len
        labels = np.ascontiguousarray(labels, dtype=np.uint32)
        if labels.shape != (n,):
            raise ValueError(f"labels has shape {labels.shape}, the store has {n} subjects")
        # (an empty store: a pointer all the same, the call takes no NULL labels)
        p_labels = labels.ctypes.data if n else C.cast(C.pointer(C.c_uint32(0)), C.c_void_p)
        count = C.c_uint64(0)
        rc = lib().smafa_db_consensus(self._h, p_labels, None, None, None, None, None, 0, C.byref(count))
        if rc != _lib.ERR_CAPACITY:
            check(rc)
        K = int(count.value)
        ids, sizes = np.zeros(K, dtype=np.uint32), np.zeros(K, dtype=np.uint32)
        codes = np.zeros((K, L), dtype=np.uint8)
        near = np.zeros(K, dtype=np.uint32) if nearest else None
        dist = np.full(n, NONE, dtype=np.uint32) if div else None
        if K:  # (K = 0: every row is unlabelled, div is NONE throughout)
            check(lib().smafa_db_consensus(self._h, p_labels, ids.ctypes.data, sizes.ctypes.data, codes.ctypes.data,
                                           near.ctypes.data if nearest else None, dist.ctypes.data if div else None, K, C.byref(count)))
        return ids, sizes, codes, near, dist

    def cluster_consensus_launch(self, d_labels: int, d_ids: int, d_sizes: int, d_codes: int, d_nearest: int = 0, d_div: int = 0,
                                 cap_clusters: int = 0) -> int:
        """device-resident form (smafa_db_consensus_launch): n_subjects uint32 labels in d_labels; cap_clusters uint32 each in
        d_ids, d_sizes and (0: not wanted) d_nearest, cap_clusters x seq_len bytes in d_codes, n_subjects uint32 in d_div (0:
        not wanted); -> K.  SmafaError with code ERR_CAPACITY where cap_clusters < K (its .count holds K): nothing is written.
        The call has waited for its work when it returns."""
        count = C.c_uint64(0)
        ptr = lambda a: C.c_void_p(a) if a else None  # noqa: E731
        rc = lib().smafa_db_consensus_launch(self._h, ptr(d_labels), ptr(d_ids), ptr(d_sizes), ptr(d_codes), ptr(d_nearest), ptr(d_div),
                                             int(cap_clusters), C.byref(count))
        if rc == _lib.ERR_CAPACITY:
            e = _lib.SmafaError(rc, lib().smafa_last_error().decode(errors="replace"))
            e.count = int(count.value)
            raise e
        check(rc)
        return int(count.value)

    # ---- abundance table ------------------------------------------------------------------------
    def assign(self, query_codes, max_divergence: int, labels=None, samples=None, n_samples: Optional[int] = None, weights=None,
               per_read: bool = True, subject_counts: bool = False) -> Assigned:
        """(entries, subject, dist, subject_counts, totals) — smafa_db_assign: every read assigned to the subject at the smallest
        distance <= max_divergence (a tie to the smaller number; NONE where there is none) and counted.  labels (uint32,
        n_subjects; None: a subject's label is its own number), samples (uint32 per read; None: sample 0), n_samples (default:
        max(samples) + 1), weights (uint32 per read; None: 1).  entries (TABLE_DTYPE) holds one {label, sample, count} per (label,
        sample) with a read of weight > 0, ordered by (label, sample), NONE last; subject, dist (uint32 per read; per_read=False:
        None); subject_counts (uint64 per subject, where asked for); totals = [entries, assigned weight, unassigned weight, reads
        with a sample number out of range].  Grows the entry buffer and calls again on ERR_CAPACITY."""
        q = np.ascontiguousarray(query_codes, dtype=np.uint8).reshape(-1, self.seq_len)
        m, n = q.shape[0], len(self)
        labels = _given(labels, n, "labels")
        samples, weights, n_samples = _per_read(samples, weights, n_samples, m)
        subject = np.full(m, NONE, dtype=np.uint32) if per_read else None
        dist = np.full(m, NONE, dtype=np.uint32) if per_read else None
        counts = np.zeros(n, dtype=np.uint64) if subject_counts else None
        totals = np.zeros(4, dtype=np.uint64)
        entries = _with_entries(m, totals, lambda e, cap: lib().smafa_db_assign(
            self._h, _ptr(q), m, _opt(max_divergence), _ptr(labels), _ptr(samples, True), n_samples, _ptr(weights, True), _ptr(subject),
            _ptr(dist), _ptr(counts), e, cap, totals.ctypes.data))
        return Assigned(entries, subject, dist, counts, totals)

    def assign_launch(self, qset: QuerySet, max_divergence: int, d_labels: int, d_samples: int, n_samples: int, d_weights: int,
                      d_subject: int, d_dist: int, d_subject_counts: int, d_entries: int, cap: int, d_totals: int) -> None:
        """device-resident form (smafa_db_assign_launch): n_subjects uint32 labels in d_labels, one uint32 per read in d_samples and
        d_weights (0: none given); one uint32 per read to d_subject and d_dist, n_subjects uint64 to d_subject_counts (0: not
        wanted); the first cap entries in table order to d_entries (16 B each; 0 with cap 0: counted only); four uint64 to
        d_totals.  The call has waited for its work when it returns."""
        ptr = lambda a: C.c_void_p(a) if a else None  # noqa: E731
        check(lib().smafa_db_assign_launch(self._h, qset._h, _opt(max_divergence), ptr(d_labels), ptr(d_samples), int(n_samples),
                                           ptr(d_weights), ptr(d_subject), ptr(d_dist), ptr(d_subject_counts), ptr(d_entries), int(cap),
                                           ptr(d_totals)))

    # ---- classification: the LCA of the best hits -------------------------------------------------
    def classify(self, query_codes, max_divergence: int, lineage, slack: int = 0, samples=None, n_samples: Optional[int] = None,
                 weights=None) -> Classified:
        """(entries, subject, dist, taxon, depth, ties, totals) — smafa_db_classify: every read given the lowest common ancestor of
        the lineages of its best hits, the subjects within its smallest distance + slack (all within max_divergence), and counted.
        lineage (uint32, n_subjects x n_ranks, 1 <= n_ranks <= 16): the taxon id of each subject at each rank, rank 0 the most
        general, NONE from the rank at which a subject is not classified.  samples, n_samples, weights: as for assign.  entries
        (TABLE_DTYPE, label = the taxon) holds one {taxon, sample, count} per (taxon, sample) with a read of weight > 0, ordered by
        (taxon, sample), TAXON_ROOT behind every taxon, NONE last; subject, dist (assign's), taxon, depth (the number of ranks the
        best hits share; NONE for an unassigned read) and ties (the number of best hits) are uint32 per read; totals = [entries,
        assigned weight, unassigned weight, reads with a sample number out of range, weight on the root, reads with ties > 1].
        Grows the entry buffer and calls again on ERR_CAPACITY."""
        q = np.ascontiguousarray(query_codes, dtype=np.uint8).reshape(-1, self.seq_len)
        m, n = q.shape[0], len(self)
        lineage = np.ascontiguousarray(lineage, dtype=np.uint32)
        if lineage.ndim != 2 or lineage.shape[0] != n:
            raise ValueError(f"lineage has shape {lineage.shape}, expected ({n}, n_ranks)")
        samples, weights, n_samples = _per_read(samples, weights, n_samples, m)
        subject, dist, taxon, depth = (np.full(m, NONE, dtype=np.uint32) for _ in range(4))
        ties = np.zeros(m, dtype=np.uint32)
        totals = np.zeros(6, dtype=np.uint64)
        entries = _with_entries(m, totals, lambda e, cap: lib().smafa_db_classify(
            self._h, _ptr(q), m, _opt(max_divergence), int(slack), _ptr(lineage), int(lineage.shape[1]), _ptr(samples, True), n_samples,
            _ptr(weights, True), _ptr(subject), _ptr(dist), _ptr(taxon), _ptr(depth), _ptr(ties), e, cap, totals.ctypes.data))
        return Classified(entries, subject, dist, taxon, depth, ties, totals)

    def classify_launch(self, qset: QuerySet, max_divergence: int, slack: int, d_lineage: int, n_ranks: int, d_samples: int, n_samples: int,
                        d_weights: int, d_subject: int, d_dist: int, d_taxon: int, d_depth: int, d_ties: int, d_entries: int, cap: int,
                        d_totals: int) -> None:
        """device-resident form (smafa_db_classify_launch): n_subjects x n_ranks uint32 in d_lineage, one uint32 per read in d_samples
        and d_weights (0: none given); one uint32 per read to d_subject, d_dist, d_taxon, d_depth and d_ties (0: not wanted); the
        first cap entries in table order to d_entries (16 B each; 0 with cap 0: counted only); six uint64 to d_totals.  The call
        has waited for its work when it returns."""
        ptr = lambda a: C.c_void_p(a) if a else None  # noqa: E731
        check(lib().smafa_db_classify_launch(self._h, qset._h, _opt(max_divergence), int(slack), ptr(d_lineage), int(n_ranks), ptr(d_samples),
                                             int(n_samples), ptr(d_weights), ptr(d_subject), ptr(d_dist), ptr(d_taxon), ptr(d_depth), ptr(d_ties),
                                             ptr(d_entries), int(cap), ptr(d_totals)))

    # ---- rows out of the store: a subset of it as a new store, its sequences back ---------------------
    def subset(self, keep, invert: bool = False) -> tuple["SubjectStore", np.ndarray]:
        """(store, old_of_new) — smafa_db_subset: the kept subjects as a NEW store on the same device, renumbered 0 .. k-1 in
        ascending old number; old_of_new[new] = old (uint32).  keep: a boolean or integer array of length len(self), non-zero:
        keep; invert: the array lists the rows to DROP (the flags of self_chimeras as they are).  The result has this store's
        layout and plane count and no index; it answers every call as a fresh store with push(codes[keep]) would.  This store
        is not modified."""
        n = len(self)
        k = np.ascontiguousarray(np.asarray(keep).reshape(-1) != 0, dtype=np.uint32)
        if k.shape[0] != n:
            raise ValueError(f"keep has {k.shape[0]} entries, the store has {n} subjects")
        old_of_new = np.zeros(n, dtype=np.uint32)
        sub = SubjectStore.__new__(SubjectStore)
        sub._h = C.c_void_p()
        sub.seq_len, sub.alphabet = self.seq_len, self.alphabet
        kept = C.c_uint64(0)
        check(lib().smafa_db_subset(self._h, _ptr(k) if n else None, 1 if invert else 0, C.byref(sub._h), _ptr(old_of_new) if n else None, n,
                                    C.byref(kept)))
        return sub, old_of_new[:kept.value].copy()

    def subset_launch(self, d_keep: int, invert: bool = False, d_old_of_new: int = 0) -> tuple["SubjectStore", int]:
        """device-resident form (smafa_db_subset_launch): len(self) uint32 in d_keep, len(self) uint32 of room in d_old_of_new (0: not
        wanted) -> (store, k).  The call has waited for its work when it returns."""
        ptr = lambda a: C.c_void_p(a) if a else None  # noqa: E731
        sub = SubjectStore.__new__(SubjectStore)
        sub._h = C.c_void_p()
        sub.seq_len, sub.alphabet = self.seq_len, self.alphabet
        kept = C.c_uint64(0)
        check(lib().smafa_db_subset_launch(self._h, ptr(d_keep), 1 if invert else 0, C.byref(sub._h), ptr(d_old_of_new), C.byref(kept)))
        return sub, int(kept.value)

    def rows(self, subjects=None, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """(m, seq_len) uint8 — smafa_db_rows: the code rows of the listed subjects (any order, repeats allowed), or of the range
        first .. first + count - 1 (count None: to the end of the store), unpacked from the bit-planes on the device: the bytes
        push() was given."""
        if subjects is not None:
            s = np.ascontiguousarray(np.asarray(subjects).reshape(-1), dtype=np.uint32)
            m = s.shape[0]
        else:
            s, m = None, (len(self) - int(first) if count is None else int(count))
            if m < 0:
                raise ValueError(f"first is {first}, the store has {len(self)} subjects")
        out = np.zeros((m, self.seq_len), dtype=np.uint8)
        check(lib().smafa_db_rows(self._h, _ptr(s) if m and s is not None else None, int(first), m, _ptr(out) if m else None))
        return out

    def rows_launch(self, d_subjects: int, first: int, m: int, d_codes: int) -> None:
        """device-resident form (smafa_db_rows_launch): m uint32 subject numbers in d_subjects (0: the range first .. first + m - 1),
        m x seq_len bytes to d_codes; a listed number >= len(self) gives a row of 0xff.  The call has waited for its work when it
        returns."""
        ptr = lambda a: C.c_void_p(a) if a else None  # noqa: E731
        check(lib().smafa_db_rows_launch(self._h, ptr(d_subjects), int(first), int(m), ptr(d_codes)))

    def last_call_stats(self) -> dict:
        ms, n, k = C.c_float(0), C.c_uint32(0), C.c_uint32(0)
        check(lib().smafa_last_call_stats(self._h, C.byref(ms), C.byref(n), C.byref(k)))
        return {"kernel_ms": ms.value, "launches": n.value, "scans": k.value}

    def launch_device(self) -> tuple[int, int]:
        """(HIP device current on the launching thread at the last scan launch, launches issued off the handle's device)"""
        dev, off = C.c_int(-1), C.c_uint64(0)
        check(lib().smafa_launch_device(self._h, C.byref(dev), C.byref(off)))
        return dev.value, off.value

    def sync(self) -> None:
        check(lib().smafa_sync(self._h))

    def last_scan_ms(self) -> tuple[float, int]:
        ms, n = C.c_float(0), C.c_uint32(0)
        check(lib().smafa_last_scan_ms(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def last_scan_plan(self) -> dict:
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(lib().smafa_last_scan_plan(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"filter_plane_resident": bool(a.value), "tiles_per_wave": b.value, "query_blocks": c.value}

    def last_scan_kernel(self) -> str:
        buf = C.create_string_buffer(128)
        check(lib().smafa_last_scan_kernel(self._h, buf, 128))
        return buf.value.decode()

    def last_call_kernels(self) -> list[str]:
        """every distinct scan-family instantiation the most recent scan / get_distances call launched, in first-launch
        order (smafa_last_call_kernels)"""
        cap = 4096
        while True:
            buf = C.create_string_buffer(cap)
            rc = lib().smafa_last_call_kernels(self._h, buf, cap)
            if rc == _lib.ERR_CAPACITY:
                cap *= 4
                continue
            check(rc)
            return buf.value.decode().split("\n") if buf.value else []

    def close(self):
        if self._h:
            lib().smafa_db_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SubjectGroup:
    """One WindowSet replicated over several GPUs behind one handle (smafa_group_*): `scan` has the contract of
    SubjectStore.scan, the batch cut into contiguous blocks, one per device (the loop of src/lib.rs:232-318 sharded)."""

    def __init__(self, seq_len: int, alphabet: int = ALPHABET_NT, devices=(0,)):
        self._h = C.c_void_p()
        self.seq_len, self.alphabet = int(seq_len), alphabet
        arr = (C.c_int * len(devices))(*[int(d) for d in devices])
        check(lib().smafa_group_create(C.byref(self._h), arr, len(devices), alphabet, self.seq_len))

    @classmethod
    def load(cls, path: str, devices=(0,)) -> "SubjectGroup":
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        arr = (C.c_int * len(devices))(*[int(d) for d in devices])
        check(lib().smafa_group_load(C.byref(self._h), arr, len(devices), os.fsencode(path)))
        info = _lib.DbInfo()
        check(lib().smafa_db_info(lib().smafa_group_member(self._h, 0), C.byref(info)))
        self.seq_len, self.alphabet = int(info.seq_len), int(info.alphabet)
        return self

    def __len__(self) -> int:
        return lib().smafa_group_size(self._h)

    def build_index(self, max_divergence: int) -> list:
        """smafa_group_build_index: every replica builds its block index; -> per member smafa_index_info()"""
        check(lib().smafa_group_build_index(self._h, int(max_divergence)))
        out = []
        for g in range(len(self)):
            info = _lib.IndexInfo()
            check(lib().smafa_index_info(lib().smafa_group_member(self._h, g), C.byref(info)))
            out.append({k: getattr(info, k) for k, _ in _lib.IndexInfo._fields_})
        return out

    def members(self):
        """per member: (smafa_db_info().device, device current at its last scan launch, launches off its device)"""
        out = []
        for g in range(len(self)):
            h = lib().smafa_group_member(self._h, g)
            info = _lib.DbInfo()
            check(lib().smafa_db_info(h, C.byref(info)))
            dev, off = C.c_int(-1), C.c_uint64(0)
            check(lib().smafa_launch_device(h, C.byref(dev), C.byref(off)))
            out.append((int(info.device), dev.value, off.value))
        return out

    def push(self, codes: np.ndarray) -> None:
        c = np.ascontiguousarray(codes, dtype=np.uint8)
        if c.ndim != 2 or c.shape[1] != self.seq_len:
            raise SmafaPanic(_lib.ERR_PANIC, "WindowSet seq length is %d, got a new sequence of length %d"
                             % (self.seq_len, c.shape[-1]))
        check(lib().smafa_group_append(self._h, c.ctypes.data, c.shape[0]))

    def scan(self, query_codes: np.ndarray, max_divergence: Optional[int] = None,
             max_num_hits: Optional[int] = None, cap: int = 1 << 16) -> np.ndarray:
        q = np.ascontiguousarray(query_codes, dtype=np.uint8)
        assert q.ndim == 2 and q.shape[1] == self.seq_len
        while True:
            out = np.zeros(max(cap, 1), dtype=HIT_DTYPE)
            n_out = C.c_uint64(0)
            rc = lib().smafa_group_scan_hits(self._h, q.ctypes.data, q.shape[0], _opt(max_divergence), _opt(max_num_hits),
                                             out.ctypes.data, cap, C.byref(n_out))
            if rc == _lib.ERR_CAPACITY:
                cap = int(n_out.value)
                continue
            check(rc)
            return out[: n_out.value]

    def close(self):
        if self._h:
            lib().smafa_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def select_rows(hits: np.ndarray, n_queries: int, n_subjects: int, subject_codes: Optional[np.ndarray], seq_len: int,
                max_divergence: Optional[int], max_num_hits: Optional[int],
                limit_per_sequence: Optional[int]) -> np.ndarray:
    """Selection rules of src/lib.rs:241-315 over an ordered hit list."""
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    cap = max(len(hits), 1)
    rows = np.zeros(cap, dtype=HIT_DTYPE)
    n_rows = C.c_uint64(0)
    codes_ptr = None
    if subject_codes is not None:
        subject_codes = np.ascontiguousarray(subject_codes, dtype=np.uint8)
        codes_ptr = subject_codes.ctypes.data
    check(lib().smafa_select_rows(hits.ctypes.data, len(hits), n_queries, n_subjects, codes_ptr, seq_len,
                                  _opt(max_divergence), _opt(max_num_hits), _opt(limit_per_sequence),
                                  rows.ctypes.data, cap, C.byref(n_rows)))
    return rows[: n_rows.value]


def read_db(path: str) -> tuple[int, np.ndarray]:
    """DB file -> (alphabet, code rows)."""
    alphabet, ptr, n, L = C.c_int(0), C.c_void_p(), C.c_uint64(0), C.c_uint32(0)
    check(lib().smafa_dbfile_read(os.fsencode(path), C.byref(alphabet), C.byref(ptr), C.byref(n), C.byref(L)))
    try:
        size = n.value * L.value
        arr = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(max(size, 1),))[:size].copy()
    finally:
        lib().smafa_free(ptr)
    return alphabet.value, arr.reshape(n.value, L.value)


def load_fastx(path: str, alphabet: int = ALPHABET_NT) -> np.ndarray:
    """FASTA/FASTQ(+gzip) of equal-length records -> code rows (needletail + from_bytes, src/lib.rs:221,235)."""
    ptr, n, L = C.c_void_p(), C.c_uint64(0), C.c_uint32(0)
    check(lib().smafa_fastx_load(os.fsencode(path), alphabet, C.byref(ptr), C.byref(n), C.byref(L)))
    try:
        size = n.value * L.value
        arr = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(max(size, 1),))[:size].copy()
    finally:
        lib().smafa_free(ptr)
    return arr.reshape(n.value, L.value)


def load_fastx_partial(path: str, alphabet: int = ALPHABET_NT):
    """-> (code rows in front of the first offending record, None or the SmafaError that record raises)"""
    ptr, n, L, pending = C.c_void_p(), C.c_uint64(0), C.c_uint32(0), C.c_int(0)
    check(lib().smafa_fastx_load_partial(os.fsencode(path), alphabet, C.byref(ptr), C.byref(n), C.byref(L), C.byref(pending)))
    err = None
    if pending.value != _lib.OK:
        msg = lib().smafa_last_error().decode(errors="replace")
        err = (SmafaPanic if pending.value == _lib.ERR_PANIC else SmafaError)(pending.value, msg)
    try:
        size = n.value * L.value
        arr = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(max(size, 1),))[:size].copy()
    finally:
        lib().smafa_free(ptr)
    return arr.reshape(n.value, L.value), err


def load_fastx_part(path: str, part: int, parts: int, alphabet: int = ALPHABET_NT):
    """-> (code rows of the records that start in this part's byte range, pending error or None, usable)"""
    ptr, n, L, pending, usable = C.c_void_p(), C.c_uint64(0), C.c_uint32(0), C.c_int(0), C.c_int(0)
    check(lib().smafa_fastx_load_part(os.fsencode(path), alphabet, part, parts, C.byref(ptr), C.byref(n), C.byref(L),
                                      C.byref(pending), C.byref(usable)))
    err = None
    if pending.value != _lib.OK:
        msg = lib().smafa_last_error().decode(errors="replace")
        err = (SmafaPanic if pending.value == _lib.ERR_PANIC else SmafaError)(pending.value, msg)
    try:
        size = n.value * L.value
        arr = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(max(size, 1),))[:size].copy() if ptr else np.zeros(0, np.uint8)
    finally:
        lib().smafa_free(ptr)
    return arr.reshape(n.value, L.value) if L.value else arr.reshape(0, 0), err, bool(usable.value)


def write_db(path: str, codes: np.ndarray, alphabet: int = ALPHABET_NT) -> None:
    c = np.ascontiguousarray(codes, dtype=np.uint8)
    check(lib().smafa_dbfile_write(os.fsencode(path), alphabet, c.ctypes.data, c.shape[0], c.shape[1]))


def write_rows(rows: np.ndarray, subject_codes: np.ndarray, alphabet: int, out_fd: int = 1, query_offset: int = 0) -> None:
    """TSV rows of `query` (src/lib.rs:292,310) for an ordered row list, written to out_fd."""
    rows = np.ascontiguousarray(rows, dtype=HIT_DTYPE)
    subject_codes = np.ascontiguousarray(subject_codes, dtype=np.uint8)
    n, L = subject_codes.shape
    check(lib().smafa_write_rows(rows.ctypes.data, len(rows), subject_codes.ctypes.data, n, L, alphabet, query_offset, out_fd))


# ------------------------------------------------------------------ the crate's pub fns
def makedb(subject_fasta: str, db_path: str, alphabet: int = ALPHABET_NT) -> None:
    """makedb(subject_fasta, db_path) — src/lib.rs:137-165."""
    check(lib().smafa_makedb(os.fsencode(subject_fasta), os.fsencode(db_path), alphabet))


def makedb_packed(subject_fasta: str, db_path: str, alphabet: int = ALPHABET_NT, device: int = 0) -> None:
    """makedb writing the packed store file; packed on GPU `device`, or by host threads when device < 0 or there is no GPU."""
    check(lib().smafa_makedb_packed(os.fsencode(subject_fasta), os.fsencode(db_path), alphabet, device))


def query(db_path: str, query_fasta: str, max_divergence: Optional[int] = None, max_num_hits: Optional[int] = None,
          limit_per_sequence: Optional[int] = None, out_fd: int = 1, device: int = 0, devices=None) -> None:
    """query(db_path, query_fasta, max_divergence, max_num_hits, limit_per_sequence) — src/lib.rs:198-325.
    `devices`: a list of GPU ordinals (entries may repeat) = one process, one handle and host thread per entry."""
    if devices is not None:
        arr = (C.c_int * len(devices))(*[int(d) for d in devices])
        check(lib().smafa_query_multi(os.fsencode(db_path), os.fsencode(query_fasta), _opt(max_divergence),
                                      _opt(max_num_hits), _opt(limit_per_sequence), out_fd, arr, len(devices)))
        return
    check(lib().smafa_query(os.fsencode(db_path), os.fsencode(query_fasta), _opt(max_divergence), _opt(max_num_hits),
                            _opt(limit_per_sequence), out_fd, device))


def cluster(input_fasta: str, max_divergence: int, out_fd: int = 1, device: int = 0,
            alphabet: int = ALPHABET_NT, devices=None) -> None:
    """cluster(input_fasta, max_divergence, print_stream) — src/cluster.rs:13-94.
    `devices`: a list of GPU ordinals (entries may repeat) = one process, one host thread and centroid replica per entry."""
    if devices is not None:
        arr = (C.c_int * len(devices))(*[int(d) for d in devices])
        check(lib().smafa_cluster_multi(os.fsencode(input_fasta), int(max_divergence), out_fd, arr, len(devices), alphabet))
        return
    check(lib().smafa_cluster(os.fsencode(input_fasta), int(max_divergence), out_fd, device, alphabet))


def count(paths, out_fd: int = 1) -> None:
    """count(paths) — src/lib.rs:378-398."""
    arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
    check(lib().smafa_count(arr, len(paths), out_fd))


def pairs(db_path: str, max_divergence: int, out_fd: int = 1, device: int = 0) -> None:
    """`smafa pairs`: every pair i < j of the DB file's own subjects within max_divergence, "i\\tj\\tdist" lines to out_fd."""
    check(lib().smafa_pairs(os.fsencode(db_path), _opt(max_divergence), out_fd, device))


def pairs_since(db_path: str, first_row: int, max_divergence: int, out_fd: int = 1, device: int = 0) -> None:
    """`smafa pairs --since ROW`: the lines of `pairs` whose larger subject number is >= first_row."""
    check(lib().smafa_pairs_since(os.fsencode(db_path), int(first_row), _opt(max_divergence), out_fd, device))


def components(db_path: str, max_divergence: int, out_fd: int = 1, device: int = 0) -> None:
    """`smafa components`: "i\\tlabel" per subject of the DB file, label = the smallest subject number of i's single-linkage
    component at max_divergence, to out_fd."""
    check(lib().smafa_components(os.fsencode(db_path), _opt(max_divergence), out_fd, device))


def density(db_path: str, max_divergence: int, min_pts: int, out_fd: int = 1, device: int = 0) -> None:
    """`smafa density`: "i\\tlabel\\tdegree" per subject of the DB file — its density-cluster label at max_divergence and
    min_pts (-1 for noise) and the number of other subjects within the bound of it — to out_fd."""
    check(lib().smafa_density(os.fsencode(db_path), _opt(max_divergence), int(min_pts), out_fd, device))


def neighbours(db_path: str, max_divergence: int, max_num_hits: Optional[int] = None, out_fd: int = 1, device: int = 0) -> None:
    """`smafa neighbours`: "i\\tj\\tdist" per subject i of the DB file and neighbour j within max_divergence, nearest first, at
    most max_num_hits per i (smafa_db_self_neighbours), to out_fd."""
    check(lib().smafa_neighbours(os.fsencode(db_path), _opt(max_divergence), _opt(max_num_hits), out_fd, device))


def peaks(db_path: str, max_divergence: int, radius: Optional[int] = 0, out_fd: int = 1, device: int = 0) -> None:
    """`smafa peaks`: "i\\tlabel\\tparent\\tweight" per subject of the DB file — its abundance-peak label and parent at
    max_divergence and its weight at `radius` (smafa_db_self_peaks) — to out_fd."""
    check(lib().smafa_peaks(os.fsencode(db_path), _opt(max_divergence), _opt(radius), out_fd, device))


def peaks_weighted(db_path: str, max_divergence: int, weights_path: str, radius: Optional[int] = 0, out_fd: int = 1, device: int = 0) -> None:
    """`smafa peaks --sizes`: the lines of peaks(), the weights read from weights_path ("i\\tweight" lines, "-": stdin) and summed
    within `radius` (smafa_db_self_peaks_weighted)"""
    check(lib().smafa_peaks_weighted(os.fsencode(db_path), _opt(max_divergence), _opt(radius), os.fsencode(weights_path), out_fd, device))


def chimeras(db_path: str, max_divergence: int, min_fold: int = 2, radius: Optional[int] = 0, weights_path: Optional[str] = None,
             out_fd: int = 1, device: int = 0) -> None:
    """`smafa chimeras`: "i\\tflag\\tleft_parent\\tleft_len\\tright_parent\\tright_len\\tweight" per subject of the DB file
    (smafa_db_self_chimeras; -1 for no parent), the weights counted at `radius` or read from weights_path ("i\\tweight" lines,
    "-": stdin), to out_fd."""
    check(lib().smafa_chimeras(os.fsencode(db_path), _opt(max_divergence), _opt(radius), int(min_fold),
                               os.fsencode(weights_path) if weights_path is not None else None, out_fd, device))


def component_levels(db_path: str, max_divergence: int, out_fd: int = 1, device: int = 0) -> None:
    """`smafa components --levels`: "i\\tlabel_0\\t...\\tlabel_N" per subject of the DB file, label_t = its label at bound t, to
    out_fd."""
    check(lib().smafa_component_levels(os.fsencode(db_path), _opt(max_divergence), out_fd, device))


def forest(db_path: str, max_divergence: int, out_fd: int = 1, device: int = 0) -> None:
    """`smafa forest`: "a\\tb\\tdist" per edge of a minimum spanning forest of the DB file's subjects up to max_divergence
    (smafa_db_self_forest), ordered by (dist, a, b), to out_fd."""
    check(lib().smafa_forest(os.fsencode(db_path), _opt(max_divergence), out_fd, device))


def reach_forest(db_path: str, max_divergence: int, min_pts: int, cores: bool = False, out_fd: int = 1, device: int = 0) -> None:
    """`smafa forest --min-pts M`: "a\\tb\\tw" per edge of the mutual-reachability forest of the DB file's subjects up to
    max_divergence at min_pts (smafa_db_self_reach_forest), ordered by (w, a, b), to out_fd — or, with cores, "i\\tcore" per
    subject, -1 for a sparse row."""
    check(lib().smafa_reach_forest(os.fsencode(db_path), _opt(max_divergence), int(min_pts), 1 if cores else 0, out_fd, device))


def stable_clusters(db_path: str, max_divergence: int, min_pts: int, min_cluster_size: int = 0, joined: bool = False, out_fd: int = 1,
                    device: int = 0) -> None:
    """`smafa stable`: "i\\tlabel" per subject of the DB file (smafa_db_self_stable), -1 for noise, to out_fd — with joined a third
    column, the level at which the subject joined its cluster."""
    check(lib().smafa_stable(os.fsencode(db_path), _opt(max_divergence), int(min_pts), int(min_cluster_size), 1 if joined else 0, out_fd, device))


def consensus(db_path: str, labels_path: str, out_fd: int = 1, device: int = 0) -> None:
    """`smafa consensus`: "label\\tsize\\tnearest\\tmax_div\\tSEQUENCE" per cluster of the labels file ("i\\tlabel" per subject of the
    DB file, as the label verbs print it; "-": stdin) in ascending label order (smafa_db_consensus), to out_fd."""
    check(lib().smafa_consensus(os.fsencode(db_path), os.fsencode(labels_path), out_fd, device))


def table(db_path: str, query_fasta: str, max_divergence: int, labels_path: Optional[str] = None, samples_path: Optional[str] = None,
          weights_path: Optional[str] = None, per_read: bool = False, per_sequence: bool = False, out_fd: int = 1, device: int = 0) -> None:
    """`smafa table`: "label<TAB>sample<TAB>count" lines of the reads of query_fasta against the DB (smafa_table); per_read:
    "read<TAB>subject<TAB>dist" lines; per_sequence: "i<TAB>count" lines, what `chimeras --weights` reads"""
    enc = lambda p: os.fsencode(p) if p is not None else None  # noqa: E731
    check(lib().smafa_table(os.fsencode(db_path), os.fsencode(query_fasta), _opt(max_divergence), enc(labels_path), enc(samples_path),
                            enc(weights_path), 1 if per_read else 0, 1 if per_sequence else 0, out_fd, device))


def classify(db_path: str, query_fasta: str, max_divergence: int, taxonomy_path: str, slack: int = 0, samples_path: Optional[str] = None,
             weights_path: Optional[str] = None, per_read: bool = False, out_fd: int = 1, device: int = 0) -> None:
    """`smafa classify`: "lineage<TAB>sample<TAB>count" lines of the reads of query_fasta against the DB under the taxonomy file
    (smafa_classify); per_read: "read<TAB>subject<TAB>dist<TAB>ties<TAB>depth<TAB>lineage" lines"""
    enc = lambda p: os.fsencode(p) if p is not None else None  # noqa: E731
    check(lib().smafa_classify(os.fsencode(db_path), os.fsencode(query_fasta), _opt(max_divergence), int(slack), enc(taxonomy_path),
                               enc(samples_path), enc(weights_path), 1 if per_read else 0, out_fd, device))


def subset(db_path: str, out_path: str, keep_path: Optional[str] = None, drop_path: Optional[str] = None, out_fd: int = 1, device: int = 0) -> None:
    """`smafa subset`: the sequences of the DB listed in keep_path, or all but the ones listed in drop_path ("-": stdin), saved to
    out_path as a packed store; "new<TAB>old" lines to out_fd (smafa_subset)"""
    enc = lambda p: os.fsencode(p) if p is not None else None  # noqa: E731
    check(lib().smafa_subset(os.fsencode(db_path), enc(keep_path), enc(drop_path), os.fsencode(out_path), out_fd, device))


def forest_linkage(edges, n: int, max_divergence: int) -> np.ndarray:
    """The linkage matrix of a forest, numpy only: (n - 1, 4) float64 rows [id_a, id_b, height, size] in the layout
    scipy.cluster.hierarchy documents — the rows 0 .. n - 1 are clusters 0 .. n - 1, merge k makes cluster n + k, id_a < id_b
    are the two clusters it joins, size the rows of the new one.  `edges` (SubjectStore.self_forest's rows, or an (m, 3) array
    of a, b, dist) are taken in the order given, each at height dist; an edge inside one cluster is an error.  Trees left
    apart at the bound — no pair within max_divergence joins them — are then merged at height max_divergence + 1, in order
    of their smallest member: a cut at any height <= max_divergence never sees those merges."""
    n = int(n)
    if isinstance(edges, np.ndarray) and edges.dtype.names:
        a, b, d = (np.asarray(edges[k]).reshape(-1) for k in ("query", "subject", "dist"))
    else:
        rows = np.asarray(edges).reshape(-1, 3)
        a, b, d = rows[:, 0], rows[:, 1], rows[:, 2]
    parent = list(range(n))                # union-find over the rows
    cluster = list(range(n))               # root row -> the id of its cluster
    size = [1] * n
    smallest = list(range(n))              # root row -> the smallest row of its cluster
    out = np.zeros((max(n - 1, 0), 4), dtype=np.float64)
    merges = 0

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def merge(ra, rb, height):
        nonlocal merges
        if size[ra] < size[rb]:
            ra, rb = rb, ra
        parent[rb] = ra
        out[merges] = (min(cluster[ra], cluster[rb]), max(cluster[ra], cluster[rb]), height, size[ra] + size[rb])
        size[ra] += size[rb]
        smallest[ra] = min(smallest[ra], smallest[rb])
        cluster[ra] = n + merges
        merges += 1

    for x, y, h in zip(a.tolist(), b.tolist(), d.tolist()):
        if not (0 <= x < n and 0 <= y < n):
            raise ValueError("edge (%d, %d) names a row outside 0 .. %d" % (x, y, n - 1))
        rx, ry = find(x), find(y)
        if rx == ry:
            raise ValueError("edge (%d, %d) closes a cycle: the edges are no forest" % (x, y))
        merge(rx, ry, float(h))
    roots = sorted({find(i) for i in range(n)}, key=lambda r: smallest[r])
    for r in roots[1:]:
        merge(find(roots[0]), r, float(int(max_divergence) + 1))
    return out
