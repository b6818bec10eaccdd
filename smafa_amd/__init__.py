"""smafa_amd — MI355X-native engine for smafa's fixed-length Hamming scan (query / cluster).

HIP kernels for gfx950 behind the C ABI of ``include/smafa_amd.h``; this package is the ctypes
mirror of the reference crate's interface for that path.  No CPU fallback.
"""
from ._lib import ALPHABET_AA, ALPHABET_NT, NONE, SmafaError, SmafaPanic, build  # noqa: F401
from .api import (HIT_DTYPE, TABLE_DTYPE, TAXON_ROOT, Assigned, Chimeras, Classified, QuerySet, TableEntry, SubjectGroup, SubjectStore, build_id, chimeras, cluster, hbm_read_probe, count, decode, device_count, encode,  # noqa: F401
                  classify, component_levels, components, consensus, density, encode_rows, forest, forest_linkage, load_fastx, load_fastx_part, makedb, makedb_packed, neighbours, pairs, pairs_since, peaks, peaks_weighted, query, reach_forest, read_db, select_rows, stable_clusters, subset, table, write_db, write_rows)
