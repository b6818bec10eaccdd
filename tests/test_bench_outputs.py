"""bench.py's arguments and --dump-outputs writer, without a GPU: a plain run is the default, --steps is checked, and the rows of the
last timed step land as float64 arrays within the size limit (a fixed sample beyond it, the same on every run)."""
import os

import numpy as np
import pytest

import bench


def test_plain_run_is_the_default():
    a = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None and a.full_record is None
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def _load(d):
    return {k: np.load(os.path.join(d, k + ".npy")) for k in ("query", "subject", "dist", "count")}


def test_dump_writes_every_row_as_float64(tmp_path):
    rows = np.array([[0, 7, 0], [0, 3, 2], [5, 4_000_000_001, 1]], dtype=np.uint32)
    bench.dump_outputs(str(tmp_path / "d"), rows, 3)
    out = _load(str(tmp_path / "d"))
    assert all(a.dtype == np.float64 for a in out.values())
    assert out["query"].tolist() == [0, 0, 5] and out["subject"].tolist() == [7, 3, 4_000_000_001] and out["dist"].tolist() == [0, 2, 1]
    assert out["count"].tolist() == [3]
    bench.dump_outputs(str(tmp_path / "e"), np.zeros((0, 3), dtype=np.uint32), 0)
    assert len(_load(str(tmp_path / "e"))["query"]) == 0


def test_dump_beyond_the_limit_is_a_fixed_ordered_sample(tmp_path):
    rng = np.random.default_rng(1)
    rows = bench.sorted_rows(rng.integers(0, 1000, size=(5000, 3)).astype(np.uint32))
    limit = 4096 + 24 * 1000
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), rows, 5000, limit=limit)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert len(a["query"]) == 1000 and a["count"].tolist() == [5000]
    assert sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a"))) <= limit
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    got = np.stack([a["query"], a["subject"], a["dist"]], axis=1).astype(np.uint32)
    assert bench.sorted_rows(got).tobytes() == got.tobytes()  # kept in the reference's order
    whole = {r.tobytes() for r in rows}
    assert all(r.tobytes() in whole for r in got)
