"""bench.py --dump-outputs (host side only): every array is written in float64, aggregates are decoded by
their type, an output over the size limit is cut to the same seeded rows on every run, and a small one is
written whole."""
import os

import numpy as np

import bench
from siddhi_amd import abi


def _arrays(n, flushes):
    r = np.random.default_rng(7)
    v = r.normal(size=n)
    v[0] = np.nan
    cnt = r.integers(1, 50, n)
    return {"flush_offsets": np.linspace(0, n, flushes + 1).astype(np.int64),
            "flush_clock": np.arange(flushes, dtype=np.int64) * 1000 + 1_700_000_000_000,
            "val_types": np.array([abi.LONG, abi.DOUBLE], np.int32),
            "ts": np.arange(n, dtype=np.int64) + 1_700_000_000_000, "expired": np.zeros(n, np.uint8),
            "rep": np.arange(n, dtype=np.int64) * 3, "keys": r.integers(0, 100_000, (1, n)),
            "vals": np.stack([cnt.astype(np.int64).view(np.uint64), v.view(np.uint64)]),
            "nulls": np.zeros((2, n), np.uint8)}, cnt, v


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_output_is_written_whole(tmp_path):
    a, cnt, v = _arrays(1000, 4)
    bench.dump_outputs(str(tmp_path / "d"), a)
    got = _load(str(tmp_path / "d"))
    assert all(x.dtype == np.float64 for x in got.values())
    assert np.array_equal(got["rows_index"], np.arange(1000)) and np.array_equal(got["flushes_index"], np.arange(4))
    assert np.array_equal(got["val0"], cnt) and np.array_equal(got["val1"], v, equal_nan=True)
    assert np.array_equal(got["ts"], a["ts"]) and np.array_equal(got["key0"], a["keys"][0])
    assert np.array_equal(got["flush_rows"], [250] * 4) and got["n_rows"][0] == 1000 and got["n_flushes"][0] == 4


def test_large_output_is_cut_to_the_same_seeded_rows(tmp_path):
    n = 700_000  # 8 row arrays + the index x 8 B x n = 50 MB: over the rows' 36 MB share
    a, cnt, v = _arrays(n, 33)
    bench.dump_outputs(str(tmp_path / "d1"), a)
    bench.dump_outputs(str(tmp_path / "d2"), a)
    g1, g2 = _load(str(tmp_path / "d1")), _load(str(tmp_path / "d2"))
    assert sorted(g1) == sorted(g2) and all(np.array_equal(g1[k], g2[k], equal_nan=True) for k in g1)
    assert sum(x.nbytes for x in g1.values()) <= bench.DUMP_MAX_BYTES
    rows = g1["rows_index"].astype(np.int64)
    assert 0 < rows.size < n and np.all(np.diff(rows) > 0)
    assert np.array_equal(g1["val1"], v[rows], equal_nan=True) and np.array_equal(g1["rep"], a["rep"][rows])
    assert g1["n_rows"][0] == n and g1["flush_rows"].sum() == n
