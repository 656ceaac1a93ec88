"""tests/order_model.py pinned without a GPU: the OrderByLimitTestCase cases that run on shapes the library
has (their inputs and assertions transcribed into tests/golden/kat_order_limit.json), hand traces of the
rules the reference cases do not reach, and the coverage of the streams tests/test_gpu_order.py uses — the
GPU tests then only compare."""
import numpy as np
import pytest

from oracle.oracle import OracleQuery
from siddhi_amd import abi
from tests import order_model as om
from tests.parity import run_pushes

KATS = om.load_kats()


@pytest.mark.parametrize("case", KATS["reference_cases"], ids=lambda c: c["name"])
def test_reference_cases(case):
    schema = abi.Schema.parse(KATS["schema"])
    ids = {}
    rows = [(1000 + i, ids.setdefault(s, len(ids)), p, v) for i, (s, p, v) in enumerate(case["events"])]
    assert [r[3] for r in rows] == list(range(len(rows)))  # volume = stream index = rep
    spec = abi.QuerySpec(schema, "lengthBatch", 4, group_by=case["group_by"], aggs=[tuple(a) for a in case["aggs"]],
                         key_capacity=16, order_by=[tuple(t) for t in case["order_by"] or ()] or None,
                         limit=case["limit"], offset=case["offset"])
    pushes = [abi.HostBatch.from_rows(schema, rows, send_size=1)]
    out = om.expected(spec, pushes)
    e = case["expect"]
    fo = out["flush_offsets"]
    assert np.diff(fo).tolist() == e["rows_per_callback"]
    assert len(out["ts"]) == e["total"]
    assert [int(out["rep"][fo[f]]) for f in range(len(fo) - 1)] == e["first_volume"]


def test_reference_cases_listed():
    """every test of the reference class is either transcribed or named as not covered"""
    names = {c["name"] for c in KATS["reference_cases"]} | set(KATS["not_covered"])
    assert names == {f"limitTest{i}" for i in range(1, 20)} - {"limitTest8"}  # (the class has no limitTest8)
    assert {c["name"] for c in KATS["reference_cases"]} == {f"limitTest{i}" for i in (1, 3, 6, 10, 12, 14)}


def _trace_arrays(t):
    n = len(t["expired"])
    vt = [abi.TYPE_NAMES[x] for x in t["val_types"]]
    vals = np.zeros((len(vt), n), np.uint64)
    for a, col in enumerate(t["vals"]):
        vals[a] = (np.array([float(x) for x in col], np.float64) if vt[a] in (abi.FLOAT, abi.DOUBLE)
                   else np.array([int(x) for x in col], np.int64)).view(np.uint64)
    return {"flush_offsets": np.array([0, n], np.int64), "flush_clock": np.array([77], np.int64),
            "val_types": np.array(vt, np.int32), "ts": np.arange(n, dtype=np.int64) + 100,
            "expired": np.array(t["expired"], np.uint8), "rep": np.arange(n, dtype=np.int64),
            "keys": np.zeros((0, n), np.int64), "vals": vals, "nulls": np.array(t["nulls"], np.uint8).reshape(len(vt), n)}


@pytest.mark.parametrize("t", KATS["hand_traces"], ids=lambda t: t["name"])
def test_hand_traces(t):
    src = _trace_arrays(t)
    out = om.apply(src, [tuple(x) for x in t["terms"]], t["limit"], t["offset"])
    assert out["rep"].tolist() == t["expect_rows"]
    assert out["flush_clock"].tolist() == [77] and out["flush_offsets"].tolist() == [0, len(t["expect_rows"])]
    # the rows travel whole
    for k in ("ts", "expired"):
        assert np.array_equal(out[k], src[k][t["expect_rows"]])
    assert np.array_equal(out["vals"], src["vals"][:, t["expect_rows"]])


def test_emptied_flush_and_single_row():
    t = dict(KATS["hand_traces"][0])
    src = _trace_arrays(t)
    two = abi.concat_arrays([src, src])
    two["flush_clock"] = np.array([77, 99], np.int64)
    # offset beyond the flush: nothing left, no flush
    out = om.apply(two, [("agg", 0)], None, 5)
    assert out["flush_clock"].size == 0 and out["ts"].size == 0 and out["flush_offsets"].tolist() == [0]
    # limit 0: the CURRENT rows go, the EXPIRED ones stay, in both flushes
    out = om.apply(two, None, 0, None)
    assert out["rep"].tolist() == [1, 3, 1, 3] and out["flush_clock"].tolist() == [77, 99]
    # rule 6: one row per chunk, kept iff offset in (unset, 0) and limit in (unset, > 0) — an EXPIRED row too
    one = {k: (v[:, :1] if v.ndim == 2 else v[:1]) for k, v in src.items() if k not in ("flush_offsets", "flush_clock", "val_types")}
    one.update(flush_offsets=np.array([0, 1], np.int64), flush_clock=np.array([5], np.int64), val_types=src["val_types"])
    one["expired"] = np.array([1], np.uint8)
    for limit, offset, kept in [(None, None, 1), (3, 0, 1), (0, None, 0), (None, 1, 0), (1, 1, 0)]:
        assert len(om.apply(one, None, limit, offset, single=True)["ts"]) == kept, (limit, offset)
    assert len(om.apply(one, None, 0, None, single=False)["ts"]) == 1  # (the general rule keeps an EXPIRED row)


def _merge(total, cnt):
    for k, v in cnt.items():
        total[k] = total[k] | v if isinstance(v, set) else total[k] + v


def test_gpu_matrix_coverage():
    """what the streams of tests/test_gpu_order.py exercise, from the model alone"""
    total = om.new_counters()
    seen = {"fam": set(), "output": set(), "keys": set(), "ss": set(), "terms": set(), "limit": set(), "offset": set()}
    for c in om.matrix():
        spec, pushes, want, cnt = om.case(*c)
        _merge(total, cnt)
        for k, v in zip(("fam", "output", "keys", "ss", "terms", "limit", "offset"), c):
            seen[k].add(v)
    assert seen["fam"] == set(om.WINDOWS) and seen["output"] == {"current", "expired", "all"}
    assert seen["keys"] == {12, 3000} and seen["ss"] == {1, 50}
    assert seen["terms"] == set(om.TERMS) - {"none", "sumv"}
    assert seen["limit"] == set(om.LIMITS) and seen["offset"] == set(om.OFFSETS)
    assert total["tie_by_position"] > 0 and total["null_order_value"] > 0 and total["emptied_by_offset"] > 0
    assert total["limit_cut_current_expired_after"] > 0 and total["alternating"] > 0
    assert any(2 <= s <= om.BLOCK_ROWS for s in total["sizes"]) and any(s > om.BLOCK_ROWS for s in total["sizes"])


def test_sizes_stream_coverage():
    """the flush sizes stand below, at and above every boundary, and both size classes are sorted"""
    spec, pushes, want, cnt = om.sizes_case()
    base = om.base_output(spec, pushes)
    assert np.diff(base["flush_offsets"]).tolist() == om.SIZES
    assert cnt["sizes"] == set(om.SIZES) - {1}
    assert np.array_equal(np.diff(want["flush_offsets"]), om.SIZES)  # (no limit: every row survives)
    spec, pushes, want, cnt = om.sizes_case("count", 10, 1)
    assert cnt["tie_by_position"] == len(om.SIZES) - 1 and cnt["emptied_by_offset"] == 1
    assert np.diff(want["flush_offsets"]).tolist() == [min(10, s - 1) for s in om.SIZES[1:]]


def test_special_doubles_reach_the_sum():
    spec, pushes, want, cnt = om.case("timeBatch700", "current", 12, 50, "sumv", None, None, special=True)
    s = want["vals"][1].view(np.float64)
    assert np.isnan(s).any() and np.isposinf(s).any() and np.isneginf(s).any()
    assert (s == 0).any()
    # ordered: per flush -Infinity first, NaN last
    fo = want["flush_offsets"]
    for f in range(len(fo) - 1):
        col = s[fo[f]:fo[f + 1]]
        num = col[~np.isnan(col)]
        assert np.all(num[:-1] <= num[1:]) and np.all(np.isnan(col[len(num):]))


def test_typed_streams_hold_both_zeros():
    """the typed GPU cases: -0.0 and 0.0 both occur in the ordered double and float columns and as float key values,
    and the model puts -0.0 first"""
    def zeros(col):
        z = col[col == 0]
        return bool(np.signbit(z).any()) and bool((~np.signbit(z)).any())
    spec, pushes, want, cnt = om.typed_case("min_double")
    assert zeros(want["vals"][1].view(np.float64)) and cnt["sizes"]
    spec, pushes, want, cnt = om.typed_case("min_float")
    assert zeros(want["vals"][3].view(np.float64)) and want["val_types"][3] == abi.FLOAT
    spec, pushes, want, cnt = om.typed_case("float_key")
    keys = want["keys"][0].view(np.float64)
    assert zeros(keys)
    fo = want["flush_offsets"]
    seen = 0
    for f in range(len(fo) - 1):
        col = keys[fo[f]:fo[f + 1]]
        z = np.nonzero(col == 0)[0]
        if len(z) == 2:   # desc: 0.0 before -0.0
            assert not np.signbit(col[z[0]]) and np.signbit(col[z[1]]) and z[1] == z[0] + 1
            seen += 1
    assert seen > 0
    spec, pushes, want, cnt = om.typed_case("bool_key", "time500", "all", 5)
    assert set(want["keys"][0].tolist()) == {0, 1} and cnt["null_order_value"] >= 0


def test_model_leaves_an_unordered_output_alone():
    spec, pushes, want, cnt = om.case("timeBatch700", "all", 12, 50, "count", None, None)
    base = om.base_output(spec, pushes)
    same = om.apply(base, None, None, 0)
    for k in base:
        assert np.array_equal(same[k], base[k]), k
    q = OracleQuery(spec)  # (the oracle ignores the spec's order fields)
    ora = run_pushes(q, pushes)
    q.close()
    for k in base:
        assert np.array_equal(ora[k], base[k]), k
