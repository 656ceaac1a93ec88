"""tests/having_expired_model.py pinned on the CPU: against the frozen oracle where the oracle can speak
(no `having`; the remove forms through a sliding window), against hand traces, against the reference's
fixture, and the coverage conditions that keep the GPU matrix of tests/test_gpu_having_expired.py from
passing vacuously."""
import dataclasses
import functools
import json
import os

import numpy as np
import pytest

from oracle.oracle import OracleQuery
from siddhi_amd import abi
from tests import having_expired_model as hx
from tests import kat_runner
from tests.parity import assert_same, run_pushes

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def _stream():
    return hx.stream()


@functools.lru_cache(maxsize=None)
def _chunks(fam, ss):
    ts, cols = _stream()
    return hx.chunks(hx.make_spec(fam, False, "all"), hx.make_pushes(ts, cols, ss))


# ---- against the oracle without having: chunking, RESET placement, row order, final states ---------------
@pytest.mark.parametrize("ss", [1, 13, 0])
@pytest.mark.parametrize("output", ["all", "expired"])
@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("fam", list(hx.WINDOWS))
def test_model_without_having_is_the_oracle(fam, grouped, output, ss):
    ts, cols = _stream()
    spec = hx.make_spec(fam, grouped, output)
    pushes = hx.make_pushes(ts, cols, ss)
    o = OracleQuery(spec)
    want = run_pushes(o, pushes)
    o.close()
    got = hx.run_model(spec, pushes, having=None, chunk_list=_chunks(fam, ss))
    # (lengthBatch without group-by, all events: the one key's current row always takes its expired row's place)
    assert want["ts"].size > 0 and (want["expired"].any() or (fam.startswith("lengthBatch") and not grouped))
    assert_same(got, want, label=f"{fam} grouped={grouped} {output} ss={ss}")


# ---- the remove forms against the oracle: a sliding time window shows every intermediate state -----------
RSCHEMA = abi.Schema.parse("k int, v double, x long")
RAGGS = [("count", None), ("sum", "v"), ("avg", "v"), ("min", "v"), ("max", "v"),
         ("sum", "x"), ("avg", "x"), ("min", "x"), ("max", "x")]
BIG = 1 << 55
REMOVE_CASES = {
    "5,3,5": ([5.0, 3.0, 5.0], [5, 3, 5]),
    "duplicates": ([2.0, 7.0, 2.0, 7.0, 1.0, 7.0, 2.0, 1.0], [4, 4, 9, 1, 9, 4, 1, 9]),
    "falling then rising": ([9.0, 8.0, 7.0, 7.5, 8.0, 9.0], [-1, -2, -3, -3, -2, -1]),
    "long sums past 2^55": ([0.5, -0.0, 0.0, 0.25], [BIG + 1, 3 * BIG + 3, -(BIG + 5), 5 * BIG + 7]),
}


@pytest.mark.parametrize("name", list(REMOVE_CASES))
def test_remove_forms_against_the_sliding_oracle(name):
    """Key A's n events, then key B's events one by one, each expiring exactly one of A's: A's expired rows
    are its states after 1 .. n removals."""
    va, xa = REMOVE_CASES[name]
    n, T = len(va), 1000
    ts = np.array([100 + 10 * i for i in range(n)] + [100 + 10 * i + T for i in range(n)], np.int64)
    k = np.array([0] * n + [1] * n, np.int32)
    v = np.array(va + [1.0] * n, np.float64)
    x = np.array(xa + [1] * n, np.int64)
    for nagg in (4, 5):   # (the plan holds 8 aggregators: count + four of each column, in two queries)
        aggs = [RAGGS[0]] + (RAGGS[1:5] if nagg == 4 else RAGGS[5:9])
        spec = abi.QuerySpec(RSCHEMA, "time", T, group_by=["k"], aggs=aggs, output="expired", key_capacity=16)
        o = OracleQuery(spec)
        out = run_pushes(o, [abi.HostBatch(RSCHEMA, ts, [k, v, x], 1)])
        o.close()
        rows = np.nonzero((out["keys"][0] == 0) & (out["expired"] == 1))[0]
        assert rows.size == n, (name, rows.size)
        st = hx.KeyState(spec)
        evs = [[0, va[i], xa[i]] for i in range(n)]
        for ev in evs:
            st.add(ev)
        fp = [t in (abi.DOUBLE, abi.FLOAT) for t in out["val_types"]]
        for i, ev in enumerate(evs):
            st.remove(ev)
            for a, val in enumerate(st.values()):
                assert bool(out["nulls"][a][rows[i]]) == (val is None), (name, aggs[a], i)
                if val is None:
                    continue
                got = out["vals"][a][rows[i]]
                want = np.array([val], np.float64 if fp[a] else np.int64).view(np.uint64)[0]
                assert got == want, (name, aggs[a], i, got, want)


def test_long_sum_removal_differs_from_exact_subtraction():
    """The (double) round trip of SumAttributeAggregatorExecutor.java:283-291 is visible past 2^53."""
    spec = abi.QuerySpec(RSCHEMA, "time", 1000, aggs=[("sum", "x")], output="expired", key_capacity=16)
    st = hx.KeyState(spec)
    xs = REMOVE_CASES["long sums past 2^55"][1]
    for x in xs:
        st.add([0, 0.0, x])
    st.remove([0, 0.0, xs[0]])
    assert st.values()[0] != sum(xs[1:])


# ---- hand traces ------------------------------------------------------------------------------------------
def _tiny(window, param, vs, ks, output, having, aggs, send_size=1, advance=None):
    n = len(vs)
    ts = np.arange(1000, 1000 + 10 * n, 10, dtype=np.int64)
    cols = [np.array(ks, np.int32), np.array(vs, np.float64), np.zeros(n, np.int64), ts.copy()]
    spec = abi.QuerySpec(hx.SCHEMA, window, param, group_by=["k"], aggs=aggs, stream_current=True, output=output,
                         key_capacity=16, having=having)
    pushes = [abi.HostBatch(hx.SCHEMA, ts, cols, send_size)]
    if advance:
        pushes.append(("advance", advance))
    return spec, pushes


def test_trace_min_5_3_5():
    """min over 5, 3, 5: removing the first 5 deletes the LATER 5 from the deque [3, 5]; removing 3 leaves it
    empty, so the min is null while one event is still in the window — `not (min < 4)` passes there."""
    spec, pushes = _tiny("timeBatch", 1000, [5.0, 3.0, 5.0], [1, 1, 1], "expired",
                         ("not", ("<", ("agg", 1), 4.0)), [("count", None), ("min", "v")], advance=5000)
    cnt = {}
    out = hx.run_model(spec, pushes, counters=cnt)
    # removals: (count 2, min 3) fails, (count 1, min null) passes, (count 0, min null) passes: the row of the last
    assert out["ts"].size == 1 and out["expired"].tolist() == [1]
    assert out["vals"][0].view(np.int64).tolist() == [0] and out["nulls"][1].tolist() == [1]
    assert out["rep"].tolist() == [2] and cnt["non_front"] == 1
    # ... and with `min < 4` only the first removal passes: count 2, min 3, the first event as representative
    spec2 = dataclasses.replace(spec, having=("<", ("agg", 1), 4.0))
    out = hx.run_model(spec2, pushes, counters=cnt)
    assert out["vals"][0].view(np.int64).tolist() == [2] and out["vals"][1].view(np.float64).tolist() == [3.0]
    assert out["rep"].tolist() == [0] and out["nulls"].sum() == 0 and cnt["kept_not_last_removal"] == 1


def test_trace_current_replaces_expired_in_place():
    """lengthBatch(3, true), all events, having count <= 1. Keys 1, 2, 1 fill batch 0; the 4th event (key 2)
    starts batch 1 and carries batch 0's removals: key 1 -> counts 1, (key 2 -> 0), key 1 -> 0. Both keys'
    expired rows pass (key 1 first: position 0, content of its last removal; key 2 position 1); then the
    event's own row (key 2, count 1) passes and takes key 2's slot in place with expired flag 0."""
    spec, pushes = _tiny("lengthBatch", 3, [1.0, 2.0, 3.0, 4.0], [1, 2, 1, 2], "all",
                         ("<=", ("agg", 0), 1), [("count", None), ("sum", "v")])
    cnt = {}
    out = hx.run_model(spec, pushes, counters=cnt)
    # chunks: e0 (k1 count 1: passes), e1 (k2 count 1: passes), e2 (k1 count 2: fails), then the closing chunk
    assert out["flush_offsets"].tolist() == [0, 1, 2, 4]
    assert out["keys"][0].tolist() == [1, 2, 1, 2]
    assert out["expired"].tolist() == [0, 0, 1, 0]
    assert out["rep"].tolist() == [0, 1, 2, 3]
    assert out["vals"][0].view(np.int64).tolist() == [1, 1, 0, 1]
    assert out["nulls"][1].tolist() == [0, 0, 1, 0]
    assert cnt["current_replaces_expired"] == 1
    # the oracle agrees on everything the oracle can see: the same stream without having
    o = OracleQuery(dataclasses.replace(spec, having=None))
    want = run_pushes(o, pushes)
    o.close()
    assert_same(hx.run_model(spec, pushes, having=None), want, label="trace")


# ---- the reference's fixture ------------------------------------------------------------------------------
def load_fixture():
    with open(os.path.join(HERE, "golden", "kat_having.json")) as f:
        return json.load(f)["cases"][0]


def fixture_spec_and_pushes(case):
    """The case as (spec with its having, pushes), built with tests/kat_runner.py's helpers."""
    dic = kat_runner.Dict()
    schema, spec = kat_runner.build(case, dic)
    having = kat_runner._conv_filter(case["query"]["having"], dic)
    spec = dataclasses.replace(spec, having=having, key_capacity=16)
    pushes = [("advance", s["advance"]) if isinstance(s, dict) else kat_runner.batch_of(schema, s, dic)
              for s in case["sends"]]
    return spec, pushes


def check_fixture(case, out):
    e = case["expect"]
    assert int((out["expired"] == 0).sum()) == e["in_count"]
    assert int((out["expired"] == 1).sum()) == e["remove_count"]
    assert out["vals"][0].view(np.int64)[out["expired"] == 1].tolist() == e["remove_values"]


def test_reference_fixture_through_the_model():
    case = load_fixture()
    spec, pushes = fixture_spec_and_pushes(case)
    assert spec.window == "timeBatch" and spec.stream_current and spec.output == "all"
    check_fixture(case, hx.run_model(spec, pushes))


# ---- the coverage conditions of the GPU matrix ------------------------------------------------------------
def _counters(fam, grouped, output, pns, sss=(13,)):
    ts, cols = _stream()
    tot = {}
    for ss in sss:
        for pn in pns:
            cnt = {}
            spec = hx.make_spec(fam, grouped, output, having=hx.PREDICATES[pn])
            hx.run_model(spec, hx.make_pushes(ts, cols, ss), chunk_list=_chunks(fam, ss), counters=cnt)
            for k, v in cnt.items():
                tot[k] = tot.get(k, 0) + v
    return tot


@pytest.mark.parametrize("fam", ["lengthBatch37", "timeBatch700", "timeBatch333s"])
def test_matrix_covers_the_remove_pass(fam):
    c = _counters(fam, True, "all", list(hx.PREDICATES))
    assert c["kept_not_last_removal"] > 0      # a surviving EXPIRED row that is not the key's last removal
    assert c["pass_then_fail"] > 0             # a passing removal and a later failing one
    assert c["key_without_row"] > 0            # a key without a row in a chunk where others keep theirs
    # a closing chunk that keeps nothing: no flush (lengthBatch(37): some key of 12 always passes; lengthBatch(1) below)
    assert c["chunk_without_row"] > 0 or fam == "lengthBatch37"
    assert c["null_in_row"] > 0                # a surviving row with a null aggregate
    assert c["non_front"] > 0                  # removeFirstOccurrence past the deque's front


def test_matrix_covers_the_length_batch_join():
    c = _counters("lengthBatch37", True, "all", list(hx.PREDICATES))
    assert c["current_replaces_expired"] > 0 and c["current_follows_expired"] > 0
    c = _counters("lengthBatch1", True, "all", list(hx.PREDICATES))
    assert c["current_replaces_expired"] > 0 and c["current_follows_expired"] > 0 and c["chunk_without_row"] > 0


def test_each_predicate_keeps_expired_and_current_rows():
    ts, cols = _stream()
    for pn in hx.PREDICATES:
        spec = hx.make_spec("timeBatch700", True, "all", having=hx.PREDICATES[pn])
        out = hx.run_model(spec, hx.make_pushes(ts, cols, 13), chunk_list=_chunks("timeBatch700", 13))
        assert (out["expired"] == 1).any(), pn
        if pn != "count==0":
            assert (out["expired"] == 0).any(), pn
