"""The `having` model (tests/having_model.py) pinned to the KAT-pinned oracle, to the hand-traced example,
and shown able to tell the reference's per-event `having` (QuerySelector.java:315-374) from the naive
"filter the final rows" — which is what makes tests/test_gpu_having.py able to fail. No GPU."""
import functools

import numpy as np
import pytest

from oracle.oracle import OracleQuery
from siddhi_amd import abi
from tests import having_model as hm
from tests.parity import assert_same, run_pushes


@functools.lru_cache(maxsize=None)
def _stream():
    return hm.stream()


@functools.lru_cache(maxsize=None)
def _chunks(fam, sc, ss):
    ts, cols = _stream()
    return hm.chunks(hm.make_spec(fam, sc, False), hm.make_pushes(ts, cols, ss))


_PLAIN = [("lengthBatch", 37, {}), ("lengthBatch", 1, {}), ("timeBatch", 700, {}), ("timeBatch", 333, {"start_time": 100}),
          ("externalTimeBatch", 700, {"ts_attr": "ts"})]
# (externalTimeBatch has no stream.current.event form)
_WINDOW_MODES = [w + (False,) for w in _PLAIN] + [w + (True,) for w in _PLAIN if w[0] != "externalTimeBatch"]


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("send_size", [1, 13, 0])
@pytest.mark.parametrize("window,param,extra,sc", _WINDOW_MODES)
def test_model_without_having_is_the_oracle(window, param, extra, sc, send_size, grouped):
    ts, cols = _stream()
    spec = abi.QuerySpec(hm.SCHEMA, window, param, group_by=["k"] if grouped else (), aggs=hm.AGGS, filter=hm.FILTER,
                         stream_current=sc, key_capacity=32, **extra)
    pushes = hm.make_pushes(ts, cols, send_size)
    o = OracleQuery(spec)
    want = run_pushes(o, pushes)
    o.close()
    assert want["ts"].size > 0
    assert_same(hm.run_model(spec, pushes, having=None), want, label="model")


def _example(having):
    schema = abi.Schema.parse("k int, x long")
    spec = abi.QuerySpec(schema, "lengthBatch", 5, group_by=["k"], aggs=[("count", None), ("sum", "x")], key_capacity=4,
                         having=having)
    A, B = 0, 1
    rows = [(100, A, 10), (101, B, 5), (102, B, 7), (103, A, 1), (104, A, 2)]
    out = hm.run_model(spec, [abi.HostBatch.from_rows(schema, rows)])
    n = out["ts"].size
    return [(int(out["keys"][0][i]), int(out["vals"][0][i]), int(out["vals"][1][i].view(np.int64)), int(out["rep"][i]))
            for i in range(n)], len(out["flush_clock"])


def test_hand_traced_example():
    A, B = 0, 1
    assert _example(None) == ([(A, 3, 13, 4), (B, 2, 12, 2)], 1)
    # B passes first (at e2), A later (at e3)
    assert _example((">=", ("agg", 1), 11)) == ([(B, 2, 12, 2), (A, 3, 13, 4)], 1)
    # A's row is not its last event
    assert _example(("==", ("agg", 0), 2)) == ([(B, 2, 12, 2), (A, 2, 11, 3)], 1)
    assert _example((">", ("agg", 0), 3)) == ([], 0)


def _observe(fam, sc, grouped, ss, pn):
    """(chunks, chunks whose rows differ from the naive filter of the no-having rows, chunks whose surviving
    keys come in another order than in the no-having flush, chunks that disappear)"""
    ts, cols = _stream()
    pred = hm.PREDICATES[pn]
    spec = hm.make_spec(fam, sc, grouped)
    pushes = hm.make_pushes(ts, cols, ss)
    cl = _chunks(fam, sc, ss)
    plain, got = {}, {}
    hm.run_model(spec, pushes, having=None, chunk_list=cl, on_chunk=lambda i, g: plain.__setitem__(i, g))
    hm.run_model(spec, pushes, having=pred, chunk_list=cl, on_chunk=lambda i, g: got.__setitem__(i, g))
    differ = reorder = gone = 0
    for i in plain:
        naive = {k: r for k, r in plain[i].items() if hm.evaluate(pred, k, r[2])}
        differ += list(naive.items()) != list(got[i].items())
        order = [k for k in plain[i] if k in got[i]]
        reorder += order != list(got[i])
        gone += not got[i]
    return len(plain), differ, reorder, gone


def test_measured_cases():
    """The two cases measured with the prototype when the feature was specified (12 keys)."""
    assert _observe("timeBatch700", False, True, 1, "count==2") == (112, 110, 109, 1)
    n, differ, reorder, gone = _observe("timeBatch700", True, True, 13, "sumx>=500000")
    assert (n, differ, reorder, n - gone) == (310, 114, 47, 298)


def _family_cases():
    out = {}
    for case in hm.matrix():
        out.setdefault((case[0], case[1]), []).append(case)
    return out


@pytest.mark.parametrize("fam,sc", sorted(_family_cases()))
def test_gpu_matrix_can_fail(fam, sc):
    """For every case of the GPU matrix whose chunks can hold several events of a key — the plain batch windows,
    and timeBatch(T, true) unless every send is one event — and whose predicate reads an aggregate, the expected
    rows differ from the naive filter in some chunk; grouped, the surviving keys are reordered in some chunk.
    (One event per chunk — lengthBatch(L, true), sends of one event — makes `having` a pure row filter, and so
    does a predicate on the key alone: nothing to demand there but the rows.) Across each window family at
    least one chunk disappears entirely."""
    gone_total = 0
    for case in _family_cases()[(fam, sc)]:
        _, _, grouped, ss, pn = case
        n, differ, reorder, gone = _observe(*case)
        gone_total += gone
        multi = not sc or (fam != "lengthBatch37" and ss != 1)
        if multi and pn != "not(k==3)":
            assert differ > 0, case
            if grouped:
                assert reorder > 0, case
    assert gone_total > 0
