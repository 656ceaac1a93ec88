"""`having` with expired / all-events output on lengthBatch(L, true) / timeBatch(T, true), on the GPU against
tests/having_expired_model.py, bit for bit: flush offsets, flush clocks, ts, keys, value bits, rep, expired
and nulls. The selector tests the condition after every removal of a closing window's events
(QuerySelector.java:280-291, :325-339): a key's expired row is that of its last PASSING removal at the
position of its first; tests/test_having_expired_model.py shows that these cases tell that from the state
after the last removal."""
import dataclasses
import functools

import numpy as np
import pytest

from oracle.oracle import OracleQuery
from siddhi_amd import abi
from tests import having_expired_model as hx
from tests.parity import assert_same, run_pushes, split_batches
from tests.test_having_expired_model import check_fixture, fixture_spec_and_pushes, load_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from siddhi_amd import runtime
    return runtime


@functools.lru_cache(maxsize=None)
def _stream(n=4000, keys=12):
    return hx.stream(n, keys)


@functools.lru_cache(maxsize=None)
def _chunks(fam, ss, n=4000, keys=12):
    ts, cols = _stream(n, keys)
    return hx.chunks(hx.make_spec(fam, False, "all"), hx.make_pushes(ts, cols, ss))


def _check(rt, spec, pushes, chunk_list=None, label=""):
    want = hx.run_model(spec, pushes, chunk_list=chunk_list)
    g = rt.GpuQuery(spec)
    got = run_pushes(g, pushes)
    g.close()
    assert_same(got, want, label=label)
    return got


@pytest.mark.parametrize("fam,grouped,output,ss,pn", hx.matrix())
def test_matrix(rt, fam, grouped, output, ss, pn):
    ts, cols = _stream()
    spec = hx.make_spec(fam, grouped, output, having=hx.PREDICATES[pn])
    _check(rt, spec, hx.make_pushes(ts, cols, ss), _chunks(fam, ss), label=f"{fam} {output} ss={ss} {pn}")


@pytest.mark.parametrize("pn", ["count==0", "not(minv<0)"])
@pytest.mark.parametrize("fam", ["lengthBatch37", "timeBatch700"])
def test_many_short_runs(rt, fam, pn):
    """3000 keys: the runs outnumber one workgroup's 256 threads, and the deques sit at offsets across blocks."""
    ts, cols = _stream(4000, 3000)
    spec = hx.make_spec(fam, True, "all", having=hx.PREDICATES[pn], keys=3000)
    got = _check(rt, spec, hx.make_pushes(ts, cols, 13), _chunks(fam, 13, 4000, 3000), label="short runs")
    assert int(got["expired"].sum()) > 256


@pytest.mark.parametrize("output", ["all", "expired"])
def test_one_long_run(rt, output):
    """No group-by, lengthBatch(3000, true), min and max in the plan: one thread, thousands of removals."""
    ts, cols = _stream()
    spec = abi.QuerySpec(hx.SCHEMA, "lengthBatch", 3000, aggs=hx.AGGS, filter=hx.FILTER, stream_current=True,
                         output=output, key_capacity=16, having=hx.PREDICATES["minv<0"])
    got = _check(rt, spec, hx.make_pushes(ts, cols, 0), label="long run")
    assert got["expired"].any()


def test_long_sums_lose_bits_as_in_java(rt):
    """sum(long) removes through (long) ((double) sum - (double) v): values of magnitude 2^55 and more."""
    n = 64
    rng = np.random.default_rng(11)
    ts = np.arange(1000, 1000 + 10 * n, 10, dtype=np.int64)
    k = rng.integers(0, 3, n).astype(np.int32)
    x = (rng.integers(1, 8, n) * (1 << 55) + rng.integers(1, 1000, n)).astype(np.int64) * rng.choice([-1, 1], n)
    cols = [k, np.ones(n), x, ts.copy()]
    aggs = [("count", None), ("sum", "x"), ("avg", "x")]
    for grouped in (True, False):
        spec = abi.QuerySpec(hx.SCHEMA, "lengthBatch", 5, group_by=["k"] if grouped else (), aggs=aggs,
                             stream_current=True, output="expired", key_capacity=16, having=(">=", ("agg", 0), 1))
        got = _check(rt, spec, [abi.HostBatch(hx.SCHEMA, ts, cols, 1)], label="long sums")
        assert got["expired"].all() and got["ts"].size > 10


def test_reference_fixture_on_gpu(rt):
    case = load_fixture()
    spec, pushes = fixture_spec_and_pushes(case)
    got = _check(rt, spec, pushes, label=case["name"])
    check_fixture(case, got)


@pytest.mark.parametrize("fam", ["lengthBatch37", "timeBatch700"])
def test_push_device_equals_host_push(rt, fam):
    import torch
    ts, cols = _stream()
    spec = hx.make_spec(fam, True, "all", having=hx.PREDICATES["sumv>2|count==1"])
    batches = split_batches(hx.SCHEMA, ts, cols, hx.CUTS, 13)
    g = rt.GpuQuery(spec)
    parts = []
    for b in batches:
        keep = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in [b.ts] + b.cols]
        torch.cuda.synchronize()
        parts.append(rt.device_out_arrays(g.push_device(len(b.ts), keep[0].data_ptr(), [t.data_ptr() for t in keep[1:]], 13)))
    g.close()
    h = rt.GpuQuery(spec)
    host = run_pushes(h, batches)
    h.close()
    assert host["expired"].any() and not host["expired"].all()
    assert_same(abi.concat_arrays(parts), host, label="device push")
    assert_same(host, hx.run_model(spec, batches), label="host push")


@pytest.mark.parametrize("fam", ["lengthBatch37", "timeBatch700"])
def test_snapshot_in_the_middle_of_a_window(rt, fam):
    ts, cols = _stream()
    spec = hx.make_spec(fam, True, "all", having=hx.PREDICATES["count==2"])
    pushes = hx.make_pushes(ts, cols, 13)
    a = rt.GpuQuery(spec)
    run_pushes(a, pushes[:2])
    blob = a.snapshot()
    rest_a = run_pushes(a, pushes[2:])
    a.close()
    b = rt.GpuQuery(spec)   # (the program is configuration: set again before the restore)
    b.restore(blob)
    rest_b = run_pushes(b, pushes[2:])
    b.close()
    assert rest_a["expired"].any()
    assert_same(rest_b, rest_a, label="restored")
    full = hx.run_model(spec, pushes)
    head = hx.run_model(spec, pushes[:2])
    nr, nf = head["ts"].size, head["flush_clock"].size
    assert np.array_equal(rest_b["rep"], full["rep"][nr:]) and np.array_equal(rest_b["flush_clock"], full["flush_clock"][nf:])
    assert np.array_equal(rest_b["expired"], full["expired"][nr:])


@pytest.mark.parametrize("fam", ["lengthBatch37", "timeBatch700"])
def test_composes_with_the_rate_limiter(rt, fam):
    """The limiter runs on the finished output: it sees the having-filtered rows, expired ones included."""
    rate = ("last", 3)
    ts, cols = _stream()
    pushes = hx.make_pushes(ts, cols, 13)
    hv = hx.make_spec(fam, True, "all", having=hx.PREDICATES["minv<0"])
    both = rt.GpuQuery(dataclasses.replace(hv, rate=rate))
    got = run_pushes(both, pushes)
    both.close()
    only = rt.GpuQuery(hv)
    limiter = rt.GpuQuery(dataclasses.replace(hv, having=None, rate=rate))
    parts = []
    for p in pushes:
        raw = only.advance_time_raw(p[1]) if isinstance(p, tuple) else only.push_raw(p)
        parts.append(limiter.rate_apply_merged(abi.out_arrays(raw)))
    only.close()
    limiter.close()
    want = abi.concat_arrays(parts)
    assert want["ts"].size > 0
    assert_same(got, want, label=f"having + {rate}")


@pytest.mark.parametrize("output", ["all", "expired"])
@pytest.mark.parametrize("fam", ["lengthBatch37", "lengthBatch1", "timeBatch700"])
def test_expired_output_without_a_program_is_the_oracle(rt, fam, output):
    """(lengthBatch(1, true): a push ends in filtered events right after a full batch — the batch stays queued
    until the next push's first passing event carries its expired rows)"""
    ts, cols = _stream()
    spec = hx.make_spec(fam, True, output)
    pushes = hx.make_pushes(ts, cols, 13)
    o = OracleQuery(spec)
    want = run_pushes(o, pushes)
    o.close()
    g = rt.GpuQuery(spec)
    got = run_pushes(g, pushes)
    g.close()
    assert_same(got, want, label="no program")
