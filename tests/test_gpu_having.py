"""`having` on the GPU (sh_query_set_having) against tests/having_model.py, bit for bit: flush offsets,
flush clocks, ts, keys, value bits, rep, and nulls / expired all zero. The reference evaluates the
condition after every event on the key's running aggregates (QuerySelector.java:315-374): a key's row is
that of its last passing event, at the position of its first passing event; tests/test_having_model.py
shows that these cases tell that from filtering the final rows."""
import dataclasses
import functools

import numpy as np
import pytest

from siddhi_amd import abi
from tests import having_model as hm
from tests.parity import assert_same, run_pushes, split_batches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from siddhi_amd import runtime
    return runtime


@functools.lru_cache(maxsize=None)
def _stream(n=4000, keys=12):
    return hm.stream(n, keys)


@functools.lru_cache(maxsize=None)
def _chunks(fam, sc, ss, n=4000, keys=12):
    ts, cols = _stream(n, keys)
    return hm.chunks(hm.make_spec(fam, sc, False), hm.make_pushes(ts, cols, ss))


def _check(rt, spec, pushes, chunk_list=None, label=""):
    want = hm.run_model(spec, pushes, chunk_list=chunk_list)
    g = rt.GpuQuery(spec)
    got = run_pushes(g, pushes)
    g.close()
    assert_same(got, want, label=label)
    assert not got["nulls"].any() and not got["expired"].any()
    return got


@pytest.mark.parametrize("fam,sc,grouped,ss,pn", hm.matrix())
def test_matrix(rt, fam, sc, grouped, ss, pn):
    ts, cols = _stream()
    spec = hm.make_spec(fam, sc, grouped, having=hm.PREDICATES[pn])
    got = _check(rt, spec, hm.make_pushes(ts, cols, ss), _chunks(fam, sc, ss), label=f"{fam} sc={sc} {pn}")
    assert got["ts"].size > 0


@pytest.mark.parametrize("sc", [False, True])
@pytest.mark.parametrize("fam", ["lengthBatch37", "timeBatch700"])
def test_many_short_runs(rt, fam, sc):
    """3000 keys: the (window, key) runs of a push outnumber one workgroup's 256 threads."""
    ts, cols = _stream(4000, 3000)
    spec = hm.make_spec(fam, sc, True, having=hm.PREDICATES["count<=3&sumv>-100"], keys=3000)
    got = _check(rt, spec, hm.make_pushes(ts, cols, 13), _chunks(fam, sc, 13, 4000, 3000), label="short runs")
    assert got["ts"].size > 256


@pytest.mark.parametrize("sc", [False, True])
def test_one_long_run(rt, sc):
    """No group-by, lengthBatch(3000): a single thread walks thousands of entries."""
    ts, cols = _stream()
    spec = abi.QuerySpec(hm.SCHEMA, "lengthBatch", 3000, aggs=hm.AGGS, filter=hm.FILTER, stream_current=sc,
                         key_capacity=16, having=(">=", ("agg", 5), 0))
    got = _check(rt, spec, hm.make_pushes(ts, cols, 0), label="long run")
    assert got["ts"].size > 0


def test_large_push(rt):
    """One push above the small-push limit (sends of 13 events: hundreds of windows close in it), then a timer."""
    ts, cols = _stream(20_000, 12)
    spec = hm.make_spec("timeBatch700", False, True, having=hm.PREDICATES["count<=3&sumv>-100"],
                        aggs=[("count", None), ("sum", "v")])
    pushes = [abi.HostBatch(hm.SCHEMA, ts, cols, 13), ("advance", int(ts[-1]) + 5_000)]
    got = _check(rt, spec, pushes, label="large push")
    assert got["flush_clock"].size > 100


@pytest.mark.parametrize("sc", [False, True])
def test_push_device_equals_host_push(rt, sc):
    import torch
    ts, cols = _stream()
    spec = hm.make_spec("timeBatch700", sc, True, having=hm.PREDICATES["sumx>=500000"])
    batches = split_batches(hm.SCHEMA, ts, cols, hm.CUTS, 13)
    g = rt.GpuQuery(spec)
    g.set_compact_flushes(True)   # (ignored for a having query: the full host flush arrays)
    g.set_device_flushes(True)
    parts = []
    for b in batches:
        keep = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in [b.ts] + b.cols]
        torch.cuda.synchronize()
        parts.append(rt.device_out_arrays(g.push_device(len(b.ts), keep[0].data_ptr(), [t.data_ptr() for t in keep[1:]], 13)))
    g.close()
    h = rt.GpuQuery(spec)
    host = run_pushes(h, batches)
    h.close()
    assert host["ts"].size > 0
    assert_same(abi.concat_arrays(parts), host, label="device push")
    assert_same(host, hm.run_model(spec, batches), label="host push")


@pytest.mark.parametrize("rate", [("last", 3), ("first_time", 500)])
@pytest.mark.parametrize("sc", [False, True])
def test_composes_with_the_rate_limiter(rt, rate, sc):
    """The limiter runs on the finished output: it sees the having-filtered rows."""
    ts, cols = _stream()
    pushes = hm.make_pushes(ts, cols, 13)
    hv = hm.make_spec("timeBatch700", sc, True, having=hm.PREDICATES["count<=3&sumv>-100"])
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


@pytest.mark.parametrize("sc", [False, True])
def test_snapshot_restores_under_the_same_program(rt, sc):
    ts, cols = _stream()
    spec = hm.make_spec("timeBatch700", sc, True, having=hm.PREDICATES["count==2"])
    pushes = hm.make_pushes(ts, cols, 13)
    a = rt.GpuQuery(spec)
    run_pushes(a, pushes[:3])
    blob = a.snapshot()
    rest_a = run_pushes(a, pushes[3:])
    a.close()
    b = rt.GpuQuery(spec)   # (the program is configuration: set again before the restore)
    b.restore(blob)
    rest_b = run_pushes(b, pushes[3:])
    b.close()
    assert rest_a["ts"].size > 0
    assert_same(rest_b, rest_a, label="restored")
    # ... and it is the uninterrupted run's continuation
    full = hm.run_model(spec, pushes)
    head = hm.run_model(spec, pushes[:3])
    nr, nf = head["ts"].size, head["flush_clock"].size
    assert np.array_equal(rest_b["rep"], full["rep"][nr:]) and np.array_equal(rest_b["flush_clock"], full["flush_clock"][nf:])


def test_refusals_on_a_live_query(rt):
    L = rt.lib()
    ts, cols = _stream()
    count2 = hm.PREDICATES["count==2"]
    # set once, before the first push
    q = rt.GpuQuery(hm.make_spec("timeBatch700", False, True))
    q.push_raw(split_batches(hm.SCHEMA, ts, cols, [100], 0)[0])
    with pytest.raises(rt.SiddhiError) as e:
        q.set_having(count2)
    assert e.value.code == abi.SH_ERR_STATE
    q.close()
    q = rt.GpuQuery(hm.make_spec("timeBatch700", False, True, having=count2))
    with pytest.raises(rt.SiddhiError) as e:
        q.set_having(count2)
    assert e.value.code == abi.SH_ERR_STATE
    q.close()
    # an externalTimeBatch timeout and a having program refuse each other, in either order
    q = rt.GpuQuery(hm.make_spec("extTimeBatch700", False, True, having=count2))
    assert L.sh_query_set_ext_timeout(q.h, 500) == abi.SH_ERR_UNSUPPORTED
    assert "having" in L.sh_last_error().decode()
    assert L.sh_query_set_ext_replace_ts(q.h, 1) == abi.SH_ERR_UNSUPPORTED
    q.close()
    q = rt.GpuQuery(hm.make_spec("extTimeBatch700", False, True, timeout=500))
    with pytest.raises(rt.SiddhiError) as e:
        q.set_having(count2)
    assert e.value.code == abi.SH_ERR_UNSUPPORTED and "timeout" in str(e.value)
    q.close()
    q = rt.GpuQuery(hm.make_spec("extTimeBatch700", False, True, replace_ts=True))
    with pytest.raises(rt.SiddhiError) as e:
        q.set_having(count2)
    assert e.value.code == abi.SH_ERR_UNSUPPORTED
    q.close()
    # a sliding window with having fails at creation
    with pytest.raises(rt.SiddhiError) as e:
        rt.GpuQuery(abi.QuerySpec(hm.SCHEMA, "time", 700, group_by=["k"], aggs=hm.AGGS, key_capacity=32, having=count2))
    assert e.value.code == abi.SH_ERR_UNSUPPORTED and "sliding" in str(e.value)
    with pytest.raises(rt.SiddhiError) as e:
        rt.GpuQuery(abi.QuerySpec(hm.SCHEMA, "timeBatch", 700, group_by=["k", "x"], aggs=hm.AGGS, key_capacity=32,
                                  having=count2))
    assert e.value.code == abi.SH_ERR_UNSUPPORTED and "wide" in str(e.value)
