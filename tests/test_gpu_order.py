"""`order by` / `limit` / `offset` on the GPU (sh_query_set_order) against tests/order_model.py over the output
of the same query without them — the oracle's, tests/length_model.py's for `length`, tests/having_model.py's
with `having` — bit for bit: flush offsets, flush clocks, ts, keys, value bits, nulls, expired and rep.
tests/test_order_model.py pins the model and shows, without a GPU, what these streams exercise; here the
outputs are only compared. Both sort routes are forced (SH_ORD_BLOCK_MAX) and each is compared with the
model, never with the other."""
import dataclasses

import numpy as np
import pytest

from siddhi_amd import abi
from tests import having_model as hm
from tests import order_model as om
from tests.parity import assert_same, run_pushes, split_batches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from siddhi_amd import runtime
    return runtime


def gpu_run(rt, spec, pushes):
    g = rt.GpuQuery(spec)
    got = run_pushes(g, pushes)
    g.close()
    return got


def case_id(c):
    fam, output, keys, ss, terms, limit, offset = c
    return f"{fam}-{output}-keys{keys}-send{ss}-{terms}-limit{limit}-offset{offset}"


@pytest.mark.parametrize("case", om.matrix(), ids=case_id)
def test_matrix(rt, case):
    """every window family x current / expired / all; 12 and 3000 keys, sends of 1 and 50, the terms, limits and
    offsets in rotation; pushes cut in three, an advance between them and one behind (it closes a timeBatch window)"""
    spec, pushes, want, cnt = om.case(*case)
    assert_same(gpu_run(rt, spec, pushes), want, label=case_id(case))


@pytest.mark.parametrize("route", ["default", "global", "block", "threshold64"])
@pytest.mark.parametrize("terms,limit,offset,output", [("four", None, None, "current"), ("count", 10, 1, "current"),
                                                       ("minmax", 1, None, "all"), ("key_desc", 0, 63, "expired")])
def test_flush_sizes_on_both_routes(rt, monkeypatch, route, terms, limit, offset, output):
    """flushes of 1, 2, 63 / 64 / 65, 255 / 256 / 257, 511 / 512 / 513, 1023 / 1024 / 1025, 2048 and 3000 rows, one
    per call: the default threshold lies between 256 and 257 rows, SH_ORD_BLOCK_MAX=0 sorts every flush with the radix
    passes, =1024 every one that fits in LDS with the workgroup kernel, =64 moves the threshold between 64 and 65"""
    if om.ROUTES[route] is None:
        monkeypatch.delenv("SH_ORD_BLOCK_MAX", raising=False)  # (the default threshold: 256 / 257 rows straddle it)
    else:
        monkeypatch.setenv("SH_ORD_BLOCK_MAX", om.ROUTES[route])
    spec, pushes, want, cnt = om.sizes_case(terms, limit, offset, output)
    before = rt.order_debug_counts()
    got = gpu_run(rt, spec, pushes)
    passes, block, glob = (b - a for a, b in zip(before, rt.order_debug_counts()))
    assert_same(got, want, label=f"{route} {terms}")
    assert passes == len(pushes)
    # (current output: call w + 1 emits window w's flush, so the calls' flush sizes are SIZES)
    sorted_calls = sum(1 for s in om.SIZES if s > 1) if output == "current" else None
    if route == "global":
        assert block == 0 and glob > 0 and (sorted_calls is None or glob == sorted_calls)
    elif route == "block":
        assert block > 0 and glob > 0  # (1025, 2048 and 3000 rows do not fit in LDS)
        if sorted_calls is not None:
            assert block == sum(1 for s in om.SIZES if 1 < s <= om.BLOCK_ROWS) and block + glob == sorted_calls
    else:
        cut = om.DEFAULT_THRESHOLD if route == "default" else 64
        assert block > 0 and glob > 0
        if sorted_calls is not None:
            assert block == sum(1 for s in om.SIZES if 1 < s <= cut) and block + glob == sorted_calls


@pytest.mark.parametrize("route", ["global", "block"])
@pytest.mark.parametrize("fam,output,ss", [("lengthBatch65sc", "all", 50), ("time500", "all", 50),
                                           ("lengthBatch2500", "expired", 50), ("length300", "all", 50)])
def test_many_flushes_on_both_routes(rt, monkeypatch, route, fam, output, ss):
    """many small flushes in one call (chunked sends into sliding windows, stream.current.event), with runs of
    both types and nulls on EXPIRED rows, through either route"""
    monkeypatch.setenv("SH_ORD_BLOCK_MAX", om.ROUTES[route])
    spec, pushes, want, cnt = om.case(fam, output, 3000, ss, "minmax", 10, 1)
    assert_same(gpu_run(rt, spec, pushes), want, label=f"{route} {fam}")


@pytest.mark.parametrize("route", ["global", "block"])
@pytest.mark.parametrize("fam", ["timeBatch700", "lengthBatch2500", "lengthBatch65"])
def test_special_doubles(rt, monkeypatch, route, fam):
    """a double sum that is NaN / +-Infinity / 0.0 for whole keys: Double.compareTo's total order"""
    monkeypatch.setenv("SH_ORD_BLOCK_MAX", om.ROUTES[route])
    for terms in ("sumv", [("agg", 1, "desc"), ("key", 0)]):
        spec, pushes, want, cnt = om.case(fam, "current", 12, 50, terms, None, None, special=True)
        assert_same(gpu_run(rt, spec, pushes), want, label=f"{route} {fam} {terms}")


@pytest.mark.parametrize("route", ["global", "block"])
@pytest.mark.parametrize("name", list(om.TYPED))
def test_typed_terms(rt, monkeypatch, route, name):
    """a float and a bool group key as terms, double and float min / max holding -0.0 and 0.0 (the float widened
    to double orders as the float does), on a batch window with current and a sliding one with all-events output"""
    monkeypatch.setenv("SH_ORD_BLOCK_MAX", om.ROUTES[route])
    for fam, output, limit in (("timeBatch700", "current", None), ("time500", "all", 5)):
        spec, pushes, want, cnt = om.typed_case(name, fam, output, limit)
        assert want["ts"].size > 0
        assert_same(gpu_run(rt, spec, pushes), want, label=f"{route} {name} {fam}")


@pytest.mark.parametrize("limit,offset", [(2, None), (None, 1), (0, None), (1, 1)])
@pytest.mark.parametrize("fam,output", [("lengthBatch65", "current"), ("timeBatch700", "all"), ("time500", "all")])
def test_limit_and_offset_alone(rt, fam, output, limit, offset):
    """a pass-through query (`select *`) and a no-group-by aggregate (processInBatchNoGroupBy's one row per chunk)"""
    for aggs in ((), om.AGGS):
        spec, pushes, want, cnt = om.case(fam, output, 12, 50, "none", limit, offset, grouped=False, aggs=aggs)
        assert_same(gpu_run(rt, spec, pushes), want, label=f"{fam} aggs={len(aggs)}")


def test_terms_on_a_no_group_by_aggregate_change_nothing(rt):
    spec, pushes, want, cnt = om.case("timeBatch700", "current", 12, 50, [("agg", 0, "desc")], 1, 0, grouped=False)
    assert want["ts"].size > 0
    assert_same(gpu_run(rt, spec, pushes), want, label="one row per chunk")


@pytest.mark.parametrize("sc", [False, True])
@pytest.mark.parametrize("pn", ["count<=3&sumv>-100", "sumx>=500000"])
def test_having(rt, sc, pn):
    """the step sees the rows that survived `having`"""
    ts, cols = hm.stream()
    pushes = hm.make_pushes(ts, cols, 13)
    spec = dataclasses.replace(hm.make_spec("timeBatch700", sc, True, having=hm.PREDICATES[pn]),
                               order_by=om.TERMS["count_key"], limit=3, offset=1)
    want = om.expected(spec, pushes)
    assert want["ts"].size > 0
    assert_same(gpu_run(rt, spec, pushes), want, label=f"having {pn}")


def test_ext_time_batch_timeout(rt):
    spec = om.make_spec("extTimeBatch700", "current", 12, "avgx_desc", 2, None, timeout=300)
    ts, cols = om.stream(12)
    pushes = om.make_pushes(ts, cols, 50)
    want = om.expected(spec, pushes)
    assert_same(gpu_run(rt, spec, pushes), want, label="timeout")


@pytest.mark.parametrize("rate", [("all", 4), ("first", 3)])
@pytest.mark.parametrize("fam,output", [("timeBatch700", "current"), ("lengthBatch65sc", "all"), ("time500", "all")])
def test_rate_limiter_behind_it(rt, fam, output, rate):
    """the limiter sees the ordered, cut rows"""
    spec, pushes, want, cnt = om.case(fam, output, 12, 50, "count_key", 10, 1, rate=rate)
    assert want["ts"].size > 0
    assert_same(gpu_run(rt, spec, pushes), want, label=f"{fam} {rate}")


@pytest.mark.parametrize("fam,output", [("timeBatch700", "current"), ("lengthBatch65sc", "all"), ("time500", "expired")])
def test_push_device(rt, fam, output):
    """sh_push_device: the rows stay in HBM, the flush layout is on the host — also when the compact and the
    device layouts are asked for (they are ignored for an ordered query)"""
    import torch
    spec, pushes, want, cnt = om.case(fam, output, 12, 50, "four", 10, 1)
    g = rt.GpuQuery(spec)
    g.set_compact_flushes(True)
    g.set_device_flushes(True)
    parts = []
    for p in pushes:
        if isinstance(p, tuple):
            parts.append(abi.out_arrays(g.advance_time_raw(p[1])))
            continue
        keep = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in [p.ts] + p.cols]
        torch.cuda.synchronize()
        parts.append(rt.device_out_arrays(g.push_device(len(p.ts), keep[0].data_ptr(), [t.data_ptr() for t in keep[1:]], 50)))
    g.close()
    assert want["ts"].size > 0
    assert_same(abi.concat_arrays(parts), want, label=f"device push {fam}")


def test_staged_push(rt):
    spec, pushes, want, cnt = om.case("timeBatch700", "all", 12, 50, "sumx_asc", 10, None)
    g = rt.GpuQuery(spec)
    bufs = [rt.PinnedBatch(om.SCHEMA, om.EVENTS) for _ in range(2)]
    parts, i = [], 0
    for p in pushes:
        if isinstance(p, tuple):
            parts.append(abi.out_arrays(g.advance_time_raw(p[1])))
            continue
        parts.append(abi.out_arrays(g.push_staged_raw(g.stage(bufs[i % 2].fill(p.ts, p.cols, 50)))))
        i += 1
    g.close()
    for b in bufs:
        b.close()
    assert_same(abi.concat_arrays(parts), want, label="staged push")


@pytest.mark.parametrize("fam,output", [("timeBatch700", "all"), ("time500", "all"), ("length300", "current")])
def test_snapshot_restore_between_pushes(rt, fam, output):
    """the step keeps no state: a checkpoint between pushes is unaffected, and the spec — configuration — is set
    again on the restored query (a query restored without it gives the unordered rows)"""
    spec, pushes, want, cnt = om.case(fam, output, 12, 50, "count_key", 10, 1)
    a = rt.GpuQuery(spec)
    head = run_pushes(a, pushes[:2])
    blob = a.snapshot()
    a.close()
    b = rt.GpuQuery(spec)
    b.restore(blob)
    tail = run_pushes(b, pushes[2:])
    b.close()
    assert_same(abi.concat_arrays([head, tail]), want, label=f"restored {fam}")
    plain = dataclasses.replace(spec, order_by=None, limit=None, offset=None)
    c = rt.GpuQuery(plain)   # (the blob carries no trace of the spec)
    c.restore(blob)
    tail_plain = run_pushes(c, pushes[2:])
    c.close()
    d = rt.GpuQuery(plain)
    run_pushes(d, pushes[:2])
    assert_same(tail_plain, run_pushes(d, pushes[2:]), label=f"restored without the spec {fam}")
    d.close()
    assert tail_plain["ts"].size > tail["ts"].size


@pytest.mark.parametrize("fam,output,ss", [("timeBatch700", "all", 50), ("lengthBatch65sc", "current", 1),
                                           ("time500", "all", 50), ("lengthBatch4", "current", 1)])
def test_query_without_the_spec_is_untouched(rt, fam, output, ss):
    """no spec: the pass is never entered (the library's debug counter stands still), the output is the oracle's,
    sh_query_stats reports every push's events — the same through sh_push and sh_push_device — and the compact
    flush layout still applies"""
    from oracle.oracle import OracleQuery
    spec = om.make_spec(fam, output, 12, "none")
    assert not spec.has_order()
    ts, cols = om.stream(12)
    pushes = om.make_pushes(ts, cols, ss)
    o = OracleQuery(spec)
    want = run_pushes(o, pushes)
    o.close()
    import torch
    before = rt.order_debug_counts()
    g = rt.GpuQuery(spec)   # host pushes ...
    d = rt.GpuQuery(spec)   # ... and the same pushes through sh_push_device
    parts, dparts = [], []
    for p in pushes:
        if isinstance(p, tuple):
            parts.append(abi.out_arrays(g.advance_time_raw(p[1])))
            dparts.append(abi.out_arrays(d.advance_time_raw(p[1])))
            continue
        parts.append(abi.out_arrays(g.push_raw(p)))
        keep = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in [p.ts] + p.cols]
        torch.cuda.synchronize()
        dparts.append(rt.device_out_arrays(d.push_device(len(p.ts), keep[0].data_ptr(), [t.data_ptr() for t in keep[1:]], ss)))
        # sh_query_stats: the events the last push consumed, on either entry path
        assert g.stats().events == len(p.ts) == d.stats().events
    g.close()
    d.close()
    assert rt.order_debug_counts() == before
    got = abi.concat_arrays(parts)
    assert_same(got, want, label=f"untouched {fam}")
    assert_same(abi.concat_arrays(dparts), want, label=f"untouched {fam}, device pushes")
    if fam == "lengthBatch65sc" and ss == 1:
        c = rt.GpuQuery(spec)
        c.set_compact_flushes(True)
        raw = c.push_raw(pushes[0])
        assert not raw.contents.flush_offsets and raw.contents.n_flushes == raw.contents.n_rows > 0
        c.close()
        c = rt.GpuQuery(dataclasses.replace(spec, limit=1))   # ... and is ignored once a spec is set
        c.set_compact_flushes(True)
        raw = c.push_raw(pushes[0])
        assert raw.contents.flush_offsets and raw.contents.n_flushes == raw.contents.n_rows > 0
        c.close()
        assert rt.order_debug_counts()[0] == before[0] + 1


def test_refusals_on_a_live_query(rt):
    L = rt.lib()
    ts, cols = om.stream(12)
    first = split_batches(om.SCHEMA, ts, cols, [100], 0)[0]
    terms = om.TERMS["sumx_asc"]
    # set once, before the first push
    q = rt.GpuQuery(om.make_spec("timeBatch700", terms="none"))
    q.push_raw(first)
    with pytest.raises(rt.SiddhiError) as e:
        q.set_order(terms, 1, None)
    assert e.value.code == abi.SH_ERR_STATE
    q.close()
    q = rt.GpuQuery(om.make_spec("timeBatch700", terms="sumx_asc"))
    with pytest.raises(rt.SiddhiError) as e:
        q.set_order(terms, 1, None)
    assert e.value.code == abi.SH_ERR_STATE
    q.close()
    # replaceTimestampWithBatchEndTime and an order refuse each other, in either order
    q = rt.GpuQuery(om.make_spec("extTimeBatch700", terms="sumx_asc"))
    assert L.sh_query_set_ext_replace_ts(q.h, 1) == abi.SH_ERR_UNSUPPORTED and "order" in L.sh_last_error().decode()
    q.close()
    q = rt.GpuQuery(om.make_spec("extTimeBatch700", terms="none", replace_ts=True))
    with pytest.raises(rt.SiddhiError) as e:
        q.set_order(terms, None, None)
    assert e.value.code == abi.SH_ERR_UNSUPPORTED and "replaceTimestamp" in str(e.value)
    q.close()
    # the shapes sh_order_check refuses fail at creation
    for kw, word in ((dict(partition="k"), "partition"), (dict(group_by=["k", "x"]), "wide")):
        with pytest.raises(rt.SiddhiError) as e:
            rt.GpuQuery(abi.QuerySpec(om.SCHEMA, "timeBatch", 700, aggs=om.AGGS, key_capacity=32, limit=1,
                                      **({"group_by": ["k"]} | kw)))
        assert e.value.code == abi.SH_ERR_UNSUPPORTED and word in str(e.value)
    with pytest.raises(rt.SiddhiError) as e:
        rt.GpuQuery(om.make_spec("timeBatch700", terms="none", limit=-2))
    assert e.value.code == abi.SH_ERR_INVALID
