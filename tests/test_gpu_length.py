"""GPU parity of the sliding `#window.length(N)` (sh_sliding.cpp, sh_length_kernels.hip) against the Python
restatement of LengthWindowProcessor.process (:106-142) and the selector in tests/length_model.py — bit-exact
through tests.parity.assert_same. The frozen oracle has no length window; the model is pinned without a GPU
in tests/test_length_model.py (the KATs, the oracle's externalTime over ordinals, the coverage of the streams
used here). Streams are 12 000 events: the scan tile is 2048 events, the pushes are cut around it."""
import numpy as np
import pytest

from siddhi_amd import abi
from tests import kat_runner
from tests import key_edges as ke
from tests import length_model as lm
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
    N, output, ss, keys, grouped, filtered = c
    return f"N{N}-{output}-send{ss}-keys{keys}{'g' if grouped else ''}-{'filter' if filtered else 'nofilter'}"


@pytest.mark.parametrize("case", lm.gpu_matrix(), ids=case_id)
def test_length_matrix(rt, case):
    """every N edge x current / all / expired x send size 1 / 7 / 0; 1 key (without and with group-by), 12 and
    200 keys, with and without the filter; pushes cut at 1 / 2047 / 2048 / 2049 passing events, a push without
    a passing event, an ('advance', t) between pushes"""
    spec, pushes, want, cnt = lm.gpu_case(*case)
    got = gpu_run(rt, spec, pushes)
    assert_same(got, want, label=case_id(case))
    if case[0] == 10**6 and case[1] == "expired":   # nothing ever expires: no flush at all
        assert got["ts"].size == 0 and got["flush_clock"].size == 0


@pytest.mark.parametrize("wave", ["1", "0"])
@pytest.mark.parametrize("output", ["all", "expired"])
@pytest.mark.parametrize("N,keys,ss", [(2, 12, 1), (65, 12, 7), (2049, 200, 1), (64, 1, 0)])
def test_length_wave_replays(rt, monkeypatch, wave, output, N, keys, ss):
    """count / sum / min / max / avg of one double column: the wave-per-key replay (k_slx_wkey) and the lane
    walk it replaced (SH_SLX_WAVE=0), on duplicates (the deque quirk) and on residues / -0.0"""
    monkeypatch.setenv("SH_SLX_WAVE", wave)
    for values in (None, "residue"):
        spec, pushes, want, cnt = lm.gpu_case(N, output, ss, keys, True, True, aggs=lm.DAGGS, values=values)
        # (one key with all events: the current row takes the expired row's slot in every chunk)
        assert cnt["expired_rows"] > 0 or (keys == 1 and output == "all" and cnt["current_replaces_expired"] > 0)
        assert_same(gpu_run(rt, spec, pushes), want, label=f"wave={wave} N={N} {output} {values}")


def _other_keys_case(kind, output, N=65):
    """hashed long keys, a two-column (int, int) key, a dictionary (string id) key, a wide (interned) key; no filter"""
    n = 8_000
    rng = np.random.default_rng(61)
    ts = np.cumsum(rng.integers(0, 40, n)).astype(np.int64) + 5_000
    v = lm.V_DEQUE[rng.integers(1, len(lm.V_DEQUE), n)]
    x = rng.integers(-10**6, 10**6, n).astype(np.int64)
    if kind == "long":
        schema = abi.Schema.parse("k long, v double, x long, ts long")
        kc = [(rng.integers(0, 40, n).astype(np.int64) - 20) * 1_000_000_007]
        gb = ["k"]
    elif kind == "pair":
        schema = abi.Schema.parse("a int, b int, v double, x long, ts long")
        kc = [rng.integers(-3, 3, n).astype(np.int32), rng.integers(0, 5, n).astype(np.int32)]
        gb = ["a", "b"]
    elif kind == "wide":   # three columns: interned on the device into one id per distinct key
        schema = abi.Schema.parse("a int, b int, l long, v double, x long, ts long")
        kc = [rng.integers(-2, 2, n).astype(np.int32), rng.integers(0, 3, n).astype(np.int32),
              rng.integers(0, 3, n).astype(np.int64) * (1 << 40)]
        gb = ["a", "b", "l"]
    else:
        schema = abi.Schema.parse("k string, v double, x long, ts long")
        kc = [rng.integers(0, 50, n).astype(np.int32)]
        gb = ["k"]
    spec = abi.QuerySpec(schema, "length", N, group_by=gb, aggs=lm.AGGS, output=output, key_capacity=64)
    return spec, split_batches(schema, ts, kc + [v, x, ts.copy()], [1, 2_048, 5_000], 7)


@pytest.mark.parametrize("output", ["current", "all"])
@pytest.mark.parametrize("kind", ["long", "pair", "string", "wide"])
def test_length_key_kinds(rt, kind, output):
    spec, pushes = _other_keys_case(kind, output)
    want = lm.run_model(spec, pushes)
    assert want["ts"].size > 0 and want["keys"].shape[0] == len(spec.group_by)
    assert_same(gpu_run(rt, spec, pushes), want, label=f"{kind} key {output}")


@pytest.mark.parametrize("output", ["current", "all"])
def test_length_key_churn_rebuilds_table(rt, output):
    """hashed keys that appear for ~N events and never again, 3 500 distinct over the run in a 1024-slot
    table: it is rebuilt from the live keys every few pushes (current output: last ordinal + N > the passing
    count; all events: window not empty or a residue) while the dropped keys' rows were already emitted"""
    n = 20_000
    rng = np.random.default_rng(23)
    ts = np.cumsum(rng.integers(0, 3, n)).astype(np.int64) + 10_000
    k = (np.arange(n, dtype=np.int64) // 40) * 7 + rng.integers(0, 10, n)
    v = rng.integers(-400, 400, n).astype(np.float64) / 8.0
    schema = abi.Schema.parse("k long, v double, ts long")
    spec = abi.QuerySpec(schema, "length", 200, group_by=["k"], aggs=[("sum", "v"), ("count", None), ("min", "v")],
                         output=output, key_capacity=400)
    assert len(np.unique(k)) > 3_000
    pushes = split_batches(schema, ts, [k, v, ts.copy()], list(range(1_000, n, 1_000)), 1)
    assert_same(gpu_run(rt, spec, pushes), lm.run_model(spec, pushes), label=f"length churn {output}")


@pytest.mark.parametrize("output", ["current", "all", "expired"])
def test_length_pass_through(rt, output):
    ts, cols = lm.gpu_stream(12, True)
    spec = abi.QuerySpec(lm.SCHEMA, "length", 250, filter=lm.FILTER, output=output)
    pushes = lm.gpu_pushes(ts, cols, 4, True)
    want = lm.run_model(spec, pushes)
    assert want["ts"].size > 0 and (output == "current" or want["expired"].sum() > 0)
    assert_same(gpu_run(rt, spec, pushes), want, label=f"pass-through {output}")


KATS = lm.load_kats()


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_length_kat_on_gpu(rt, case):
    schema, spec, dic, flushes = kat_runner.run_query(case, rt.GpuQuery)
    kat_runner.check_query(case, flushes, schema, dic)
    lm.check_kat_extras(case, flushes)


# ---- the other entry points -------------------------------------------------------------------------------
def test_length_push_device(rt):
    import torch
    dev = torch.device("cuda", 0)
    spec, pushes, want, _ = lm.gpu_case(64, "all", 7, 12, True, True)
    g = rt.GpuQuery(spec)
    parts = []
    for p in pushes:
        if isinstance(p, tuple):
            parts.append(abi.out_arrays(g.advance_time_raw(p[1])))
            continue
        t = torch.from_numpy(p.ts).to(dev)
        cols = [torch.from_numpy(c).to(dev) for c in p.cols]
        torch.cuda.synchronize()
        out = g.push_device(len(p.ts), t.data_ptr(), [c.data_ptr() for c in cols], p.b.send_size)
        torch.cuda.synchronize()
        parts.append(rt.device_out_arrays(out))
    g.close()
    assert_same(abi.concat_arrays(parts), want, label="push_device")


def test_length_staged_ingest(rt):
    spec, pushes, want, _ = lm.gpu_case(2048, "all", 1, 200, True, False)
    batches = [p for p in pushes if not isinstance(p, tuple)]
    cap = max(len(p.ts) for p in batches)
    bufs = [rt.PinnedBatch(lm.SCHEMA, cap), rt.PinnedBatch(lm.SCHEMA, cap)]
    g = rt.GpuQuery(spec)
    parts, i = [], 0
    for p in pushes:
        if isinstance(p, tuple):
            parts.append(abi.out_arrays(g.advance_time_raw(p[1])))
            continue
        pb = bufs[i % 2].fill(p.ts, p.cols, p.b.send_size)
        parts.append(abi.out_arrays(g.push_staged_raw(g.stage(pb))))
        i += 1
    g.close()
    for b in bufs:
        b.close()
    assert_same(abi.concat_arrays(parts), want, label="staged ingest")


def last_every(out, n, grouped):
    """`output last every n events` over the selector's chunks (one flush each), plainly:
    LastPerEventOutputRateLimiter (:47-71) keeps the n-th event; LastGroupByPerEventOutputRateLimiter (:51-83)
    keeps each key's last event and sends them all, in first-seen order, at every n-th event. What one
    chunk sends is one flush at the chunk's clock."""
    counter, held = 0, {}
    rows, fo, fc = [], [0], []
    for f in range(len(out["flush_clock"])):
        sent = []
        for r in range(int(out["flush_offsets"][f]), int(out["flush_offsets"][f + 1])):
            counter += 1
            if grouped:
                held[tuple(out["keys"][:, r].tolist())] = r
            if counter == n:
                counter = 0
                sent += list(held.values()) if grouped else [r]
                held = {}
        if sent:
            rows += sent
            fo.append(len(rows))
            fc.append(int(out["flush_clock"][f]))
    idx = np.array(rows, np.int64)
    res = {"flush_offsets": np.array(fo, np.int64), "flush_clock": np.array(fc, np.int64), "val_types": out["val_types"]}
    for k in ("ts", "expired", "rep"):
        res[k] = out[k][idx]
    for k in ("keys", "vals", "nulls"):
        res[k] = out[k][:, idx]
    return res


@pytest.mark.parametrize("grouped", [True, False])
def test_length_rate_limiter_behind(rt, grouped):
    import dataclasses
    spec, pushes, want, _ = lm.gpu_case(64, "all", 7, 12 if grouped else 1, grouped, True)
    limited = last_every(want, 3, grouped)
    assert 0 < limited["ts"].size < want["ts"].size
    got = gpu_run(rt, dataclasses.replace(spec, rate=("last", 3)), pushes)
    assert_same(got, limited, label=f"last every 3 grouped={grouped}")


# ---- checkpoints --------------------------------------------------------------------------------------------
class _ModelAsOracle:
    """stands in for the oracle inside tests.test_gpu_snapshot.checkpointed"""

    def __init__(self, spec):
        self.spec = spec

    def close(self):
        pass


def _checkpointed(monkeypatch, spec, pushes, cut):
    from tests import test_gpu_snapshot as snap
    monkeypatch.setattr(snap, "OracleQuery", _ModelAsOracle)
    monkeypatch.setattr(snap, "run_pushes",
                        lambda q, p: lm.run_model(q.spec, p) if isinstance(q, _ModelAsOracle) else run_pushes(q, p))
    return snap.checkpointed(spec, pushes, cut)


@pytest.mark.parametrize("output", ["current", "all"])
@pytest.mark.parametrize("N,cut", [(4094, 2), (2048, 3), (2048, 5)])
def test_length_checkpoint(monkeypatch, output, N, cut):
    """pushes cut at 1 / 2047 / 2048 / 2049 passing events: a snapshot with the window half full (2047 of
    4094), exactly full (2048 of 2048, nothing expired yet) and with expiry under way; the restored query
    continues bit-identically"""
    spec, pushes, want, _ = lm.gpu_case(N, output, 7, 12, True, True)
    got, ref, nbytes = _checkpointed(monkeypatch, spec, pushes, cut)
    assert nbytes > 1000
    assert_same(ref, want, label="model")
    assert_same(got, ref, label=f"length({N}) ckpt {output} cut {cut}")


@pytest.mark.parametrize("output", ["current", "all"])
def test_length_checkpoint_mid_rebuild_hysteresis_and_truncated_blob(rt, output):
    """the churn stream, snapshotted after a rebuild left its hysteresis floor raised; restores from truncated
    blobs fail and leave the running query as it was"""
    n = 12_000
    rng = np.random.default_rng(29)
    ts = np.cumsum(rng.integers(0, 3, n)).astype(np.int64) + 10_000
    k = (np.arange(n, dtype=np.int64) // 40) * 7 + rng.integers(0, 10, n)
    v = rng.integers(-400, 400, n).astype(np.float64) / 8.0
    schema = abi.Schema.parse("k long, v double, ts long")
    spec = abi.QuerySpec(schema, "length", 200, group_by=["k"], aggs=[("sum", "v"), ("count", None)], output=output,
                         key_capacity=400)
    pushes = split_batches(schema, ts, [k, v, ts.copy()], list(range(1_000, n, 1_000)), 1)
    want = lm.run_model(spec, pushes)
    g = rt.GpuQuery(spec)
    a = run_pushes(g, pushes[:5])
    blob = g.snapshot()
    b = run_pushes(g, pushes[5:7])
    for cut in (24, len(blob) // 3, len(blob) - 9):
        with pytest.raises(Exception, match="truncated|does not match|restore"):
            g.restore(blob[:cut])
    c = run_pushes(g, pushes[7:])
    g.close()
    assert_same(abi.concat_arrays([a, b, c]), want, label="after failed restores")
    g2 = rt.GpuQuery(spec)
    g2.restore(blob)
    d = run_pushes(g2, pushes[5:])
    g2.close()
    assert_same(abi.concat_arrays([a, d]), want, label="restored mid-hysteresis")


# ---- what stays refused -------------------------------------------------------------------------------------
def test_length_refusals(rt):
    from siddhi_amd.shard import ShardedQuery
    E = rt.SiddhiError
    base = dict(group_by=["k"], aggs=[("count", None), ("sum", "v")], key_capacity=64)
    with pytest.raises(E, match="partition with around a sliding length window") as e:
        rt.GpuQuery(abi.QuerySpec(lm.SCHEMA, "length", 10, partition="k", **base))
    assert e.value.code == abi.SH_ERR_UNSUPPORTED
    with pytest.raises(E, match="sliding length window is not sharded") as e:
        ShardedQuery(abi.QuerySpec(lm.SCHEMA, "length", 10, **base), 0, 2)
    assert e.value.code == abi.SH_ERR_UNSUPPORTED
    with pytest.raises(E, match="a sliding length window") as e:
        rt.GpuQuery(abi.QuerySpec(lm.SCHEMA, "length", 10, having=("==", ("agg", 0), ("long", 2)), **base))
    assert e.value.code == abi.SH_ERR_UNSUPPORTED
    with pytest.raises(E, match="stream.current.event has no meaning on a sliding length window") as e:
        rt.GpuQuery(abi.QuerySpec(lm.SCHEMA, "length", 10, stream_current=True, **base))
    assert e.value.code == abi.SH_ERR_UNSUPPORTED
    for bad in (0, -3, 2**31):
        with pytest.raises(E) as e:
            rt.GpuQuery(abi.QuerySpec(lm.SCHEMA, "length", bad, **base))
        assert e.value.code == abi.SH_ERR_INVALID
    rt.GpuQuery(abi.QuerySpec(lm.SCHEMA, "length", 2**31 - 1, **base)).close()


# ---- the key table's edges ------------------------------------------------------------------------------------
def test_length_sentinel_key(rt):
    """tests/key_edges.py's LONGS: the key whose bits are the table's EMPTY mark goes to its reserved slot, its
    neighbours and the home-colliding keys probe around it"""
    ks = ke.longs()
    ts, cols, _ = ke.stream(ks, 8_000, 23, [1, 5_555])
    spec = abi.QuerySpec(ks.schema, "length", 500, group_by=ks.group_by, aggs=ke.AGGS, output="all", key_capacity=128)
    pushes = split_batches(ks.schema, ts, cols, [1, 5_555], 3)
    want = lm.run_model(spec, pushes)
    m = ke.sentinel_rows(want, ks)
    assert m.sum() > 10 and not m.all() and want["expired"][m].any()
    assert_same(gpu_run(rt, spec, pushes), want, label="sentinel key")
