"""The multisplit fold ("persistent fold"): k_aggregate_own as a persistent grid whose
workgroups take every grid-th (window, key partition) unit and keep the next chunk's records in flight, and
the first-occurrence bitmap words its rows are emitted from. Every case compares the GPU with the oracle
bit for bit (tests/parity.py, no tolerance); the switch case compares GPU runs by their output digest as
well. (The per-unit first lists and k_first_words of the same issue were measured and dropped, DESIGN.md
§4, so there is no SH_FOLD_FIRST_LIST to switch.)

Base shape: `k string, v double, ts long`, timeBatch(1000) count / min / max / avg by k, 3,000 dictionary
keys (P = 8 key partitions, so a unit is one of 8 partitions of a window), one send per event, pushes of
300,001 events (262,144 in case 3): the smallest that take the early split.

Windows closed per push on the oracle (flushes), recorded from a CPU run of every case:
  case 1  25 events per ms, 3 x 300,001: 12, 12, 12 (about 3,100 records per unit: one chunk)
  case 2  100 per ms, 3 x 300,001: 3, 3, 3 (about 12,500 records per unit: four chunks, the last partial)
  case 3  3 per ms, 3 x 262,144: 87, 87, 88 (about 700 units per push, 375 records each: more units than
          the persistent grid, and keys without events in a window)
  case 4  case 1 with window 5 of every push holding keys = 0 (mod 8) only (7 of its 8 units empty): 12, 12, 12
  case 5  k int, 3,000 hashed values (K = 2: the sentinel slot's second key per owner): 12, 12, 12
  case 5b case 5's keys on case 3's stream, one window per push holding a single key: 87, 87, 88
  case 6  lengthBatch(1000) sum(volume), avg(price) by symbol, 3,000 symbols, 2 x 300,000: 300, 300 (R = 4);
          four value columns, timeBatch(1000), 2 x 300,001 at 25 per ms: 12, 12 (R = 2, table-driven fold)
  case 7  output="all" on case 1's stream: 12, 12, 12
  case 8  case 1 with SH_FOLD_GRID=0 (one workgroup per unit): as case 1
  case 9  snapshot after push 1 of case 1, restored into a fresh query: 12 | 12, 12
"""
import functools

import numpy as np
import pytest

from oracle.oracle import OracleQuery
from siddhi_amd import abi, digest, synth
from tests.parity import assert_same, run_pushes, split_batches

pytestmark = pytest.mark.gpu

KS = abi.Schema.parse("k string, v double, ts long")
KI = abi.Schema.parse("k int, v double, ts long")
C1 = abi.Schema.parse("symbol string, price double, volume long, ts long")
K4 = abi.Schema.parse("k string, a double, b double, c long, d long, ts long")
AGGS = [("count", None), ("min", "v"), ("max", "v"), ("avg", "v")]
KEYS = 3_000
N1 = 300_001          # a partial last tile
NT = 262_144          # the smallest push that takes the early split


def base_spec(schema=KS, **kw):
    return abi.QuerySpec(schema, "timeBatch", 1000, group_by=["k"], aggs=AGGS, key_capacity=KEYS, **kw)


@functools.lru_cache(maxsize=None)
def stream(n, per_ms):
    return synth.keyed_stream(0, n, 0xC2, KEYS, per_ms)


def pushes_of(per_ms, n=N1, schema=KS):
    ts, cols = stream(3 * n, per_ms)
    return split_batches(schema, ts, cols, [n, 2 * n], 1)


def case_one_chunk():
    return base_spec(), pushes_of(25)


def case_four_chunks():
    return base_spec(), pushes_of(100)


def case_many_units():
    return base_spec(), pushes_of(3, NT)


def case_empty_units():
    # window 5 of every push (12 windows of 25,000 events each per push; the windows are aligned to the
    # first event's millisecond) keeps only keys that are multiples of 8: partitions 1..7 get no record
    ts, cols = stream(3 * N1, 25)
    k = cols[0].copy()
    win = (ts - ts[0]) // 1000
    for w in (5, 17, 29):
        m = win == w
        assert m.sum() == 25_000
        k[m] -= k[m] % 8
    return base_spec(), split_batches(KS, ts, [k, cols[1], cols[2]], [N1, 2 * N1], 1)


def case_hashed():
    ts, cols = stream(3 * N1, 25)
    k = (cols[0].astype(np.int64) * 700_001 - 1_000_000_000).astype(np.int32)  # 3,000 distinct values, both signs
    assert np.unique(k).size == KEYS
    return base_spec(KI), split_batches(KI, ts, [k, cols[1], cols[2]], [N1, 2 * N1], 1)


def case_hashed_sparse():
    # case 5's hashed keys at 3 events per ms on 262,144-event pushes (about 700 units per push, many keys
    # absent from a window), and one window per push reduced to a single key: every other unit of that
    # window is empty and is followed directly by the next unit's epilogue on the K = 2 row path
    n = NT
    ts, cols = stream(3 * n, 3)
    k0 = cols[0].copy()
    win = (ts - ts[0]) // 1000
    for w in (40, 130, 220):
        m = win == w
        assert m.sum() == 3_000
        k0[m] = 8
    k = (k0.astype(np.int64) * 700_001 - 1_000_000_000).astype(np.int32)
    return base_spec(KI), split_batches(KI, ts, [k, cols[1], cols[2]], [n, 2 * n], 1)


def case_two_columns():
    ts, cols = synth.c1_stock(0, 600_000, symbols=KEYS)
    spec = abi.QuerySpec(C1, "lengthBatch", 1000, group_by=["symbol"], aggs=[("sum", "volume"), ("avg", "price")],
                         key_capacity=KEYS)
    return spec, split_batches(C1, ts, cols, [300_000], 1)


def case_four_columns():
    n = 2 * N1
    ts, cols = stream(3 * N1, 25)
    d = synth.draws(0xF4, 0, n, 3)
    b = synth.uniform_price(d[:, 0])
    c = (synth.hi53(d[:, 1]) % np.uint64(10_000)).astype(np.int64) - 5_000
    e = (synth.hi53(d[:, 2]) % np.uint64(1_000_000)).astype(np.int64)
    spec = abi.QuerySpec(K4, "timeBatch", 1000, group_by=["k"],
                         aggs=[("sum", "a"), ("max", "b"), ("sum", "c"), ("min", "d")], key_capacity=KEYS)
    return spec, split_batches(K4, ts[:n], [cols[0][:n], cols[1][:n], b, c, e, ts[:n].copy()], [N1], 1)


def case_all_events():
    return base_spec(output="all"), pushes_of(25)


CASES = {
    "one_chunk": case_one_chunk, "four_chunks": case_four_chunks, "many_units": case_many_units,
    "empty_units": case_empty_units, "hashed": case_hashed, "hashed_sparse": case_hashed_sparse, "two_columns": case_two_columns,
    "four_columns": case_four_columns, "all": case_all_events,
}


@functools.lru_cache(maxsize=None)
def oracle_out(case):
    """The oracle's output of a case and the windows it closes in each push, computed once."""
    spec, pushes = CASES[case]()
    o = OracleQuery(spec)
    parts = [run_pushes(o, [p]) for p in pushes]
    o.close()
    return abi.concat_arrays(parts), [len(p["flush_clock"]) for p in parts]


def want_of(case, min_flushes=1):
    """The oracle's output; every push of the case closes at least `min_flushes` windows."""
    out, flushes = oracle_out(case)
    assert all(f >= min_flushes for f in flushes), f"{case}: windows closed per push {flushes}"
    return out


@pytest.fixture(scope="module")
def rt():
    from siddhi_amd import runtime
    return runtime


def gpu_host(rt, spec, pushes):
    """Host-fed pushes with host output (sh_push)."""
    g = rt.GpuQuery(spec)
    out = run_pushes(g, pushes)
    g.close()
    return out


def gpu_device(rt, spec, pushes):
    """The benchmark's path: batches in HBM, rows left in HBM (sh_push_device)."""
    import torch
    dev = torch.device("cuda", 0)
    g = rt.GpuQuery(spec)
    parts = []
    for p in pushes:
        ts = torch.from_numpy(p.ts).to(dev)
        cols = [torch.from_numpy(c).to(dev) for c in p.cols]
        torch.cuda.synchronize()
        out = g.push_device(len(p.ts), ts.data_ptr(), [c.data_ptr() for c in cols], p.b.send_size)
        torch.cuda.synchronize()
        parts.append(rt.device_out_arrays(out))
        del ts, cols
    g.close()
    return abi.concat_arrays(parts)


def test_one_chunk_per_unit(rt):
    """Case 1: 96 units per push, one chunk each; pushes 2 and 3 start with pending events, and the
    25,000-event windows straddle the bitmap's 2,048-word tiles."""
    spec, pushes = CASES["one_chunk"]()
    want = want_of("one_chunk")
    assert_same(gpu_device(rt, spec, pushes), want, label="one chunk, device")
    assert_same(gpu_host(rt, spec, pushes), want, label="one chunk, host")


def test_four_chunks_per_unit(rt):
    """Case 2: about 12,500 records per unit, the prefetch across the chunks of one unit; the last chunk
    is partial."""
    spec, pushes = CASES["four_chunks"]()
    n_unit = 100_000 / 8
    assert 3 * 4096 < n_unit < 4 * 4096
    assert_same(gpu_device(rt, spec, pushes), want_of("four_chunks"), label="four chunks")


def test_more_units_than_the_grid(rt):
    """Case 3: 87 windows x 8 partitions per push, more than the 512 workgroups resident at once; a window
    has 3,000 events over 3,000 keys, so about a third of the keys are absent from it (holes in the row
    region)."""
    spec, pushes = CASES["many_units"]()
    want = want_of("many_units", min_flushes=80)
    rows_per_window = np.diff(want["flush_offsets"])
    assert rows_per_window.max() < KEYS * 0.75
    assert_same(gpu_device(rt, spec, pushes), want, label="many units")


def test_empty_units(rt):
    """Case 4: one window per push whose events all fall in key partition 0."""
    spec, pushes = CASES["empty_units"]()
    want = want_of("empty_units")
    assert np.diff(want["flush_offsets"]).min() <= KEYS // 8
    assert_same(gpu_device(rt, spec, pushes), want, label="empty units")


def test_hashed_keys_two_per_owner(rt):
    """Case 5: `k int`, hashed slots, K = 2."""
    spec, pushes = CASES["hashed"]()
    assert_same(gpu_device(rt, spec, pushes), want_of("hashed"), label="hashed keys")


def test_hashed_keys_sparse_windows_and_empty_units(rt):
    """Case 5b: K = 2 with more units than the grid, keys absent from windows and, once per push, a window
    of one key (its other units are empty), under the grid and with one workgroup per unit."""
    spec, pushes = CASES["hashed_sparse"]()
    want = want_of("hashed_sparse", min_flushes=80)
    assert np.diff(want["flush_offsets"]).min() == 1
    assert_same(gpu_device(rt, spec, pushes), want, label="hashed, sparse")


def test_two_value_columns(rt):
    """Case 6a: lengthBatch(1000) sum(volume), avg(price): R = 4, 2,400 units per push (two value columns:
    one workgroup per unit, the prefetch only from chunk to chunk)."""
    spec, pushes = CASES["two_columns"]()
    want = want_of("two_columns", min_flushes=250)
    assert_same(gpu_device(rt, spec, pushes), want, label="two columns")
    assert_same(gpu_host(rt, spec, pushes), want, label="two columns, host")


def test_four_value_columns(rt):
    """Case 6b: four value columns, the table-driven fold with R = 2."""
    spec, pushes = CASES["four_columns"]()
    assert_same(gpu_device(rt, spec, pushes), want_of("four_columns"), label="four columns")


def test_all_events_output(rt):
    """Case 7: output="all", whose expired rows read the bitmap words of the batch before."""
    spec, pushes = CASES["all"]()
    want = want_of("all")
    assert want["expired"].any()
    assert_same(gpu_host(rt, spec, pushes), want, label="all events")


def test_switches_give_one_digest(rt, monkeypatch):
    """Case 8: one workgroup per unit (SH_FOLD_GRID=0) on a fresh query (the switch is read when a query is
    created), for the one-chunk and the many-unit shapes."""
    for case in ("one_chunk", "many_units"):
        spec, pushes = CASES[case]()
        want = want_of(case)
        outs = [gpu_device(rt, spec, pushes)]
        monkeypatch.setenv("SH_FOLD_GRID", "0")
        outs.append(gpu_device(rt, spec, pushes))
        monkeypatch.delenv("SH_FOLD_GRID")
        for o in outs:
            assert_same(o, want, label="switch, " + case)
        assert len({digest.output_digest(o) for o in outs}) == 1


def test_snapshot_and_restore(rt):
    """Case 9: a snapshot after push 1, restored into a fresh query that takes pushes 2 and 3."""
    spec, pushes = CASES["one_chunk"]()
    g = rt.GpuQuery(spec)
    a = run_pushes(g, pushes[:1])
    blob = g.snapshot()
    g.close()
    g2 = rt.GpuQuery(spec)
    g2.restore(blob)
    b = run_pushes(g2, pushes[1:])
    g2.close()
    assert_same(abi.concat_arrays([a, b]), want_of("one_chunk"), label="snapshot / restore")
