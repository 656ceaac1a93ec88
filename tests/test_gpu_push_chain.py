"""The bookkeeping chain of a large batch-window push ("two streams"): the closed-form pass
counts of an unfiltered sorted timeBatch push, the side stream that counts the queued events' tiles beside
k_boundaries and fills the bitmap / segment offsets beside the multisplit, and the spare pending buffers
the open window is compacted into beside the fold. Every case compares the GPU with the oracle bit for
bit (tests/parity.py, no tolerance); a few compare two GPU runs by their output digest.

Shapes are the smallest that reach the changed code: the early split needs a push of >= 2^18 events and
more than one key partition (3,000 dictionary keys give P = 8). Base shape: `k string, v double, ts long`,
timeBatch(1000) count / min / max / avg by k, one send per event, 25 events per ms (25k per window).

Windows closed per push on the oracle (flushes), recorded from a CPU run of every case:
  case 1  3 x 300,001 events: 12, 12, 12; 3 x 262,144 events: 10, 10, 11
  case 2  the same pushes with the filter v > 100 (50.0 % pass): 12, 12, 12
  case 3  300,001 -> 12; 262,144 at 400 per ms -> 0; 1,000 -> 0; 300,001 -> 12
  case 4  one timestamp of push 2 below its predecessor: 12, 12, 12
  case 5  k int, 3,000 hashed values: 12, 12, 12
  case 6  one host-fed push of 300,001 events: 12 (sh_push with host output is also how cases 2-5, 7 and 8
          run; cases 1-5 and 9 run from HBM with device output as well)
  case 7  snapshot after push 1, restored into a fresh query: 12 | 12, 12
  case 8  output="all": 12, 12, 12; having count() >= 2 (two pushes: the Python selector model takes
          1.6 s per push): 12, 12
  case 9  lengthBatch(1000), filter price > 100 (50.0 % pass), 2 x 300,000 events: 150, 150
  case 10 as case 1
"""
import dataclasses
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
AGGS = [("count", None), ("min", "v"), ("max", "v"), ("avg", "v")]
KEYS = 3_000
N1 = 300_001          # a partial last tile
NT = 262_144          # a whole number of tiles, the smallest push that takes the early split


def base_spec(schema=KS, **kw):
    return abi.QuerySpec(schema, "timeBatch", 1000, group_by=["k"], aggs=AGGS, key_capacity=KEYS, **kw)


@functools.lru_cache(maxsize=None)
def base_stream(n):
    return synth.keyed_stream(0, n, 0xC2, KEYS, 25)


def base_pushes(n=N1, schema=KS):
    ts, cols = base_stream(3 * n)
    return split_batches(schema, ts, cols, [n, 2 * n], 1)


@functools.lru_cache(maxsize=None)
def oracle_out(case):
    """The oracle's output of a case, computed once (spec and pushes come from CASES)."""
    spec, pushes = CASES[case]()
    o = OracleQuery(spec)
    out = run_pushes(o, pushes)
    o.close()
    return out


def case_three_pushes():
    return base_spec(), base_pushes()


def case_whole_tiles():
    return base_spec(), base_pushes(NT)


def case_filtered():
    return base_spec(filter=(">", "v", 100.0)), base_pushes()


def case_mixed():
    # 300,001 events at 25 per ms; 262,144 at 400 per ms inside the window the first push left open (no
    # window closes: the push appends in place after a swap); 1,000 events on the small path; 300,001 again
    sizes = [N1, NT, 1_000, N1]
    n = sum(sizes)
    _, cols = synth.keyed_stream(0, n, 0xC2, KEYS, 25)
    t0 = synth.T0
    a = t0 + np.arange(N1, dtype=np.int64) // 25
    b = a[-1] + 1 + np.arange(NT, dtype=np.int64) // 400
    c = b[-1] + 1 + np.arange(1_000, dtype=np.int64) // 25
    d = c[-1] + 1 + np.arange(N1, dtype=np.int64) // 25
    ts = np.concatenate([a, b, c, d])
    cuts = list(np.cumsum(sizes)[:-1])
    return base_spec(), split_batches(KS, ts, [cols[0], cols[1], ts.copy()], cuts, 1)


def case_unsorted():
    ts, cols = base_stream(3 * N1)
    ts = ts.copy()
    ts[N1 + 150_000] -= 3   # inside push 2, below its predecessor
    return base_spec(), split_batches(KS, ts, [cols[0], cols[1], ts.copy()], [N1, 2 * N1], 1)


def case_hashed():
    ts, cols = base_stream(3 * N1)
    k = (cols[0].astype(np.int64) * 700_001 - 1_000_000_000).astype(np.int32)  # 3,000 distinct values, both signs
    assert np.unique(k).size == KEYS
    return base_spec(KI), split_batches(KI, ts, [k, cols[1], cols[2]], [N1, 2 * N1], 1)


def case_all_events():
    return base_spec(output="all"), base_pushes()


def case_lengthbatch():
    ts, cols = synth.c1_stock(0, 600_000)
    spec = abi.QuerySpec(C1, "lengthBatch", 1000, group_by=["symbol"], aggs=[("sum", "volume"), ("avg", "price")],
                         filter=(">", "price", 100), key_capacity=1000)
    return spec, split_batches(C1, ts, cols, [300_000], 100)


CASES = {
    "three": case_three_pushes, "tiles": case_whole_tiles, "filtered": case_filtered, "mixed": case_mixed,
    "unsorted": case_unsorted, "hashed": case_hashed, "all": case_all_events, "lengthbatch": case_lengthbatch,
}


@pytest.fixture(scope="module")
def rt():
    from siddhi_amd import runtime
    return runtime


def gpu_host(rt, spec, pushes):
    """Host-fed pushes with host output (sh_push): run_closed synchronises and finishes the rows itself."""
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


def flushes_per_push(spec, pushes):
    """Windows the oracle closes in each push (the docstring's figures; also run on the CPU alone)."""
    o = OracleQuery(spec)
    n = [len(run_pushes(o, [p])["flush_clock"]) for p in pushes]
    o.close()
    return n


def test_three_pushes_device_and_host_and_single_stream(rt, monkeypatch):
    """Case 1: partial last tile, ~12 windows per push, pushes 2 and 3 start with queued events (np_t > 0)
    and with the spare set swapped in. The one-stream form gives the same digest."""
    spec, pushes = CASES["three"]()
    want = oracle_out("three")
    assert len(want["flush_clock"]) >= 3 * 2
    dev = gpu_device(rt, spec, pushes)
    assert_same(dev, want, label="three pushes, device")
    assert_same(gpu_host(rt, spec, pushes), want, label="three pushes, host")
    monkeypatch.setenv("SH_SIDE_STREAM", "0")   # read when the query is created
    one = gpu_device(rt, spec, pushes)
    monkeypatch.delenv("SH_SIDE_STREAM")
    assert digest.output_digest(one) == digest.output_digest(dev)


def test_whole_tiles(rt):
    """Case 1, pushes of exactly 262,144 events: the last tile is full and writes the totals."""
    spec, pushes = CASES["tiles"]()
    assert_same(gpu_device(rt, spec, pushes), oracle_out("tiles"), label="whole tiles")


def test_filtered_pushes_keep_the_scan_chain(rt):
    """Case 2: FK = 1, about half the events pass; tile counts are scanned and k_fix_bounds runs."""
    spec, pushes = CASES["filtered"]()
    want = oracle_out("filtered")
    frac = sum(int((p.cols[1] > 100.0).sum()) for p in pushes) / (3 * N1)
    assert 0.4 < frac < 0.6
    assert_same(gpu_host(rt, spec, pushes), want, label="filtered")
    assert_same(gpu_device(rt, spec, pushes), want, label="filtered, device")


def test_mixed_push_sizes_on_one_query(rt):
    """Case 3: large, large without a close (appends in place after a swap), small path, large."""
    spec, pushes = CASES["mixed"]()
    assert flushes_per_push(spec, pushes[:2])[1] == 0
    assert_same(gpu_host(rt, spec, pushes), oracle_out("mixed"), label="mixed sizes")
    assert_same(gpu_device(rt, spec, pushes), oracle_out("mixed"), label="mixed sizes, device")


def test_unsorted_timestamp_redoes_the_window_assignment(rt):
    """Case 4: the single-pass form reports `unsorted` with the side-stream count already queued."""
    spec, pushes = CASES["unsorted"]()
    assert_same(gpu_device(rt, spec, pushes), oracle_out("unsorted"), label="unsorted")


def test_hashed_keys(rt):
    """Case 5: `k int`, hashed slots (the slot column is written and read by every side-stream kernel)."""
    spec, pushes = CASES["hashed"]()
    assert_same(gpu_device(rt, spec, pushes), oracle_out("hashed"), label="hashed keys")
    assert_same(gpu_host(rt, spec, pushes), oracle_out("hashed"), label="hashed keys, host")


def test_host_output_of_one_large_push(rt):
    """Case 6: sh_push of a HostBatch of 300,001 events: run_closed waits and finishes the rows itself."""
    spec, pushes = CASES["three"]()
    o = OracleQuery(spec)
    want = run_pushes(o, pushes[:1])
    o.close()
    assert len(want["flush_clock"]) >= 2
    assert_same(gpu_host(rt, spec, pushes[:1]), want, label="host output")


def test_snapshot_after_a_swap_and_restore(rt):
    """Case 7: the snapshot after push 1 reads the swapped-in buffers; a fresh query continues from it."""
    spec, pushes = CASES["three"]()
    g = rt.GpuQuery(spec)
    a = run_pushes(g, pushes[:1])
    blob = g.snapshot()
    g.close()
    g2 = rt.GpuQuery(spec)
    g2.restore(blob)
    b = run_pushes(g2, pushes[1:])
    g2.close()
    assert_same(abi.concat_arrays([a, b]), oracle_out("three"), label="snapshot / restore")


def test_all_events_output(rt):
    """Case 8a: output="all" (expired rows of the batch before, xmode)."""
    spec, pushes = CASES["all"]()
    want = oracle_out("all")
    assert want["expired"].any()
    assert_same(gpu_host(rt, spec, pushes), want, label="all events")


def test_having_program(rt):
    """Case 8b: `having count() >= 2` (hv.on keeps the one stream), against tests/having_model.py."""
    from tests import having_model as hm
    spec, pushes = CASES["three"]()
    spec = dataclasses.replace(spec, having=(">=", ("agg", 0), 2))
    pushes = pushes[:2]
    want = hm.run_model(spec, pushes)
    assert len(want["flush_clock"]) >= 2 * 2
    assert_same(gpu_host(rt, spec, pushes), want, label="having")


def test_lengthbatch_early_split(rt):
    """Case 9: not the single-pass form, but the early split and the side stream apply (P = 2)."""
    spec, pushes = CASES["lengthbatch"]()
    want = oracle_out("lengthbatch")
    assert len(want["flush_clock"]) >= 2 * 2
    assert_same(gpu_host(rt, spec, pushes), want, label="lengthBatch")
    assert_same(gpu_device(rt, spec, pushes), want, label="lengthBatch, device")


def test_two_fresh_queries_give_one_digest(rt):
    """Case 10: determinism of the two-stream push."""
    spec, pushes = CASES["three"]()
    a = digest.output_digest(gpu_device(rt, spec, pushes))
    b = digest.output_digest(gpu_device(rt, spec, pushes))
    assert a == b == digest.output_digest(oracle_out("three"))
