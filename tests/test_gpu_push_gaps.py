"""The small kernels and copies between the four big passes of a large batch-window push (DESIGN.md §4,
"the chain between the passes"): the column scan of the multisplit's [tile][partition] counts
(k_col_reduce / k_col_lines / k_col_apply) and the push's tail, where a two-stream push has k_bits_pre
store the rows per segment (as bitmap ranks at the segment ends) and the key table's control words into
mapped host memory instead of queueing two copies behind the emission. Every case compares the GPU with
the oracle bit for bit (tests/parity.py, no tolerance).

Shapes are the smallest that reach the code: the early split needs a push of >= 2^18 events and more than
one key partition. 3,000 dictionary keys give P = 8 partitions and 100,000 give P = 256, the headline's
count (size_partitions: the dense table is the capacity rounded up to a power of two, 4,096 and 131,072
slots, over at most 512 local keys per partition; the runtime does not expose P, so this was checked by
reading size_partitions, not at run time). Tiles are 2,048 events: 300,001 events
are 147 tiles (a partial last one; 147 = 9 * 16 + 3, so the last block of kColT = 16 tiles is partial),
262,144 are 128. Base shape: `k string, v double, ts long`, timeBatch(1000) count / min / max / avg by k,
one send per event, 25 events per ms.

Case 7 of the issue names dictionary id 3,000 at key_capacity 3,000. That id lies inside the 4,096-slot
dense table and is accepted, before this change as after it; the first id the table rejects is 4,096, and
that is the one the failing push carries.
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
AGGS = [("count", None), ("min", "v"), ("max", "v"), ("avg", "v")]
KEYS = 3_000
KEYS_P256 = 100_000
N1 = 300_001          # a partial last tile; 147 tiles
NT = 262_144          # whole tiles, the smallest push that takes the early split
TILE = 2_048
COL_T = 16


def base_spec(schema=KS, keys=KEYS, **kw):
    return abi.QuerySpec(schema, "timeBatch", 1000, group_by=["k"], aggs=AGGS, key_capacity=keys, **kw)


@functools.lru_cache(maxsize=None)
def base_stream(n, keys=KEYS):
    return synth.keyed_stream(0, n, 0xC2, keys, 25)


def base_pushes(n=N1, schema=KS, keys=KEYS):
    ts, cols = base_stream(3 * n, keys)
    return split_batches(schema, ts, cols, [n, 2 * n], 1)


def case_three():
    return base_spec(), base_pushes()


def case_tiles():
    return base_spec(), base_pushes(NT)


def case_three_p256():
    return base_spec(keys=KEYS_P256), base_pushes(keys=KEYS_P256)


def case_tiles_p256():
    return base_spec(keys=KEYS_P256), base_pushes(NT, keys=KEYS_P256)


def case_one_push():
    return base_spec(), base_pushes()[:1]


def case_other_paths():
    # 262,144 events at 400 per ms (655 ms: inside the first window, nothing closes), 1,000 events on the
    # small path, then two large pushes at 25 per ms that close windows (the second starts with queued events)
    sizes = [NT, 1_000, N1, N1]
    n = sum(sizes)
    _, cols = synth.keyed_stream(0, n, 0xC2, KEYS, 25)
    a = synth.T0 + np.arange(NT, dtype=np.int64) // 400
    b = a[-1] + np.arange(1_000, dtype=np.int64) // 25
    c = b[-1] + 1 + np.arange(2 * N1, dtype=np.int64) // 25
    ts = np.concatenate([a, b, c])
    assert b[-1] - synth.T0 < 1000
    return base_spec(), split_batches(KS, ts, [cols[0], cols[1], ts.copy()], list(np.cumsum(sizes)[:-1]), 1)


def case_unsorted():
    ts, cols = base_stream(3 * N1)
    ts = ts.copy()
    ts[N1 + 150_000] -= 3   # inside push 2, below its predecessor
    return base_spec(), split_batches(KS, ts, [cols[0], cols[1], ts.copy()], [N1, 2 * N1], 1)


def case_many_windows():
    ts, cols = synth.c1_stock(0, 600_000)
    spec = abi.QuerySpec(C1, "lengthBatch", 1000, group_by=["symbol"], aggs=[("sum", "volume"), ("avg", "price")],
                         key_capacity=1000)
    return spec, split_batches(C1, ts, cols, [300_000], 100)


def case_filtered():
    return base_spec(filter=(">", "v", 100.0)), base_pushes()


def case_hashed():
    ts, cols = base_stream(3 * N1)
    k = (cols[0].astype(np.int64) * 700_001 - 1_000_000_000).astype(np.int32)  # 3,000 distinct values, both signs
    assert np.unique(k).size == KEYS
    return base_spec(KI), split_batches(KI, ts, [k, cols[1], cols[2]], [N1, 2 * N1], 1)


def case_all_events():
    return base_spec(output="all"), base_pushes()


CASES = {
    "three": case_three, "tiles": case_tiles, "three_p256": case_three_p256, "tiles_p256": case_tiles_p256,
    "one": case_one_push, "other": case_other_paths, "unsorted": case_unsorted, "windows": case_many_windows,
    "filtered": case_filtered, "hashed": case_hashed, "all": case_all_events,
}


@functools.lru_cache(maxsize=None)
def oracle_out(case):
    """The oracle's output of a case, computed once and left unchanged."""
    spec, pushes = CASES[case]()
    o = OracleQuery(spec)
    out = run_pushes(o, pushes)
    o.close()
    return out


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


def device_push(rt, g, p):
    import torch
    dev = torch.device("cuda", 0)
    ts = torch.from_numpy(p.ts).to(dev)
    cols = [torch.from_numpy(c).to(dev) for c in p.cols]
    torch.cuda.synchronize()
    try:
        out = g.push_device(len(p.ts), ts.data_ptr(), [c.data_ptr() for c in cols], p.b.send_size)
        torch.cuda.synchronize()
        return rt.device_out_arrays(out)
    finally:
        torch.cuda.synchronize()
        del ts, cols


def gpu_device(rt, spec, pushes):
    """The benchmark's path: batches in HBM, rows left in HBM (sh_push_device)."""
    g = rt.GpuQuery(spec)
    parts = [device_push(rt, g, p) for p in pushes]
    g.close()
    return abi.concat_arrays(parts)


@pytest.mark.parametrize("case", ["three", "tiles"])
def test_basic_pushes_device_and_host(rt, case):
    """Case 1: three pushes of 300,001 events (a partial last tile) and of 262,144 (whole tiles); pushes 2
    and 3 start with queued events. Device output and host output."""
    spec, pushes = CASES[case]()
    want = oracle_out(case)
    assert len(want["flush_clock"]) >= 3 * 2
    assert_same(gpu_device(rt, spec, pushes), want, label=f"{case}, device")
    assert_same(gpu_host(rt, spec, pushes), want, label=f"{case}, host")


@pytest.mark.parametrize("case", ["three_p256", "tiles_p256"])
def test_256_partitions_device_and_host(rt, case):
    """Case 2: the same pushes over 100,000 dictionary keys, P = 256 (the module docstring says how P was
    checked): k_col_lines runs 16 workgroups of 16 partitions x 64 row groups."""
    spec, pushes = CASES[case]()
    want = oracle_out(case)
    assert len(want["flush_clock"]) >= 3 * 2
    assert_same(gpu_device(rt, spec, pushes), want, label=f"{case}, device")
    assert_same(gpu_host(rt, spec, pushes), want, label=f"{case}, host")


def test_tile_count_not_a_multiple_of_the_block(rt):
    """Case 3: one push whose combined tile count (147) is above kColT = 16 and no multiple of it."""
    spec, pushes = CASES["one"]()
    tiles = -(-len(pushes[0].ts) // TILE)
    assert tiles > COL_T and tiles % COL_T != 0
    assert_same(gpu_device(rt, spec, pushes), oracle_out("one"), label="147 tiles")


def test_other_paths_before_the_large_pushes(rt):
    """Case 4: a large push that closes no window, a small push, then large pushes that close windows: the
    pushes without run_closed copy the control words as before, the later ones take them from k_bits_pre."""
    spec, pushes = CASES["other"]()
    o = OracleQuery(spec)
    per_push = [len(run_pushes(o, [p])["flush_clock"]) for p in pushes]
    o.close()
    assert per_push[0] == 0 and per_push[1] == 0 and per_push[2] >= 2 and per_push[3] >= 2
    assert_same(gpu_device(rt, spec, pushes), oracle_out("other"), label="other paths, device")
    assert_same(gpu_host(rt, spec, pushes), oracle_out("other"), label="other paths, host")


def test_unsorted_timestamp(rt):
    """Case 5: one timestamp of push 2 below its predecessor forces the redo with the prefix passes."""
    spec, pushes = CASES["unsorted"]()
    assert_same(gpu_device(rt, spec, pushes), oracle_out("unsorted"), label="unsorted")


def test_more_than_256_windows_per_push(rt):
    """Case 6: lengthBatch(1000) unfiltered, 300 windows per push (more than kFirstBounds = 256: the first
    push fetches the rest of the boundaries in a second copy, the second gets them in one); 600 segment
    ends per push go through k_bits_pre's rank stores."""
    spec, pushes = CASES["windows"]()
    want = oracle_out("windows")
    assert len(want["flush_clock"]) == 600
    assert_same(gpu_device(rt, spec, pushes), want, label="300 windows, device")
    assert_same(gpu_host(rt, spec, pushes), want, label="300 windows, host")


def test_failing_push_still_fails_and_a_fresh_query_is_exact(rt):
    """Case 7: a large push holding a dictionary id outside the dense table (4,096: see the module docstring)
    fails with SH_ERR_INVALID and check_result's text, from the control words k_bits_pre stored; the next
    valid push on a fresh query is exact."""
    spec, pushes = CASES["one"]()
    bad = pushes[0].cols[0].copy()
    bad[200_000] = 4_096
    g = rt.GpuQuery(spec)
    with pytest.raises(rt.SiddhiError, match=r"dictionary id outside \[0, key_capacity\)") as e:
        device_push(rt, g, abi.HostBatch(KS, pushes[0].ts, [bad, pushes[0].cols[1], pushes[0].cols[2]], 1))
    assert e.value.code == abi.SH_ERR_INVALID
    g.close()
    assert_same(gpu_device(rt, spec, pushes), oracle_out("one"), label="after a failed push")


@pytest.mark.parametrize("case", ["filtered", "hashed", "all"])
def test_kept_paths(rt, case):
    """Case 8: the filter v > 100, hashed `k int` keys and output="all" at the base shape."""
    spec, pushes = CASES[case]()
    want = oracle_out(case)
    assert len(want["flush_clock"]) >= 3 * 2
    assert_same(gpu_host(rt, spec, pushes), want, label=case)
    if case != "all":
        assert_same(gpu_device(rt, spec, pushes), want, label=f"{case}, device")


def test_single_stream_layout(rt, monkeypatch):
    """Case 8, SH_SIDE_STREAM=0 on a fresh query: the one-stream layout with the copies at the tail."""
    spec, pushes = CASES["three"]()
    monkeypatch.setenv("SH_SIDE_STREAM", "0")   # read when the query is created
    one = gpu_device(rt, spec, pushes)
    monkeypatch.delenv("SH_SIDE_STREAM")
    assert_same(one, oracle_out("three"), label="one stream")
    assert digest.output_digest(one) == digest.output_digest(oracle_out("three"))
