"""First-occurrence marks as epoch bytes and the XCD-contiguous unit order of the persistent fold
("Epoch marks and XCD runs"): the fold stores the push's epoch byte at a row's first event
instead of an atomic on the bitmap word, k_flags_tile packs the bytes into the bitmap words (run_closed
takes the bytes where the push can have a mark per 32 closed events — its row bound times 32 reaches the
closed events — and the atomics elsewhere; SH_FIRST_FLAGS=1 / 0 force one form), and with a grid that is a
multiple of 8 every XCD takes one contiguous run of the fold's units
(SH_XCD_WINDOWS). The same order for the emission's blocks was measured and dropped, so the emission is
the parent's and there is nothing of it to switch. Every case compares the GPU with the oracle bit for
bit (tests/parity.py, no tolerance); the switch case compares the runs' output digests as well.

Base shape, as tests/test_gpu_fold_chain.py: `k string, v double, ts long`, timeBatch(1000) count / min /
max / avg by k, 3,000 dictionary keys (P = 8 key partitions: a unit is one of 8 partitions of a window), one
send per event, pushes of 300,001 events or 262,144 (the smallest that takes the early split).

Windows closed per push on the oracle (flushes), recorded from a CPU run of every case:
  case 1   25 events per ms, 3 x 300,001: 12, 12, 12 (96 units per push: the grid is the unit count, a
           multiple of 8, so every XCD has a run of 12 units, one per workgroup)
  case 2   3 per ms, 3 x 262,144: 87, 87, 88 (696 / 704 units on a grid of 512 where two workgroups per
           CU are resident: runs of 87 or 88 units that end inside a window, 64 workgroups per run, the
           second round of a run shorter than the first)
  case 3   200 per ms, 2 x 300,001: 1, 2 (8 units: one per XCD; 16 units: runs of two, a window over
           four XCDs. With P = 8 the unit count is a multiple of 8, per = n_units / 8 exactly, so no XCD's
           run of units is empty and every workgroup has a first unit: a workgroup without one needs more
           units than the grid and a count that is no multiple of 8 (P < 8 and hundreds of windows).
           Case 11's grid of 26 units is the one no run applies to. At most 3,001 rows per 200,000-event
           window: the atomics by default, so the case also runs with SH_FIRST_FLAGS=1.)
  case 4   SH_FLAG_EPOCH0=254, 4 x 300,001 of case 1's stream: 12, 12, 12, 12 (epochs 254, 255, 1, 2)
  case 5   25 per ms, pushes of 262,144, 600,002 and 262,144: 10, 24, 10
  case 6   500 keys (P = 1), 300,001 events at 100 per ms, 20,000 at 10 per ms, 300,001 at 100 per ms:
           3, 2, 3 (windows of 100,000 events take the multisplit fold — 501 rows at most each: the atomics
           by default — and the middle push's two windows of at most 10,000 events take k_aggregate_flat
           with the bytes; also run with SH_FIRST_FLAGS=1, every push with the bytes)
  case 7   k int, 3,000 hashed values (K = 2) on case 2's stream: 87, 87, 88
  case 8   output="all" on case 1's stream: 12, 12, 12
  case 9   cases 1 and 2 (both take the bytes by default) with SH_FIRST_FLAGS=0, SH_XCD_WINDOWS=0, both,
           SH_FOLD_GRID=0, and SH_FIRST_FLAGS=1: as cases 1, 2
  case 10  a failing push of case 1 (dictionary id 4,096, outside the 4,096-slot table), then case 1 on a
           fresh query: 12, 12, 12
  case 11  1,000 keys (P = 2: size_partitions gives P = 2 for a 1,024-slot and 4 for a 2,048-slot table,
           so nseg * P need not be a multiple of 8), 23 per ms, 3 x 300,001: 13, 13, 13 (26 units: the grid
           is the unit count and no multiple of 8, the order b, b + grid, ... stays)
  case 12  1,000 keys (P = 2), 1 per ms, 2 x 262,144: 262, 262 (524 units on the grid of 512: per = 66, the
           last XCD's run is units 462..523, so its workgroups 62 and 63 — units 524 and 525 — have no unit
           at all, and the other runs' second round takes 2 of 64 workgroups)
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
AGGS = [("count", None), ("min", "v"), ("max", "v"), ("avg", "v")]
KEYS = 3_000
N1 = 300_001          # a partial last tile
NT = 262_144          # the smallest push that takes the early split


def base_spec(schema=KS, keys=KEYS, **kw):
    return abi.QuerySpec(schema, "timeBatch", 1000, group_by=["k"], aggs=AGGS, key_capacity=keys, **kw)


@functools.lru_cache(maxsize=None)
def stream(n, per_ms, keys=KEYS):
    return synth.keyed_stream(0, n, 0xC2, keys, per_ms)


def even_pushes(per_ms, n, count=3, schema=KS, keys=KEYS):
    ts, cols = stream(count * n, per_ms, keys)
    return split_batches(schema, ts, cols, [n * i for i in range(1, count)], 1)


def case_grid_is_units():
    return base_spec(), even_pushes(25, N1)


def case_many_units():
    return base_spec(), even_pushes(3, NT)


def case_few_windows():
    return base_spec(), even_pushes(200, N1, count=2)


def case_four_pushes():
    return base_spec(), even_pushes(25, N1, count=4)


def case_regrow():
    n = NT + 600_002 + NT
    ts, cols = stream(n, 25)
    return base_spec(), split_batches(KS, ts, cols, [NT, NT + 600_002], 1)


def case_flat_between():
    # one partition (500 keys in a 512-slot table): windows of 65,536 events or more take the multisplit
    # fold, shorter ones k_aggregate_flat. 100 events per ms, then 20,000 events at 10 per ms, then 100 again
    keys, small = 500, 20_000
    n = 2 * N1 + small
    _, cols = stream(n, 100, keys)
    step = np.concatenate([np.arange(N1) // 100, N1 // 100 + 1 + np.arange(small) // 10])
    step = np.concatenate([step, step[-1] + 1 + np.arange(N1) // 100])
    ts = (synth.T0 + step).astype(np.int64)
    return base_spec(keys=keys), split_batches(KS, ts, [cols[0], cols[1], ts.copy()], [N1, N1 + small], 1)


def case_hashed_many_units():
    ts, cols = stream(3 * NT, 3)
    k = (cols[0].astype(np.int64) * 700_001 - 1_000_000_000).astype(np.int32)  # 3,000 distinct values, both signs
    assert np.unique(k).size == KEYS
    return base_spec(KI), split_batches(KI, ts, [k, cols[1], cols[2]], [NT, 2 * NT], 1)


def case_all_events():
    return base_spec(output="all"), even_pushes(25, N1)


def case_two_partitions():
    return base_spec(keys=1_000), even_pushes(23, N1, keys=1_000)


def case_workgroups_without_a_unit():
    return base_spec(keys=1_000), even_pushes(1, NT, count=2, keys=1_000)


CASES = {
    "grid_is_units": case_grid_is_units, "many_units": case_many_units, "few_windows": case_few_windows,
    "four_pushes": case_four_pushes, "regrow": case_regrow, "flat_between": case_flat_between,
    "hashed_many_units": case_hashed_many_units, "all": case_all_events, "two_partitions": case_two_partitions,
    "no_unit": case_workgroups_without_a_unit,
}
# windows closed per push on the oracle (the module docstring's record)
FLUSHES = {
    "grid_is_units": [12, 12, 12], "many_units": [87, 87, 88], "few_windows": [1, 2],
    "four_pushes": [12, 12, 12, 12], "regrow": [10, 24, 10], "flat_between": [3, 2, 3],
    "hashed_many_units": [87, 87, 88], "all": [12, 12, 12], "two_partitions": [13, 13, 13],
    "no_unit": [262, 262],
}


@functools.lru_cache(maxsize=None)
def oracle_out(case):
    """The oracle's output of a case and the windows it closes in each push, computed once."""
    spec, pushes = CASES[case]()
    o = OracleQuery(spec)
    parts = [run_pushes(o, [p]) for p in pushes]
    o.close()
    return abi.concat_arrays(parts), [len(p["flush_clock"]) for p in parts]


def want_of(case):
    """The oracle's output; every push of the case closes the windows the module docstring states."""
    out, flushes = oracle_out(case)
    assert flushes == FLUSHES[case], f"{case}: windows closed per push {flushes}"
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


def both_paths(rt, case):
    spec, pushes = CASES[case]()
    want = want_of(case)
    assert_same(gpu_device(rt, spec, pushes), want, label=case + ", device")
    assert_same(gpu_host(rt, spec, pushes), want, label=case + ", host")


def test_grid_is_the_unit_count(rt):
    """Case 1: 96 units per push on a grid of 96, runs of 12 units per XCD; pushes 2 and 3 start with
    pending events."""
    both_paths(rt, "grid_is_units")


def test_more_units_than_the_grid(rt):
    """Case 2: about 700 units per push; the XCDs' runs end inside windows, and 87 windows are not a
    multiple of 8."""
    both_paths(rt, "many_units")


@pytest.mark.parametrize("flags", [None, "1"])
def test_fewer_than_eight_windows(rt, monkeypatch, flags):
    """Case 3: a push that closes exactly one window (8 units, one per XCD), then one that closes two (16
    units, runs of two); with the form of the marks the push takes by default and with the bytes."""
    if flags:
        monkeypatch.setenv("SH_FIRST_FLAGS", flags)
    both_paths(rt, "few_windows")


def test_epoch_wraps(rt, monkeypatch):
    """Case 4: epochs 254, 255, 1, 2. What this catches is an epoch of 0 or 256 at the wrap (a zeroed or
    truncated byte would match no mark, or every cleared byte) and a fill at the wrap that damages the
    push. It cannot show that the fill is needed: before the wrap only bytes 254 and 255 exist, after it
    only 1 and 2 are compared, and a stale byte aliases only 255 calls later, which no quick test reaches."""
    monkeypatch.setenv("SH_FLAG_EPOCH0", "254")
    both_paths(rt, "four_pushes")


def test_flags_regrown_then_used_below_capacity(rt):
    """Case 5: the 600,002-event push regrows the flag bytes (cleared, nothing carried over); the third
    push uses less than the capacity, with the second's marks behind its last closed event."""
    both_paths(rt, "regrow")


@pytest.mark.parametrize("flags", [None, "1"])
def test_flat_units_between_large_pushes(rt, monkeypatch, flags):
    """Case 6: the middle push's windows go through k_aggregate_flat, which marks through the same bytes;
    the pushes around it take the multisplit fold with one partition — with the atomics by default (the
    epoch advances only on the middle push), with the bytes and consecutive epochs under SH_FIRST_FLAGS=1."""
    if flags:
        monkeypatch.setenv("SH_FIRST_FLAGS", flags)
    both_paths(rt, "flat_between")


def test_hashed_keys_many_units(rt):
    """Case 7: `k int`, hashed slots, K = 2 (both marks of a thread), more units than the grid and rows
    with holes in the row region."""
    both_paths(rt, "hashed_many_units")


def test_all_events_output(rt):
    """Case 8: output="all", whose expired rows read the bitmap words of the batch before."""
    spec, pushes = CASES["all"]()
    want = want_of("all")
    assert want["expired"].any()
    assert_same(gpu_host(rt, spec, pushes), want, label="all events")


SWITCHES = [{}, {"SH_FIRST_FLAGS": "0"}, {"SH_XCD_WINDOWS": "0"}, {"SH_FIRST_FLAGS": "0", "SH_XCD_WINDOWS": "0"},
            {"SH_FOLD_GRID": "0"}, {"SH_FIRST_FLAGS": "1"}]


@pytest.mark.parametrize("case", ["grid_is_units", "many_units"])
def test_switches_give_one_digest(rt, monkeypatch, case):
    """Case 9: the issue's five settings of the switches and the forced bytes, a fresh query each (they are
    read when a query is created)."""
    spec, pushes = CASES[case]()
    want = want_of(case)
    digests = set()
    for env in SWITCHES:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            out = gpu_device(rt, spec, pushes)
        assert_same(out, want, label=f"{case}, {env}")
        digests.add(digest.output_digest(out))
    assert len(digests) == 1


def test_failing_push_then_a_fresh_query(rt):
    """Case 10: a push holding a dictionary id outside the dense table fails after run_closed has taken
    its epoch and the fold has stored marks; a fresh query is exact. The fresh query has its own bytes and
    epoch, so the rule that the epoch is taken before anything can fail is exercised here, not observed;
    SH_TRACE's run_closed line prints the form of the marks and the epoch of every call."""
    spec, pushes = CASES["grid_is_units"]()
    bad = pushes[0].cols[0].copy()
    bad[200_000] = 4_096
    g = rt.GpuQuery(spec)
    with pytest.raises(rt.SiddhiError, match=r"dictionary id outside \[0, key_capacity\)") as e:
        device_push(rt, g, abi.HostBatch(KS, pushes[0].ts, [bad, pushes[0].cols[1], pushes[0].cols[2]], 1))
    assert e.value.code == abi.SH_ERR_INVALID
    g.close()
    assert_same(gpu_device(rt, spec, pushes), want_of("grid_is_units"), label="after a failed push")


def test_two_partitions(rt):
    """Case 11: P = 2, 26 units per push: a grid that is no multiple of 8 keeps the order b, b + grid."""
    both_paths(rt, "two_partitions")


def test_workgroups_without_a_unit(rt):
    """Case 12: more units than the grid and a count that is no multiple of 8: two workgroups of the last
    XCD's run start past its end and must store nothing."""
    both_paths(rt, "no_unit")
