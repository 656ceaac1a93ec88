"""Group keys at the key table's edges on every GPU path: the key whose bits are the table's EMPTY mark
(reserved slot mask + 1), its neighbours, probe chains that start at the last slot and wrap to slot 0, and
the full table. Every case is GPU = oracle, bit-exact through tests.parity.assert_same; the streams and
their properties are pinned without a GPU in tests/test_key_edges_model.py, the cases live in
tests/key_edges.py. No reference KAT groups by such keys: parity is against the oracle, and a second check
renames every edge key to a small integer and demands the same GPU rows apart from the key columns."""
import numpy as np
import pytest

from oracle.oracle import OracleAggregation
from siddhi_amd import abi
from tests import key_edges as ke
from tests.parity import assert_same, run_pushes, split_batches
from tests.test_gpu_parity import both

pytestmark = pytest.mark.gpu

CASES = ke.query_cases()


@pytest.fixture(scope="module")
def rt():
    from siddhi_amd import runtime
    return runtime


def of_path(*paths):
    cs = [c for c in CASES if c.path in paths]
    return pytest.mark.parametrize("case", cs, ids=[c.id for c in cs])


def run_case(rt, case):
    out = both(rt, case.spec, case.pushes, label=case.id)
    assert out["ts"].size > 0
    return out


@of_path("batch")
def test_batch_windows(rt, case):
    """lengthBatch / timeBatch, output current / expired / all, every key set; the filtered variants take
    k_boundaries' scan-chain form."""
    run_case(rt, case)


@of_path("multisplit")
def test_lds_multisplit_two_partitions(rt, case):
    """600 keys, key_capacity 512: a 1024-slot table split into key partitions, the sentinel key the extra
    local key (NL = size / P + 1) of partition 0."""
    run_case(rt, case)


def test_lds_multisplit_early_counting_split(rt):
    """One push of 2^18 + 1 events: k_boundaries counts the push's tiles for the split queued right behind it.
    (The one case above 20k events: 0.15 s on an MI355X.)"""
    n = (1 << 18) + 1
    case = ke.multisplit_case(n + 4_000, (n,))
    assert len(case.pushes[0].ts) == n
    run_case(rt, case)


@of_path("stream.current", "batch having")
def test_stream_current(rt, case):
    """lengthBatch(L, true) / timeBatch(T, true): every window holds the sentinel key and the key in slot 0,
    whose packed sort keys were one run before the slot bits counted the reserved slot — with a `having` program
    too, which runs in the same sc_rows. All-events output sorts the keys whole, and `having` on a plain batch
    window (the two `batch having` cases) sorts in hv_closed, which always counted size + 1 slots: those are
    the controls. The oracle's selector has no `having`, so the reference of those cases is the selector model
    over the oracle's chunks (tests/having_model.py; tests/having_expired_model.py for all-events output)."""
    if case.spec.having is None:
        run_case(rt, case)
        return
    from tests import having_expired_model, having_model
    model = having_model if case.spec.output == "current" else having_expired_model
    want = model.run_model(case.spec, case.pushes)
    g = rt.GpuQuery(case.spec)
    got = run_pushes(g, case.pushes)
    g.close()
    assert_same(got, want, label=case.id)
    m = ke.sentinel_rows(got, case.ks)
    assert m.sum() > 10 and not m.all()


@of_path("sliding", "sliding churn")
def test_sliding_windows(rt, case):
    """time / externalTime with current and all-events output; a 2 s window keeps the sentinel key's ring alive
    across pushes. The churn case rebuilds the 128-slot table every few pushes (k_sl_rekey_map / k_slx_rekey_map
    keep slot `size`): the sentinel key survives while it is live and is dropped and re-created like any other."""
    run_case(rt, case)


@of_path("rate")
def test_output_rate_limiters(rt, case):
    """first / last / all every N events and `output first every <t> ms` with t = 0 and 500, keyed by the group
    key. The first_time limiter's own key -> time table grows between two sentinel-key rows less than t apart."""
    run_case(rt, case)


@of_path("partition", "partition group")
def test_partition_lanes(rt, case):
    """`partition with (p)`, p a long from LONGS: grouped by p, without group-by, and grouped by an (int, int)
    key from PAIRS_II — the (partition slot, group slot) table, whose group table hands out the reserved slot."""
    run_case(rt, case)


@of_path("wide")
def test_wide_keys(rt, case):
    """group by a, s, l and group by l, a: the long column has an interning level of its own, whose table has
    the same EMPTY mark."""
    out = run_case(rt, case)
    assert (out["keys"][case.l_row] == ke.SENTINEL).any()


@of_path("checkpoint")
def test_checkpoint_mid_window(case):
    """Snapshot after the second push (a window is open, the sentinel key live) and restore into a fresh query."""
    from tests.test_gpu_snapshot import checkpointed
    got, ref, _ = checkpointed(case.spec, case.pushes, 2)
    assert_same(got, ref, label=case.id)
    assert ke.sentinel_rows(ref, case.ks).sum() > 10


GPU_RENAME = [c for c in ke.rename_cases(CASES) if c.id in (
    "LONGS-timeBatch-all-send1", "LONGS-lengthBatch-current-send3", "PAIRS_II-timeBatch-current-send1",
    "LONGS-lengthBatch-current-plain", "LONGS-timeBatch-all-plain", "PAIRS_II-timeBatch-current-plain",
    "LONGS-time-all", "PAIRS_II-time-current", "LONGS-first_time-500", "LONGS+RATE40-first_time-500", "LONGS-first-3")]
assert len(GPU_RENAME) == 11


@pytest.mark.parametrize("case", GPU_RENAME, ids=[c.id for c in GPU_RENAME])
def test_gpu_same_rows_under_key_renaming(rt, case):
    """GPU against GPU: every edge key renamed to a small integer (ordinary home slots, no reserved slot) gives
    the same rows apart from the key columns. Holds where row order does not depend on the key's value: batch
    windows and stream.current order a chunk's rows by first arrival, sliding windows emit a row per event,
    the limiters pick rows by position and per-key state. (Not the partition lanes: due partitions fire in
    java.util.HashMap order of the key's text.)"""
    def run(spec, pushes):
        g = rt.GpuQuery(spec)
        out = run_pushes(g, pushes)
        g.close()
        return out

    a, b = ke.renamed_runs(case, run)
    ke.assert_same_but_keys(a, b, case.ks, ke.renamed(case.ks), case.id)


# ---- incremental aggregation ---------------------------------------------------------------------
@pytest.mark.parametrize("event_time", [True, False])
def test_incremental_aggregation(rt, event_time):
    """sec...min grouped by a long from LONGS: tables and one `within ... per` retrieval. With `aggregate by ts`
    the root keys by (bucket, group), so the long is interned first (sh_aggregation.cpp: `intern` for a long
    beside a bucket) and the interning table meets the sentinel — the control; in processing time the root's
    own table takes the long directly."""
    from tests.test_gpu_aggregation import both as agg_both
    ks = ke.longs()
    n = 12_000
    idx = ke.key_indices(ks.n, n, 53, [1, 5_000])
    rng = np.random.default_rng(54)
    clock = 1_706_745_000_000 + np.cumsum(rng.integers(0, 40, n)).astype(np.int64)
    v = rng.integers(-500, 500, n).astype(np.float64) / 8.0
    sch = abi.Schema.parse("k long, v double, ts long")
    spec = abi.AggregationSpec(sch, [("sum", "v"), ("count", None), ("min", "v"), ("max", "v")], group_by=["k"],
                               ts="ts" if event_time else None, durations=("sec", "min"), key_capacity=128)
    pushes = split_batches(sch, clock, [ks.cols[0][idx], v, clock.copy()], [1, 5_000], 25)
    rows = agg_both(rt, spec, pushes + [("advance", int(clock[-1]) + 200_000)], "agg LONGS", checkpoints=(1,))
    assert rows > ks.n
    g, o = rt.GpuAggregation(spec), OracleAggregation(spec)
    for q in (g, o):
        for p in pushes:
            q.push(p)
    span = (abi.DUR_NAMES["sec"], int(clock[0]) - 60_000, int(clock[-1]) + 60_000)
    gf, of = g.find(*span), o.find(*span)
    g.close()
    o.close()
    assert gf == of and len(gf) > ks.n


# ---- sharded owner -------------------------------------------------------------------------------
def test_sharded_owner_routing(rt):
    """Two shards in one process (LocalShards): both sides route the sentinel key to the same owner, whose
    table gives it the reserved slot; the merged output equals the single-stream oracle's."""
    from tests.test_gpu_shard import run_oracle, run_sharded, spec as shard_spec
    ks = ke.longs()
    sch = abi.Schema.parse("k long, v double, ts long")
    n = 16_000
    ts, cols, _ = ke.stream(ks, n, 59, [6_000])
    cols = [cols[0], cols[1], ts.copy()]
    sp = shard_spec(128, schema=sch)
    pushes = [(ts[:6_000], [c[:6_000] for c in cols]), (ts[6_000:], [c[6_000:] for c in cols])]
    adv = int(ts[-1]) + 5_000
    got = run_sharded(sp, 2, pushes, 1, [[0.5], [0.3]], advance=adv)
    ref = run_oracle(sp, pushes, 1, advance=adv)
    assert (ref["keys"][0] == ke.SENTINEL).sum() > 5
    assert_same(got, ref, label="sharded LONGS x2")


# ---- the full table ------------------------------------------------------------------------------
def _full_table_stream(keys, n=4_000, seed=61):
    rng = np.random.default_rng(seed)
    k = np.array(keys, dtype=np.int64)[np.concatenate([np.arange(len(keys)), rng.integers(0, len(keys), n - len(keys))])]
    ts = (np.cumsum(rng.integers(0, 3, n)) + 10_000).astype(np.int64)
    v = rng.integers(-500, 500, n).astype(np.float64) / 8.0
    return ts, [k, v, ts.copy()]


@pytest.mark.parametrize("window,param", [("timeBatch", 500), ("time", 300)])
def test_full_table(rt, window, param):
    """key_capacity 8 is a 16-slot table. One push brings 16 distinct keys, 8 of them with home slot 15, and the
    sentinel key: every slot is used (the last insert probes the whole table) and the sentinel takes slot 16;
    the output equals the oracle's. One more key in that push fails loudly — `group key table full: raise
    key_capacity` (KeyTableHost::check_result) — instead of mixing two keys. (Between pushes the table is rebuilt
    larger, so only a first push can fill it.)"""
    keys, one_more = ke.full_table_keys()
    sch = abi.Schema.parse("k long, v double, ts long")
    spec = abi.QuerySpec(sch, window, param, group_by=["k"], aggs=[("count", None), ("sum", "v"), ("min", "v")],
                         key_capacity=8)
    ts, cols = _full_table_stream(keys)
    assert len(np.unique(cols[0][:3_000])) == 17
    pushes = split_batches(sch, ts, cols, [3_000], 1) + [("advance", int(ts[-1]) + 2_000)]
    out = both(rt, spec, pushes, label=f"full table {window}")
    assert len(np.unique(out["keys"][0])) == 17
    ts, cols = _full_table_stream(keys + [one_more])
    g = rt.GpuQuery(spec)
    with pytest.raises(rt.SiddhiError, match="key table full"):
        g.push(abi.HostBatch(sch, ts[:3_000], [c[:3_000] for c in cols], 1))
    g.close()
