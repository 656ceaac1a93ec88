"""What tests/test_gpu_key_edges.py depends on, checked without a GPU: the key generators still collide, the
streams still carry the sentinel key where the cases need it, and the oracle itself treats the key with the
EMPTY mark's bits like any other key (a key-renamed copy of the stream gives the same rows)."""
import numpy as np
import pytest

from oracle.oracle import OracleQuery
from siddhi_amd import abi, synth
from tests import key_edges as ke
from tests.parity import run_pushes

CASES = ke.query_cases()


def oracle(spec, pushes):
    o = OracleQuery(spec)
    out = run_pushes(o, pushes)
    o.close()
    return out


# ---- the generators ------------------------------------------------------------------------------
def test_sentinel_forms_share_the_empty_marks_bits():
    assert ke.SENTINEL == -2 ** 63 + 1 and ke.SENTINEL & ke.M64 == ke.SENTINEL_BITS
    for make in ke.KEYSETS.values():
        ks = make()
        assert ks.packed[0] == ke.SENTINEL_BITS, ks.name
        assert ks.packed.count(ke.SENTINEL_BITS) == 1, ks.name
    assert ke.SENTINEL_DOUBLE == -4.9e-324 and ke.SENTINEL_DOUBLE.view(np.uint64) == ke.SENTINEL_BITS
    f, b = ke.SENTINEL_PAIR_FI
    assert f == 0 and np.signbit(f) and (int(f.view(np.uint32)) << 32 | b) == ke.SENTINEL_BITS
    a, b = ke.SENTINEL_PAIR_II
    assert ((a & 0xFFFFFFFF) << 32 | b) == ke.SENTINEL_BITS
    assert ke.longs().n == 67 and ke.pairs_ii().n == 16 and ke.pairs_fi().distinct() == 16 and ke.doubles().distinct() == 8


def test_home_colliding_keys_start_at_the_last_slot_of_every_table():
    keys = [int(k) for k in ke.home_colliding_keys(150)]
    assert len(set(keys)) == 150 and ke.SENTINEL not in keys
    for lg in range(4, 33):
        assert all(ke.key_home(k, lg) == 2 ** lg - 1 for k in keys), lg
    # ordinary small keys do not: the generator, not the hash, makes the chain
    assert len({ke.key_home(k, 7) for k in range(60)}) == 60
    # key 0's home is slot 0 of every table: the slot the sentinel key's packed run merged into
    assert all(ke.key_home(0, lg) == 0 for lg in range(4, 33))


def test_rate_colliding_keys_start_at_the_last_slot_of_every_limiter_table():
    keys = [int(k) for k in ke.rate_colliding_keys(40)]
    assert len(set(keys)) == 40 and ke.SENTINEL not in keys
    assert not set(keys) & {int(k) for k in ke.longs().cols[0]}
    for lg in range(6, 33):
        assert all(ke.mix64(k) & (2 ** lg - 1) == 2 ** lg - 1 for k in keys), lg


def test_mix64_restatement_and_round_trip():
    z = np.array([0, 1, ke.SENTINEL_BITS, ke.M64, 0x0123456789ABCDEF], dtype=np.uint64)
    assert [ke.mix64(int(v)) for v in z] == [int(v) for v in synth.mix64(z)]
    rng = np.random.default_rng(1)
    for v in [int(x) for x in rng.integers(0, 2 ** 63, 200)] + [0, ke.M64, ke.SENTINEL_BITS]:
        assert ke.unmix64(ke.mix64(v)) == v and ke.mix64(ke.unmix64(v)) == v


def test_full_table_keys():
    keys, one_more = ke.full_table_keys()
    assert keys[0] == ke.SENTINEL and len(set(keys)) == 17 and one_more not in keys
    assert sum(ke.key_home(k, 4) == 15 for k in keys[1:]) == 8 and ke.key_home(one_more, 4) == 15


# ---- the streams ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_streams_keep_the_sentinel_key_at_the_edges(case):
    """Every push starts and ends with a sentinel-key event; the oracle's output has sentinel-key rows in every
    push that gives rows, in more than one flush, and — where rows follow the events — as the first and last
    row of each push; the stream holds the intended number of distinct keys."""
    ks = case.ks
    sent = [c[0] for c in ks.cols]
    kcols = [case.spec.schema.col(g) for g in (["l"] if case.path == "wide" else ks.group_by)]

    def is_sent(batch):
        m = np.ones(len(batch.ts), dtype=bool)
        for c, s in zip(kcols, sent):
            col = batch.cols[c]
            m &= (col.view(np.uint32) == s.view(np.uint32)) if col.dtype == np.float32 else \
                 (col.view(np.uint64) == s.view(np.uint64)) if col.dtype == np.float64 else (col == s)
        return m

    batches = [p for p in case.pushes if not isinstance(p, tuple)]
    if case.path != "sliding churn":
        for b in batches:
            m = is_sent(b)
            assert m[0] and m[-1], "a push does not start and end with the sentinel key"
    if case.n_keys > 0:
        with np.errstate(invalid="ignore"):  # (a NaN payload widened to double)
            allk = np.concatenate([np.stack([b.cols[c].astype(np.float64).view(np.int64) if b.cols[c].dtype == np.float32
                                             else b.cols[c].view(np.int64) if b.cols[c].dtype == np.float64
                                             else b.cols[c].astype(np.int64) for c in kcols]) for b in batches], axis=1)
        probe = ke.KeySet("probe", ks.key_schema, ks.group_by, ks.cols)
        distinct = len({tuple(ke._canon(allk[:, i], probe)) for i in range(allk.shape[1])})
        assert distinct == case.n_keys
    o = OracleQuery(case.spec)
    flushes_with = 0
    for p in case.pushes:
        out = abi.out_arrays(o.advance_time_raw(p[1]) if isinstance(p, tuple) else o.push_raw(p))
        if case.path == "wide":
            m = out["keys"][case.l_row] == ke.SENTINEL
        elif not case.spec.group_by:  # (no key columns in the rows: the input checks above stand alone)
            m = np.ones(len(out["ts"]), dtype=bool)
        else:
            m = ke.sentinel_rows(out, ks)
        if isinstance(p, tuple) or case.path == "sliding churn":
            continue
        if len(out["ts"]) > 0 and len(p.ts) > 1:
            assert m.any(), "a push without sentinel-key rows"
        if case.per_event_rows and len(out["ts"]):
            assert m[0] and m[-1]
        fo = out["flush_offsets"]
        flushes_with += sum(bool(m[a:b].any()) for a, b in zip(fo[:-1], fo[1:]))
        if case.path in ("batch", "multisplit") and len(p.ts) > 1_000:
            # batch windows: the push's first and last window both hold the key
            assert m[fo[0]:fo[1]].any() and m[fo[-2]:fo[-1]].any()
    o.close()
    if case.path != "sliding churn":
        assert flushes_with > 1


def test_stream_current_windows_hold_the_sentinel_key_and_the_slot_0_key():
    """The packed sort key merged the sentinel key's run with slot 0's: a window must hold both. Key 0 has home
    slot 0 at every table size (LONGS holds 0, PAIRS_II the pair (0, 0)), and LONGS' home-colliding keys wrap
    from the last slot into slot 0 as well."""
    for name in ("LONGS", "PAIRS_II"):
        ks = ke.KEYSETS[name]()
        zero = ks.packed.index(0)
        _, _, idx = ke.stream(ks, 10_000, 19, ke.CUTS)
        for L in (100,):
            w = np.arange(len(idx)) // L
            both = [np.any(idx[w == i] == 0) and np.any(idx[w == i] == zero) for i in range(w.max() + 1)]
            assert sum(both) > len(both) // 2, name


def test_churn_case_drops_and_recreates_the_sentinel_key():
    c = ke.churn_case()
    k = np.concatenate([p.cols[0] for p in c.pushes])
    ts = np.concatenate([p.ts for p in c.pushes])
    s = ts[k == ke.SENTINEL]
    gaps = np.diff(s)
    assert (gaps > 1_000).sum() == 1 and gaps.max() > 50 * 20  # one silence far longer than the 50 ms window
    out = oracle(c.spec, c.pushes)
    m = ke.sentinel_rows(out, c.ks)
    cnt = out["vals"][1][m]
    assert m.sum() == len(s) and cnt.max() == 3 and cnt[np.searchsorted(s, s[np.argmax(gaps) + 1])] == 1


# ---- the oracle on the sentinel key --------------------------------------------------------------
def test_oracle_hand_trace_sentinel_key():
    """lengthBatch(4) over 8 events, keys S S A S | A S S B: rows per batch in first-arrival order."""
    sch = abi.Schema.parse("k long, v double, ts long")
    S, A, B = ke.SENTINEL, 0, ke.SENTINEL + 1
    spec = abi.QuerySpec(sch, "lengthBatch", 4, group_by=["k"], aggs=[("count", None), ("sum", "v")], key_capacity=16)

    def run(s, a, b):
        rows = [(100 + i, k, v, 100 + i) for i, (k, v) in enumerate(
            [(s, 1.0), (s, 2.0), (a, 4.0), (s, 8.0), (a, 16.0), (s, 32.0), (s, 64.0), (b, 128.0)])]
        return oracle(spec, [abi.HostBatch.from_rows(sch, rows, 1)])

    out = run(S, A, B)
    assert out["flush_offsets"].tolist() == [0, 2, 5]
    assert out["keys"][0].tolist() == [S, A, A, S, B]
    assert out["vals"][0].tolist() == [3, 1, 1, 2, 1]
    assert out["vals"][1].view(np.float64).tolist() == [11.0, 4.0, 16.0, 96.0, 128.0]
    ren = run(1000, 1001, 1002)
    assert ren["keys"][0].tolist() == [1000, 1001, 1001, 1000, 1002]
    for f in ("flush_offsets", "flush_clock", "ts", "rep", "expired", "nulls"):
        assert np.array_equal(out[f], ren[f])
    assert all(np.array_equal(x, y) for x, y in zip(out["vals"], ren["vals"]))


RENAME = ke.rename_cases(CASES)


@pytest.mark.parametrize("case", RENAME, ids=[c.id for c in RENAME])
def test_oracle_same_rows_under_key_renaming(case):
    """Batch windows, stream.current, sliding windows and the rate limiters order rows by arrival (QuerySelector's
    LinkedHashMap, the limiters' per-key maps are looked up, never walked): renaming every edge key to a small
    integer changes the key columns alone."""
    a, b = ke.renamed_runs(case, oracle)
    ke.assert_same_but_keys(a, b, case.ks, ke.renamed(case.ks), case.id)
