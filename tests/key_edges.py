"""Group keys at the edges of the device key table (sh_device.h key_home / probe_step / key_slot /
key_slots): helpers for tests/test_key_edges_model.py (CPU) and tests/test_gpu_key_edges.py. No tests here.

The table's EMPTY mark is the bit pattern 0x8000000000000001. A real key with those bits — the long
Long.MIN_VALUE + 1, the int pair (Integer.MIN_VALUE, 1), the (float, int) pair (-0.0f, 1), the double
-4.9E-324 — takes the reserved slot mask + 1 behind the table. `home_colliding_keys` all have the table's
last slot as their home at every table size (the chain wraps to slot 0 at once); `rate_colliding_keys`
do the same to the `output first every <t>` limiter's own table, which hashes with mix64."""
from dataclasses import dataclass, field
from typing import List

import numpy as np

from siddhi_amd import abi

M64 = (1 << 64) - 1
PHI = 0x9E3779B97F4A7C15          # key_home's multiplier
SENTINEL_BITS = 0x8000000000000001  # kEmptyKey
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
LONG_MIN, LONG_MAX = -2 ** 63, 2 ** 63 - 1


def as_i64(u: int) -> int:
    u &= M64
    return u - (1 << 64) if u >> 63 else u


SENTINEL = as_i64(SENTINEL_BITS)  # Long.MIN_VALUE + 1
SENTINEL_PAIR_II = (INT_MIN, 1)
SENTINEL_PAIR_FI = (np.float32(-0.0), 1)


def f64_of_bits(b: int) -> np.float64:
    return np.array([b & M64], dtype=np.uint64).view(np.float64)[0]


def f32_of_bits(b: int) -> np.float32:
    return np.array([b & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0]


SENTINEL_DOUBLE = f64_of_bits(SENTINEL_BITS)  # -4.9E-324
NAN_PAYLOAD_F64 = f64_of_bits(0x7FF0000000000123)
NAN_PAYLOAD_F32 = f32_of_bits(0x7F800123)


# ---- the two hashes, restated -------------------------------------------------------------------
def key_home(key: int, lg: int) -> int:
    """sh_device.h key_home for a table of 2^lg slots: the top lg bits of key * PHI."""
    return (((key & M64) * PHI) & M64) >> (64 - lg)


def mix64(z: int) -> int:
    """sh_device.h mix64 (= siddhi_amd.synth.mix64) on one Python int."""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def unmix64(z: int) -> int:
    z &= M64
    z = z ^ (z >> 31) ^ (z >> 62)
    z = (z * pow(0x94D049BB133111EB, -1, 1 << 64)) & M64
    z = z ^ (z >> 27) ^ (z >> 54)
    z = (z * pow(0xBF58476D1CE4E5B9, -1, 1 << 64)) & M64
    return z ^ (z >> 30) ^ (z >> 60)


def home_colliding_keys(n: int) -> np.ndarray:
    """n distinct keys whose product with PHI has its top 32 bits set: key_home == mask for 2^4..2^32 slots."""
    inv = pow(PHI, -1, 1 << 64)
    return np.array([as_i64(((0xFFFFFFFF << 32 | j) * inv) & M64) for j in range(n)], dtype=np.int64)


def rate_colliding_keys(n: int) -> np.ndarray:
    """n distinct keys with mix64(key) & tmask == tmask for every limiter table of up to 2^32 slots."""
    return np.array([as_i64(unmix64((j << 32) | 0xFFFFFFFF)) for j in range(n)], dtype=np.int64)


# ---- key sets -----------------------------------------------------------------------------------
TAIL = "v double, x long, ts long"
AGGS = [("count", None), ("sum", "v"), ("min", "v"), ("max", "x"), ("avg", "x")]


@dataclass
class KeySet:
    """Distinct group keys, key 0 the sentinel: `cols` holds one array per group-by column, `packed` the 64
    bits the table sees for each key (make_key: one 8-byte column, or two 32-bit halves, NaN canonical)."""
    name: str
    key_schema: str
    group_by: List[str]
    cols: List[np.ndarray]
    packed: List[int] = field(default_factory=list)

    @property
    def n(self):
        return len(self.cols[0])

    @property
    def schema(self):
        return abi.Schema.parse(f"{self.key_schema}, {TAIL}")

    def distinct(self):
        """keys the engine tells apart (every NaN payload is the one key "NaN")"""
        return len(set(self.packed))

    def out_keys(self):
        """[column][key] as sh_out reports them: integers widened, floats as the bits of the double"""
        rows = []
        for c in self.cols:
            if c.dtype == np.float32:
                with np.errstate(invalid="ignore"):  # (a NaN payload widened to double)
                    rows.append(c.astype(np.float64).view(np.int64))
            elif c.dtype == np.float64:
                rows.append(c.view(np.int64))
            else:
                rows.append(c.astype(np.int64))
        return np.stack(rows)


def _bits32(x) -> int:
    if isinstance(x, (np.float32, float)):
        f = np.float32(x)
        return 0x7FC00000 if np.isnan(f) else int(np.array([f]).view(np.uint32)[0])
    return int(x) & 0xFFFFFFFF


def longs(colliders=60, extra=()) -> KeySet:
    # (SENTINEL - 1 is Long.MIN_VALUE; 1 is there for key 0's other neighbour: 7 keys and the colliders)
    k = [SENTINEL, SENTINEL + 1, LONG_MIN, LONG_MAX, 0, -1, 1]
    k += [int(x) for x in home_colliding_keys(colliders)] + [int(x) for x in extra]
    assert len(set(k)) == len(k)
    return KeySet("LONGS", "k long", ["k"], [np.array(k, dtype=np.int64)], [x & M64 for x in k])


INTS = [1, 0, -1, 2]


def pairs_ii() -> KeySet:
    ab = [(a, b) for a in (INT_MIN, 0, -1, INT_MAX) for b in INTS]
    ab.remove(SENTINEL_PAIR_II)
    ab.insert(0, SENTINEL_PAIR_II)
    return KeySet("PAIRS_II", "a int, b int", ["a", "b"],
                  [np.array([p[0] for p in ab], dtype=np.int32), np.array([p[1] for p in ab], dtype=np.int32)],
                  [(_bits32(a) << 32) | _bits32(b) for a, b in ab])


def pairs_fi() -> KeySet:
    fs = [np.float32(-0.0), np.float32(0.0), np.float32(1.5), np.float32(np.nan), NAN_PAYLOAD_F32]
    fb = [(f, b) for f in fs for b in INTS]
    return KeySet("PAIRS_FI", "f float, b int", ["f", "b"],
                  [np.array([p[0] for p in fb], dtype=np.float32), np.array([p[1] for p in fb], dtype=np.int32)],
                  [(_bits32(f) << 32) | _bits32(b) for f, b in fb])


def doubles() -> KeySet:
    bits = [SENTINEL_BITS, SENTINEL_BITS + 1, 0x8000000000000000, 0x0, 0x1, 0x3FF8000000000000,
            0x7FF8000000000000, 0x7FF0000000000123, 0xFFF8000000000001, 0x7FEFFFFFFFFFFFFF]
    d = np.array(bits, dtype=np.uint64).view(np.float64)
    return KeySet("DOUBLES", "d double", ["d"], [d.copy()],
                  [0x7FF8000000000000 if np.isnan(x) else b for x, b in zip(d, bits)])


def wide_longs(n_keys=600, colliders=150, seed=77) -> KeySet:
    """the sentinel, `colliders` home-colliding keys and random 64-bit keys: n_keys in all"""
    rng = np.random.default_rng(seed)
    k = [SENTINEL] + [int(x) for x in home_colliding_keys(colliders)]
    k += [int(x) for x in rng.integers(LONG_MIN, LONG_MAX, n_keys - len(k), dtype=np.int64)]
    assert len(set(k)) == n_keys
    return KeySet("LONGS600", "k long", ["k"], [np.array(k, dtype=np.int64)], [x & M64 for x in k])


KEYSETS = {"LONGS": longs, "PAIRS_II": pairs_ii, "PAIRS_FI": pairs_fi, "DOUBLES": doubles}


def renamed(ks: KeySet) -> KeySet:
    """The same number of keys as small distinct integers (key i -> 1000 + i, or the pair (100 + i, 7)): for
    key sets without NaNs, whose keys are all distinct to the engine."""
    assert ks.distinct() == ks.n
    if len(ks.cols) == 1:
        k = np.arange(ks.n, dtype=np.int64) + 1000
        return KeySet(ks.name + "_renamed", "k long", ["k"], [k], [int(x) for x in k])
    a = np.arange(ks.n, dtype=np.int32) + 100
    b = np.full(ks.n, 7, dtype=np.int32)
    return KeySet(ks.name + "_renamed", "a int, b int", ["a", "b"], [a, b], [(int(x) << 32) | 7 for x in a])


# ---- streams ------------------------------------------------------------------------------------
def key_indices(n_keys, n, seed, cuts=(), share=0.08):
    """Which key each event carries: the sentinel (key 0) for `share` of the events and for the first and
    last event of every push; the other keys uniformly."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_keys, n)
    idx[rng.random(n) < share] = 0
    for c in [0, n] + list(cuts):
        if c > 0:
            idx[c - 1] = 0
        if c < n:
            idx[c] = 0
    return idx


def stream(ks: KeySet, n, seed, cuts=(), step=3, share=0.08, idx=None):
    """(ts, cols, idx): timestamps advance 0..step-1 ms per event; v = k/8 doubles (sums are exact)."""
    rng = np.random.default_rng(seed + 1000)
    ts = (np.cumsum(rng.integers(0, step, n)) + 10_000).astype(np.int64)
    if idx is None:
        idx = key_indices(ks.n, n, seed, cuts, share)
    v = rng.integers(-500, 500, n).astype(np.float64) / 8.0
    x = rng.integers(-50, 50, n).astype(np.int64)
    return ts, [c[idx] for c in ks.cols] + [v, x, ts.copy()], idx


def key_index_of_rows(out, ks: KeySet):
    """the key index of every output row (NaN keys: the first key with the same packed bits)"""
    ok = ks.out_keys()
    # canonical NaN per float column, as the engine reports one NaN
    table = {}
    for i in range(ks.n - 1, -1, -1):
        table[tuple(_canon(ok[:, i], ks))] = i
    rows = out["keys"]
    return np.array([table[tuple(_canon(rows[:, r], ks))] for r in range(rows.shape[1])], dtype=np.int64)


def _canon(col, ks):
    out = []
    for c, v in zip(ks.cols, col):
        v = int(v)
        if c.dtype in (np.float32, np.float64) and np.isnan(np.array([v], dtype=np.int64).view(np.float64)[0]):
            v = 0x7FF8000000000000
        out.append(v)
    return out


def assert_same_but_keys(a, b, ks_a: KeySet, ks_b: KeySet, label=""):
    """Two runs over streams that differ in the key columns only: everything but the key columns is equal,
    and every row carries the same key index."""
    for f in ("flush_offsets", "flush_clock", "ts", "nulls", "expired", "rep", "val_types"):
        assert np.array_equal(a[f], b[f]), f"{label}: {f} differ"
    for i in range(len(a["val_types"])):
        assert np.array_equal(a["vals"][i], b["vals"][i]), f"{label}: agg {i} differs"
    assert np.array_equal(key_index_of_rows(a, ks_a), key_index_of_rows(b, ks_b)), f"{label}: rows' keys differ"


def sentinel_rows(out, ks: KeySet):
    ok = ks.out_keys()[:, 0]
    m = np.ones(out["keys"].shape[1], dtype=bool)
    for c in range(len(ok)):
        m &= out["keys"][c] == ok[c]
    return m


# ---- the cases: one list, run by the oracle alone (test_key_edges_model.py) and by GPU and oracle ----
@dataclass
class Case:
    id: str
    path: str          # which GPU path the case is for
    spec: object
    pushes: list
    ks: KeySet
    n_keys: int        # distinct keys intended in the stream
    per_event_rows: bool = False  # every event gives a row in stream order (first / last row of a push: the sentinel's)


def _pushes(ks, ts, cols, cuts, send, advance=5_000):
    from tests.parity import split_batches
    p = split_batches(ks.schema, ts, cols, cuts, send)
    if advance:
        p.append(("advance", int(ts[-1]) + advance))
    return p


CUTS = [1, 7_777]


def batch_cases():
    out = []
    for name, make in KEYSETS.items():
        ks = make()
        for window, param in (("lengthBatch", 777), ("timeBatch", 500)):
            sends = (1, 3) if name == "LONGS" else ((3,) if window == "lengthBatch" else (1,))
            for send in sends:
                ts, cols, _ = stream(ks, 12_000, 11, CUTS)
                for output in ("current", "expired", "all"):
                    spec = abi.QuerySpec(ks.schema, window, param, group_by=ks.group_by, aggs=AGGS, output=output,
                                         key_capacity=128)
                    out.append(Case(f"{name}-{window}-{output}-send{send}", "batch", spec,
                                    _pushes(ks, ts, cols, CUTS, send), ks, ks.distinct()))
    ks = longs()
    ts, cols, _ = stream(ks, 12_000, 13, CUTS)
    for window, param in (("lengthBatch", 777), ("timeBatch", 500)):
        spec = abi.QuerySpec(ks.schema, window, param, group_by=ks.group_by, aggs=AGGS, filter=(">", "v", -40.0),
                             key_capacity=128)
        out.append(Case(f"LONGS-{window}-filtered", "batch", spec, _pushes(ks, ts, cols, CUTS, 3), ks, ks.n))
        # `having` on a plain batch window: hv_closed's own sort over (window, slot), sized for size + 1 slots
        spec = abi.QuerySpec(ks.schema, window, param, group_by=ks.group_by, aggs=AGGS, key_capacity=128,
                             having=("and", ("<=", ("agg", 0), 3), (">", ("agg", 1), -100.0)))
        out.append(Case(f"LONGS-{window}-having", "batch having", spec, _pushes(ks, ts, cols, CUTS, 3), ks, ks.n))
    return out


SC_HAVING = ("or", (">=", ("agg", 0), 2), (">", ("agg", 1), -20.0))
MS_AGGS = [("count", None), ("min", "v"), ("max", "v"), ("avg", "v")]


def multisplit_case(n=20_000, cuts=(1, 7_777)):
    """600 keys in a 1024-slot table: two key partitions, the sentinel local key 512 of partition 0"""
    ks = wide_longs()
    ts, cols, _ = stream(ks, n, 17, cuts, share=0.02)
    spec = abi.QuerySpec(ks.schema, "timeBatch", 500, group_by=ks.group_by, aggs=MS_AGGS, key_capacity=512)
    return Case(f"LONGS600-timeBatch-{n}", "multisplit", spec, _pushes(ks, ts, cols, list(cuts), 1), ks, ks.n)


def stream_current_cases():
    out = []
    for name in ("LONGS", "PAIRS_II"):
        ks = KEYSETS[name]()
        for window, param, send in (("lengthBatch", 100, 3), ("timeBatch", 300, 1)):
            ts, cols, _ = stream(ks, 10_000, 19, CUTS)
            for output in ("current", "all"):
                for hv in (False, True):
                    spec = abi.QuerySpec(ks.schema, window, param, group_by=ks.group_by, aggs=AGGS, output=output,
                                         stream_current=True, key_capacity=128, having=SC_HAVING if hv else None)
                    out.append(Case(f"{name}-{window}-{output}-{'having' if hv else 'plain'}", "stream.current", spec,
                                    _pushes(ks, ts, cols, CUTS, send), ks, ks.n, per_event_rows=not hv and output == "current"))
    return out


def sliding_cases():
    out = []
    for name, window, n in (("LONGS", "time", 12_000), ("LONGS", "externalTime", 12_000), ("PAIRS_II", "time", 8_000)):
        ks = KEYSETS[name]()
        ts, cols, _ = stream(ks, n, 23, [1, 5_555])
        for output in ("current", "all"):
            # 2 s: the sentinel key's ring lives across the pushes (a push spans ~5 s)
            spec = abi.QuerySpec(ks.schema, window, 2_000, group_by=ks.group_by, aggs=AGGS, output=output,
                                 key_capacity=128, ts_attr="ts" if window == "externalTime" else None)
            out.append(Case(f"{name}-{window}-{output}", "sliding", spec, _pushes(ks, ts, cols, [1, 5_555], 1), ks,
                            ks.n, per_event_rows=output == "current"))
    return out


def churn_case():
    """test_sliding_key_churn_bound's shape — a new key every 4 events, a 128-slot table rebuilt every few
    pushes of 100 events — with a sentinel-key event every 21 ms (three live in the 50 ms window) until event 3000, none until 4500 (the key's
    window drains: it is dropped by a rebuild) and again from there (re-created)."""
    ks = KeySet("CHURN", "k long", ["k"], [np.array([SENTINEL], dtype=np.int64)], [SENTINEL_BITS])
    n = 6_000
    ts = np.arange(n, dtype=np.int64) * 3 + 1_000
    k = (np.arange(n, dtype=np.int64) // 4) * 1_000_003 + 5
    sent = (np.arange(n) % 7 == 0) & ((np.arange(n) < 3_000) | (np.arange(n) >= 4_500))
    k[sent] = SENTINEL
    v = (np.arange(n) % 97).astype(np.float64) / 8
    x = (np.arange(n) % 13).astype(np.int64)
    spec = abi.QuerySpec(ks.schema, "time", 50, group_by=["k"], aggs=[("sum", "v"), ("count", None), ("max", "v")],
                         key_capacity=64)
    from tests.parity import split_batches
    pushes = split_batches(ks.schema, ts, [k, v, x, ts.copy()], list(range(100, n, 100)), 1)
    return Case("CHURN-time", "sliding churn", spec, pushes, ks, len(np.unique(k)))


RATES = [("first", 3), ("last", 4), ("all", 7), ("first_time", 0), ("first_time", 500)]


def rate_cases():
    """lengthBatch(97) flushes every ~100 ms and nearly every flush has a sentinel-key row, so consecutive
    sentinel rows lie less than t = 500 ms apart; push 1 is one sentinel event (a 64-slot limiter table),
    push 2 brings every other key (more than 32, then more than 64 with the mix64-colliding keys: the table
    is rebuilt) and its first rows follow the sentinel key's last output by less than t."""
    out = []
    sets = [("LONGS", longs()), ("PAIRS_II", pairs_ii()),
            ("LONGS+RATE40", longs(extra=rate_colliding_keys(40)))]
    # ((float, int) keys: the limiters pack the rows' reported keys again, a float reported widened to double)
    sets.append(("PAIRS_FI", pairs_fi()))
    for name, ks in sets:
        ts, cols, _ = stream(ks, 12_000, 29, [1, 500, 6_000])
        for kind, n in (RATES if name != "PAIRS_FI" else [("first", 3), ("last", 4), ("first_time", 500)]):
            spec = abi.QuerySpec(ks.schema, "lengthBatch", 97, group_by=ks.group_by, aggs=AGGS, key_capacity=128,
                                 rate=(kind, n))
            out.append(Case(f"{name}-{kind}-{n}", "rate", spec, _pushes(ks, ts, cols, [1, 500, 6_000], 3, 0), ks, ks.distinct()))
    return out


def partition_cases():
    out = []
    lk = longs()
    pk = pairs_ii()
    n = 12_000
    idx_p = key_indices(lk.n, n, 31, CUTS)
    idx_g = key_indices(pk.n, n, 37, CUTS)
    # partition key alone (schema p long, ...), grouped by it or not
    ksp = KeySet("LONGS", "p long", ["p"], lk.cols, lk.packed)
    ts, cols, _ = stream(ksp, n, 31, CUTS, idx=idx_p)
    for window, param, send, group in (("time", 150, 1, True), ("lengthBatch", 3, 5, False), ("lengthBatch", 100, 5, True)):
        for output in ("current", "all"):
            spec = abi.QuerySpec(ksp.schema, window, param, group_by=["p"] if group else [], aggs=AGGS, partition="p",
                                 output=output, key_capacity=256)
            adv = 5_000 if window == "time" else 0
            out.append(Case(f"p-LONGS-{window}{param}-{'grouped' if group else 'nogroup'}-{output}", "partition", spec,
                            _pushes(ksp, ts, cols, CUTS, send, adv), ksp, lk.n))
    # a long partition key and an (int, int) group key other than it: the (partition, group) table
    ksg = KeySet("LONGSxPAIRS_II", "p long, a int, b int", ["a", "b"], pk.cols, pk.packed)
    tsg, colsg, _ = stream(ksg, n, 31, CUTS, idx=idx_g)
    few = np.array([0, 1, 4, 7, 8, 9])  # six partitions: the sentinel, its neighbour, 0 and three home-colliding keys
    colsg = [lk.cols[0][few[idx_p % few.size]]] + colsg
    for window, param, send in (("time", 150, 1), ("lengthBatch", 37, 3)):
        for output in ("current", "all"):
            spec = abi.QuerySpec(ksg.schema, window, param, group_by=["a", "b"], aggs=AGGS, partition="p",
                                 output=output, key_capacity=1024)
            adv = 5_000 if window == "time" else 0
            out.append(Case(f"p-LONGS-g-PAIRS_II-{window}-{output}", "partition group", spec,
                            _pushes(ksg, tsg, colsg, CUTS, send, adv), ksg, pk.n))
    return out


WIDE_SCH = "a int, s string, l long"


def wide_cases():
    out = []
    lk = longs()
    n = 10_000
    idx = key_indices(lk.n, n, 41, CUTS)
    rng = np.random.default_rng(43)
    a = rng.integers(-1, 2, n).astype(np.int32)
    s = rng.integers(0, 3, n).astype(np.int32)
    a[idx == 0] = 1   # (the sentinel long beside one (a, s) pair and others beside it)
    ks = KeySet("WIDE", WIDE_SCH, ["l"], lk.cols, lk.packed)
    ts, cols, _ = stream(ks, n, 41, CUTS, idx=idx)
    cols = [a, s] + cols
    for group in (["a", "s", "l"], ["l", "a"]):
        for window, param, output in (("timeBatch", 400, "all"), ("time", 300, "all")):
            spec = abi.QuerySpec(ks.schema, window, param, group_by=group, aggs=AGGS, output=output, key_capacity=2048)
            c = Case(f"wide-{'_'.join(group)}-{window}", "wide", spec, _pushes(ks, ts, cols, CUTS, 3), ks, -1)
            c.l_row = group.index("l")
            out.append(c)
    return out


def checkpoint_cases():
    ks = longs()
    ts, cols, _ = stream(ks, 12_000, 47, [1, 4_321, 8_000])
    mk = lambda w, p, **kw: abi.QuerySpec(ks.schema, w, p, group_by=ks.group_by, aggs=AGGS, key_capacity=128, **kw)
    specs = [("batch", mk("timeBatch", 500, output="all")), ("sliding", mk("time", 2_000, output="all")),
             ("first_time", mk("lengthBatch", 97, rate=("first_time", 500))),
             ("stream.current", mk("timeBatch", 300, stream_current=True))]
    return [Case(f"ckpt-{n}", "checkpoint", sp, _pushes(ks, ts, cols, [1, 4_321, 8_000], 3), ks, ks.n) for n, sp in specs]


def full_table_keys():
    """16 non-sentinel keys, 8 of them home-colliding, and one more"""
    hc = [int(x) for x in home_colliding_keys(9)]
    return [SENTINEL] + hc[:8] + [3, 5, 6, 7, 11, 12, 13, 14], hc[8]


def query_cases():
    return (batch_cases() + [multisplit_case()] + stream_current_cases() + sliding_cases() + [churn_case()] +
            rate_cases() + partition_cases() + wide_cases() + checkpoint_cases())


# ---- the renaming check --------------------------------------------------------------------------
def rename_cases(cases):
    """the cases whose row order does not depend on the key's value, over key sets without NaNs"""
    return [c for c in cases if c.path in ("batch", "stream.current", "sliding", "rate") and c.ks.name in ("LONGS", "PAIRS_II")]


def renamed_runs(case, run):
    """run(spec, pushes) on the case and on its copy with every key renamed (`renamed`)"""
    import dataclasses
    ks, rk = case.ks, renamed(case.ks)
    nk = len(ks.cols)
    table = {tuple(int(c[i]) for c in ks.cols): i for i in range(ks.n)}
    pushes = []
    for p in case.pushes:
        if isinstance(p, tuple):
            pushes.append(p)
            continue
        idx = np.array([table[t] for t in zip(*[p.cols[c].tolist() for c in range(nk)])])
        pushes.append(abi.HostBatch(rk.schema, p.ts, [c[idx] for c in rk.cols] + p.cols[nk:], p.b.send_size))
    spec = dataclasses.replace(case.spec, schema=rk.schema, group_by=rk.group_by, _keep=[])
    return run(case.spec, case.pushes), run(spec, pushes)
