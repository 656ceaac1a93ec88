"""Expected output of a query with `order by` / `limit` / `offset`.

The frozen oracle (and tests/length_model.py for `length`, tests/having_model.py with `having`) know the
windows and the selector's rows but not the selector's last step, so `apply` restates that step and nothing
else, over an out_arrays-shaped output, and returns the same shape:

    expected = order_model.apply(oracle_output_without_order, terms, limit, offset, ...)

The step (QuerySelector.java:355-370 at the end of processInBatchGroupBy; processNoGroupBy :191-199 and
processInBatchNoGroupBy :304-310 end the same way) runs once per chunk — one flush — on the rows that
survived `having`:

 1. orderEventChunk :452-483 — the chunk is cut into maximal runs of consecutive rows of one type (CURRENT /
    EXPIRED); each run is sorted on its own with List.sort (stable); the runs keep their places.
 2. OrderByEventComparator.compare :63-117, term by term — both values non-null: Integer / Long / Float /
    Double / Boolean.compareTo, negated for desc (Double.compareTo: -0.0 < 0.0, every NaN equal and above
    +Infinity; false < true); exactly one null: the non-null row first, asc and desc alike; both null: the
    next term; all terms equal: 0, the earlier row stays first.
 3. offsetEventChunk :502-519 — the chunk's first `offset` rows are removed.
 4. limitEventChunk :485-500 — `(limit > count) && (CURRENT && currentOn) || (EXPIRED && expiredOn)`, `&&`
    first: an EXPIRED row is always kept and counted, a CURRENT row only while fewer than `limit` rows were
    kept; the count never falls, so a row at position p after the offset is kept iff EXPIRED or p < limit.
 5. a chunk that keeps no row gives no flush; the others keep their clocks.
 6. processInBatchNoGroupBy (aggregators, no group-by; execute :140-159 takes it for every window family): the
    chunk's one row, no ordering; kept iff offset is unset or 0 and limit is unset or > 0 (`single`).
"""
import dataclasses
import functools
import json
import os
import struct

import numpy as np

from siddhi_amd import abi

_FP = (abi.FLOAT, abi.DOUBLE)


def _double_compare(a, b):
    """Double.compareTo"""
    if a < b:
        return -1
    if a > b:
        return 1
    # doubleToLongBits: every NaN is 0x7ff8000000000000; compared as signed longs
    ba = 0x7FF8000000000000 if a != a else struct.unpack("<q", struct.pack("<d", a))[0]
    bb = 0x7FF8000000000000 if b != b else struct.unpack("<q", struct.pack("<d", b))[0]
    return 0 if ba == bb else (-1 if ba < bb else 1)


def compare(r1, r2, terms, is_fp):
    """OrderByEventComparator.compare on two rows' term values (None = null)"""
    for t, term in enumerate(terms):
        v1, v2 = r1[t], r2[t]
        if v1 is not None and v2 is not None:
            res = _double_compare(v1, v2) if is_fp[t] else (v1 > v2) - (v1 < v2)
            if len(term) > 2 and term[2] == "desc":
                res = -res
            if res != 0:
                return res
        elif v1 is not None:
            return -1
        elif v2 is not None:
            return 1
    return 0


def single_row(spec):
    """rule 6 applies: aggregators without group-by (the selector batches for every window family, execute :140-159)"""
    return not spec.group_by and len(spec.aggs) > 0


def key_types(spec):
    return [spec.schema.types[spec.schema.col(g)] for g in spec.group_by]


def new_counters():
    return {"flushes": 0, "tie_by_position": 0, "null_order_value": 0, "emptied_by_offset": 0,
            "emptied": 0, "limit_cut_current_expired_after": 0, "alternating": 0, "sizes": set()}


def apply(out, terms=(), limit=None, offset=None, ktypes=(), single=False, counters=None):
    """The step over an out_arrays-shaped output; returns the same shape. terms: abi.compile_order's syntax.
    ktypes: abi types of the key columns (a float / double key is reported as its double's bits). counters:
    new_counters(), filled with what the flushes exercised; sizes: the row counts of the flushes that were sorted."""
    terms = list(terms or ())
    fo, fc = out["flush_offsets"], out["flush_clock"]
    vt = [int(t) for t in out["val_types"]]
    n = len(out["ts"])
    is_fp = []
    cols = []  # per term: the rows' values as Python numbers, None where null
    for kind, idx, *_ in terms:
        if kind == "key":
            fp = ktypes[idx] in _FP
            raw = out["keys"][idx]
            col = raw.view(np.float64).tolist() if fp else raw.tolist()
        else:
            fp = vt[idx] in _FP
            raw = out["vals"][idx]
            col = raw.view(np.float64).tolist() if fp else raw.view(np.int64).tolist()
            col = [None if nl else v for v, nl in zip(col, out["nulls"][idx].tolist())]
        is_fp.append(fp)
        cols.append(col)
    exp = out["expired"].tolist()
    cmp = functools.cmp_to_key(lambda a, b: compare(a[1], b[1], terms, is_fp))
    keep, nfo, nfc = [], [0], []
    for f in range(len(fc)):
        lo, hi = int(fo[f]), int(fo[f + 1])
        rows = list(range(lo, hi))
        if counters is not None:
            counters["flushes"] += 1
        if single:
            assert hi - lo == 1, "processInBatchNoGroupBy: one row per chunk"
            if not ((offset is None or offset == 0) and (limit is None or limit > 0)):
                rows = []
        else:
            if terms and hi - lo > 1:
                ordered, run = [], []
                nruns = 0
                for r in rows + [None]:
                    if r is not None and (not run or exp[r] == exp[run[-1]]):
                        run.append(r)
                        continue
                    vals = [(q, tuple(c[q] for c in cols)) for q in run]
                    srt = sorted(vals, key=cmp)  # (stable, as List.sort)
                    nruns += 1
                    if counters is not None:
                        if any(compare(a[1], b[1], terms, is_fp) == 0 for a, b in zip(srt, srt[1:])):
                            counters["tie_by_position"] += 1
                        if len(run) > 1 and any(v is None for _, vs in vals for v in vs):
                            counters["null_order_value"] += 1
                    ordered += [q for q, _ in srt]
                    run = [r]
                rows = ordered
                if counters is not None:
                    counters["sizes"].add(hi - lo)
                    if nruns == hi - lo:
                        counters["alternating"] += 1
            if offset:
                if counters is not None and rows and offset >= len(rows):
                    counters["emptied_by_offset"] += 1
                rows = rows[offset:]
            if limit is not None:
                kept = [r for p, r in enumerate(rows) if exp[r] or p < limit]
                if counters is not None:
                    cut = [p for p, r in enumerate(rows) if not (exp[r] or p < limit)]
                    if cut and any(exp[r] for r in rows[cut[0] + 1:]):
                        counters["limit_cut_current_expired_after"] += 1
                rows = kept
        if not rows:
            if counters is not None:
                counters["emptied"] += 1
            continue
        keep += rows
        nfo.append(len(keep))
        nfc.append(int(fc[f]))
    idx = np.array(keep, np.int64)
    res = {"flush_offsets": np.array(nfo, np.int64), "flush_clock": np.array(nfc, np.int64),
           "val_types": out["val_types"].copy()}
    for k in ("ts", "expired", "rep"):
        res[k] = out[k][idx] if n else out[k].copy()
    for k in ("keys", "vals", "nulls"):
        res[k] = out[k][:, idx] if n else out[k].copy()
    return res


# ---- expected output of a spec (window behaviour from the oracle / the length model / the having model) ----

def base_output(spec, pushes):
    """`spec` without order / limit / offset and without its limiter, over `pushes`"""
    from oracle.oracle import OracleQuery
    from tests.parity import run_pushes
    plain = dataclasses.replace(spec, order_by=None, limit=None, offset=None, rate=None)
    if spec.window == "length":
        from tests import length_model
        return length_model.run_model(plain, pushes)
    if spec.having is not None:
        from tests import having_model
        return having_model.run_model(plain, pushes)
    q = OracleQuery(plain)
    out = run_pushes(q, pushes)
    q.close()
    return out


def rate_limited(out, kind, n, grouped):
    """py_limit (tests/test_oracle_rate.py) over an out_arrays-shaped output, back in that shape"""
    from tests.test_oracle_rate import flushes_of, py_limit
    fl = py_limit(flushes_of(out), kind, n, grouped)
    nk, na = out["keys"].shape[0], out["vals"].shape[0]
    rows = [p for _, ps in fl for p in ps]
    m = len(rows)
    fo = np.cumsum([0] + [len(ps) for _, ps in fl]).astype(np.int64)
    return {
        "flush_offsets": fo, "flush_clock": np.array([c for c, _ in fl], np.int64), "val_types": out["val_types"].copy(),
        "ts": np.array([p[0] for p in rows], np.int64), "expired": np.array([p[1] for p in rows], np.uint8),
        "rep": np.array([p[5] for p in rows], np.int64),
        "keys": np.array([p[2] for p in rows], np.int64).reshape(m, nk).T.copy(),
        "vals": np.array([p[3] for p in rows], np.uint64).reshape(m, na).T.copy(),
        "nulls": np.array([p[4] for p in rows], np.uint8).reshape(m, na).T.copy(),
    }


def expected(spec, pushes, counters=None, base=None):
    out = base_output(spec, pushes) if base is None else base
    out = apply(out, spec.order_by, spec.limit, spec.offset, key_types(spec), single_row(spec), counters)
    if spec.rate:
        out = rate_limited(out, spec.rate[0], spec.rate[1], bool(spec.group_by))
    return out


# ---- the cases tests/test_order_model.py and tests/test_gpu_order.py share -----------------------------------
SCHEMA = abi.Schema.parse("k int, v double, x long, ts long")
AGGS = [("count", None), ("sum", "v"), ("min", "x"), ("max", "x"), ("avg", "x"), ("sum", "x")]
# the largest flush the block route can hold (kOrdBlockRows, sh_order.h) and the default route threshold (the
# measured crossover, Tuning::ord_block_max); the forced routes are SH_ORD_BLOCK_MAX = 0 (global) and = BLOCK_ROWS
BLOCK_ROWS = 1024
DEFAULT_THRESHOLD = 256
ROUTES = {"default": None, "global": "0", "block": str(BLOCK_ROWS), "threshold64": "64"}

TERMS = {
    "none": None,
    "sumx_asc": [("agg", 5, "asc")],
    "avgx_desc": [("agg", 4, "desc")],
    "count": [("agg", 0)],                                     # many ties, decided by position
    "count_key": [("agg", 0, "desc"), ("key", 0, "asc")],      # many ties, decided by the key
    "key_desc": [("key", 0, "desc")],
    "four": [("agg", 0, "asc"), ("agg", 2, "desc"), ("agg", 1, "asc"), ("key", 0, "desc")],
    "sumv": [("agg", 1, "asc"), ("agg", 0, "desc")],            # a double sum with NaN / +-0.0 / +-Infinity
    "minmax": [("agg", 2, "desc"), ("agg", 3, "asc")],          # null on an EXPIRED row whose key emptied
}
LIMITS = [None, 0, 1, 10]
OFFSETS = [None, 0, 1, 5000]   # (5000: more rows than any flush holds)

# window families: name -> (window, param, extra QuerySpec fields)
WINDOWS = {
    "lengthBatch1": ("lengthBatch", 1, {}),
    "lengthBatch4": ("lengthBatch", 4, {}),
    "lengthBatch65": ("lengthBatch", 65, {}),
    "lengthBatch2500": ("lengthBatch", 2500, {}),
    "timeBatch700": ("timeBatch", 700, {}),
    "extTimeBatch700": ("externalTimeBatch", 700, {"ts_attr": "ts"}),
    "lengthBatch65sc": ("lengthBatch", 65, {"stream_current": True}),
    "time500": ("time", 500, {}),
    "externalTime500": ("externalTime", 500, {"ts_attr": "ts"}),
    "length300": ("length", 300, {}),
}
EVENTS = 6_000


def stream(keys, seed=11, n=EVENTS, special=False):
    """tests/having_model.stream's shape. special: v depends on the key alone — NaN for k % 6 == 0, +Infinity
    for 1, -Infinity for 2, -0.0 for 3, 0.0 for 4 — so that no sum adds +Infinity to -Infinity (the sign of a
    generated NaN is the adder's choice, not the library's)."""
    rng = np.random.default_rng(seed)
    ts = np.cumsum(rng.integers(0, 40, n)).astype(np.int64) + 5_000
    ts[n // 2:] += 20_000
    k = rng.integers(0, keys, n).astype(np.int32)
    v = rng.integers(-4000, 4000, n).astype(np.float64) / 16.0
    if special:
        table = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0])
        m = k % 6
        v = np.where(m < 5, table[np.minimum(m, 4)], v)
    x = rng.integers(-10**6, 10**6, n).astype(np.int64)
    return ts, [k, v, x, ts.copy()]


def make_pushes(ts, cols, send_size, advance=True, schema=SCHEMA):
    """cut in three, an advance between the pushes and one behind them (it closes a timeBatch window)"""
    from tests.parity import split_batches
    n = len(ts)
    cuts = [n // 3 + 1, 2 * n // 3 + 7]
    pushes = split_batches(schema, ts, cols, cuts, send_size)
    if advance:
        pushes.insert(2, ("advance", int(ts[cuts[1] - 1]) + 1_500))
        pushes.append(("advance", int(ts[-1]) + 5_000))
    return pushes


def make_spec(family, output="current", keys=12, terms="sumx_asc", limit=None, offset=None, grouped=True, aggs=AGGS,
              **kw):
    window, param, extra = WINDOWS[family]
    return abi.QuerySpec(SCHEMA, window, param, group_by=["k"] if grouped else (), aggs=aggs, output=output,
                         key_capacity=max(16, 2 * keys), order_by=TERMS[terms] if isinstance(terms, str) else terms,
                         limit=limit, offset=offset, **extra, **kw)


def matrix():
    """(family, output, keys, send size, terms, limit, offset): every window with every output; key counts, send
    sizes, terms, limits and offsets rotate so that each value meets every window and every output."""
    names = [t for t in TERMS if t not in ("none", "sumv")]
    out = []
    i = 0
    for a, fam in enumerate(WINDOWS):
        for b, output in enumerate(("current", "expired", "all")):
            for c in range(2):
                keys = (12, 3000)[(a + b + c) % 2]
                ss = (1, 50)[(a + c) % 2]
                if ss == 1 and keys == 3000 and fam in ("time500", "externalTime500", "length300"):
                    ss = 50  # (a flush per event: nothing to sort; kept for 12 keys)
                terms = names[i % len(names)]
                limit = LIMITS[(i + a) % 4]
                offset = OFFSETS[(i // 2 + b) % 4]
                if limit is None and offset is None and terms is None:
                    limit = 1
                out.append((fam, output, keys, ss, terms, limit, offset))
                i += 1
    return out


_cache = {}


def case(fam, output, keys, ss, terms, limit, offset, special=False, **kw):
    """(spec, pushes, expected output, counters) of one case; the base output is computed once per query shape"""
    key = (fam, output, keys, ss, terms if isinstance(terms, str) else repr(terms), limit, offset, special,
           repr(sorted(kw.items())))
    if key not in _cache:
        spec = make_spec(fam, output, keys, terms, limit, offset, **kw)
        ts, cols = stream(keys, special=special)
        pushes = make_pushes(ts, cols, ss)
        bkey = ("base", fam, output, keys, ss, special, repr(sorted(kw.items())))
        if bkey not in _cache:
            _cache[bkey] = base_output(spec, pushes)
        cnt = new_counters()
        _cache[key] = (spec, pushes, expected(spec, pushes, cnt, base=_cache[bkey]), cnt)
    return _cache[key]


# flush sizes around every boundary of the sort: one row, a pair, the wave (64), the workgroup = the default
# route threshold (256), its rows-per-thread steps (512), the block route's capacity (1024), and beyond
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2048, 3000]


def sizes_stream(seed=5):
    """timeBatch(1000) windows of exactly SIZES[w] distinct keys each (window w: [w * 1000, w * 1000 + 1000)),
    so flush w has SIZES[w] rows; count ties abound (every key once) and x decides"""
    rng = np.random.default_rng(seed)
    ks, tss = [], []
    for w, m in enumerate(SIZES):
        ks.append(rng.permutation(4000)[:m].astype(np.int32))
        tss.append(np.sort(rng.integers(0, 1000, m)).astype(np.int64) + 1000 * w + 10_000)
    k = np.concatenate(ks)
    ts = np.concatenate(tss)
    n = len(k)
    v = rng.integers(-4000, 4000, n).astype(np.float64) / 16.0
    x = rng.integers(-50, 50, n).astype(np.int64)  # (few values: ties)
    return ts, [k, v, x, ts.copy()]


def sizes_case(terms="four", limit=None, offset=None, output="current"):
    """one push per window (a call then holds one flush: the route is chosen per call) and a closing advance"""
    key = ("sizes", terms, limit, offset, output)
    if key not in _cache:
        from tests.parity import split_batches
        ts, cols = sizes_stream()
        cuts = np.cumsum(SIZES)[:-1].tolist()
        pushes = split_batches(SCHEMA, ts, cols, cuts, 0) + [("advance", int(ts[-1]) + 3_000)]
        spec = abi.QuerySpec(SCHEMA, "timeBatch", 1000, group_by=["k"], aggs=AGGS, output=output, key_capacity=8192,
                             start_time=10_000, order_by=TERMS[terms], limit=limit, offset=offset)
        cnt = new_counters()
        _cache[key] = (spec, pushes, expected(spec, pushes, cnt), cnt)
    return _cache[key]


# ---- float / bool key terms, float and double min / max over +-0.0 ------------------------------------------
TYPED_SCHEMA = abi.Schema.parse("k int, v double, f float, b bool, ts long")
TYPED_AGGS = [("count", None), ("min", "v"), ("max", "v"), ("min", "f"), ("max", "f")]
# (group-by columns, terms): a float key and a bool key as terms, a float beside an int key, double and float
# min / max (a float is reported widened to double) whose values include -0.0 and 0.0
TYPED = {
    "float_key": (["f"], [("key", 0, "desc")]),
    "bool_key": (["b"], [("key", 0, "desc"), ("agg", 0)]),
    "int_float_keys": (["k", "f"], [("key", 1), ("key", 0, "desc")]),
    "min_double": (["k"], [("agg", 1), ("key", 0)]),
    "max_double_desc": (["k"], [("agg", 2, "desc"), ("key", 0)]),
    "min_float": (["k"], [("agg", 3), ("agg", 4, "desc"), ("key", 0)]),
}


def typed_stream(n=3000, seed=23):
    """v and f drawn from a few values around zero: a key's min / max is -0.0 for some keys and 0.0 for others
    (the aggregators keep the first of two equal values), and f as a key takes both zeros"""
    rng = np.random.default_rng(seed)
    ts = np.cumsum(rng.integers(0, 40, n)).astype(np.int64) + 5_000
    k = rng.integers(0, 40, n).astype(np.int32)
    zeros = np.array([-0.0, 0.0, 0.0, -0.0, 1.5, -2.25, 7.0, -0.5])
    v = zeros[rng.integers(0, len(zeros), n)]
    f = zeros[rng.integers(0, len(zeros), n)].astype(np.float32)
    # a third of the keys see nothing below zero: their min is one of the zeros
    pos = (k % 3 == 0)
    v = np.where(pos & (v < 0), -v, v)
    f = np.where(pos & (f < 0), -f, f).astype(np.float32)
    b = (rng.integers(0, 2, n)).astype(np.uint8)
    return ts, [k, v, f, b, ts.copy()]


def typed_case(name, fam="timeBatch700", output="current", limit=None, offset=None):
    key = ("typed", name, fam, output, limit, offset)
    if key not in _cache:
        group_by, terms = TYPED[name]
        window, param, extra = WINDOWS[fam]
        extra = {k: v for k, v in extra.items() if k != "ts_attr"}
        spec = abi.QuerySpec(TYPED_SCHEMA, window, param, group_by=group_by, aggs=TYPED_AGGS, output=output,
                             key_capacity=256, order_by=terms, limit=limit, offset=offset, **extra)
        ts, cols = typed_stream()
        pushes = make_pushes(ts, cols, 50, schema=TYPED_SCHEMA)
        cnt = new_counters()
        _cache[key] = (spec, pushes, expected(spec, pushes, cnt), cnt)
    return _cache[key]


def load_kats():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_order_limit.json")) as f:
        return json.load(f)
