"""Expected output of a batch-window query with a `having` condition.

The frozen oracle knows every window but its selector has no `having`, so the model takes all window
behaviour from the oracle and restates only the selector (QuerySelector.processInBatchGroupBy,
core/query/selector/QuerySelector.java:315-374; processInBatchNoGroupBy :271-313):

  a chunk is what the window hands the selector in one call; RESET empties every key's aggregators; within
  a chunk, in stream order, each event is folded into its key's state, the key's output row is formed (the
  event's timestamp, the event as `rep`, the aggregates after the fold), `having` is evaluated on that row
  and, if it passes, grouped[key] = row — the key keeps the position of its FIRST pass and the row of its
  LAST pass. After the chunk the flush holds the grouped rows in insertion order at the chunk's flush clock;
  an empty `grouped` gives no flush.

Two oracle queries run over the same pushes, both with the spec's window, parameters, filter,
stream_current and output mode: (a) no group-by, no aggregators — each flush is one chunk, its rows the
chunk's events (rep = stream index); (b) no group-by, count() — each flush gives the count at the chunk's
last event, which tells whether a RESET preceded the chunk (for these windows a RESET never falls between
two events of one chunk).

Only predicates whose Python comparison is exact are meaningful: a LONG aggregate against an INT / LONG
constant, a DOUBLE aggregate against a DOUBLE constant, an INT key against an INT constant.
"""
import dataclasses

import numpy as np

from oracle.oracle import OracleQuery
from siddhi_amd import abi
from tests.parity import run_pushes

_FP = (abi.FLOAT, abi.DOUBLE)


def _wrap64(x):
    return ((x + 2**63) % 2**64) - 2**63


def val_types(spec):
    out = []
    for fn, col in spec.aggs:
        t = spec.schema.types[spec.schema.col(col)] if col is not None else abi.LONG
        if fn == "count":
            out.append(abi.LONG)
        elif fn == "sum":
            out.append(abi.DOUBLE if t in _FP else abi.LONG)
        elif fn == "avg":
            out.append(abi.DOUBLE)
        else:
            out.append(t)
    return out


class _Key:
    """One key's aggregator state: the Java executors' add-only forms."""

    def __init__(self, spec):
        self.c = 0
        self.s = [None] * len(spec.aggs)

    def fold(self, spec, ev):
        self.c += 1
        for a, (fn, col) in enumerate(spec.aggs):
            if fn == "count":
                continue
            ci = spec.schema.col(col)
            x = ev[ci]
            fp = spec.schema.types[ci] in _FP
            s = self.s[a]
            if fn == "sum":
                if fp:
                    self.s[a] = (0.0 if s is None else s) + float(x)   # sequential double adds
                else:
                    self.s[a] = _wrap64((0 if s is None else s) + int(x))  # Java long wraps
            elif fn == "avg":
                self.s[a] = (0.0 if s is None else s) + float(x)
            elif fn == "min":
                self.s[a] = x if s is None or x < s else s
            else:
                self.s[a] = x if s is None or x > s else s

    def values(self, spec):
        out = []
        for a, (fn, col) in enumerate(spec.aggs):
            if fn == "count":
                out.append(self.c)
            elif fn == "avg":
                out.append(self.s[a] / float(self.c))
            else:
                out.append(self.s[a])
        return out


def evaluate(expr, keys, vals):
    """The having condition on one row (plain Python comparisons: see the module docstring)."""
    def operand(x):
        if isinstance(x, tuple) and len(x) == 2 and x[0] == "agg":
            return vals[x[1]]
        if isinstance(x, tuple) and len(x) == 2 and x[0] == "key":
            return keys[x[1]]
        if isinstance(x, tuple) and len(x) == 2 and x[0] in abi.TYPE_NAMES:
            return x[1]
        return x
    head = expr[0]
    if head == "and":
        return evaluate(expr[1], keys, vals) and evaluate(expr[2], keys, vals)
    if head == "or":
        return evaluate(expr[1], keys, vals) or evaluate(expr[2], keys, vals)
    if head == "not":
        return not evaluate(expr[1], keys, vals)
    a, b = operand(expr[1]), operand(expr[2])
    return {">": a > b, ">=": a >= b, "<": a < b, "<=": a <= b, "==": a == b, "!=": a != b}[head]


def _events(spec, pushes):
    """The pushes' columns as Python values, by stream index."""
    batches = [p for p in pushes if not (isinstance(p, tuple) and p[0] == "advance")]
    cols = []
    for c, t in enumerate(spec.schema.types):
        col = np.concatenate([b.cols[c] for b in batches])
        cols.append(col.astype(np.float64).tolist() if t in _FP else col.astype(np.int64).tolist())
    return cols


def chunks(spec, pushes):
    """[(flush clock, reset before it, [(stream index, timestamp) of the chunk's events])] from the oracle."""
    base = dict(having=None, rate=None, group_by=())
    qa = OracleQuery(dataclasses.replace(spec, aggs=(), **base))
    qb = OracleQuery(dataclasses.replace(spec, aggs=[("count", None)], **base))
    A = run_pushes(qa, pushes)
    B = run_pushes(qb, pushes)
    qa.close()
    qb.close()
    assert np.array_equal(A["flush_clock"], B["flush_clock"])
    nf = len(A["flush_clock"])
    assert np.array_equal(B["flush_offsets"], np.arange(nf + 1))
    counts = B["vals"][0].view(np.int64)
    out, n = [], 0
    for f in range(nf):
        lo, hi = int(A["flush_offsets"][f]), int(A["flush_offsets"][f + 1])
        cnt = int(counts[f])
        reset = cnt != n + (hi - lo)
        if reset:
            assert cnt == hi - lo, (f, cnt, n, hi - lo)
        n = cnt
        out.append((int(A["flush_clock"][f]), reset, list(zip(A["rep"][lo:hi].tolist(), A["ts"][lo:hi].tolist()))))
    return out


def run_model(spec, pushes, having="spec", chunk_list=None, on_chunk=None):
    """out_arrays-shaped expected output of `spec` (its `having`, or the one given; None = no having) over
    `pushes`. on_chunk(index, grouped) sees every chunk's surviving {key: (ts, rep, values)} in order."""
    if having == "spec":
        having = spec.having
    cols = _events(spec, pushes)
    gcols = [spec.schema.col(g) for g in spec.group_by]
    vt = val_types(spec)
    na, nk = len(spec.aggs), len(gcols)
    state = {}
    fo, fc, ts, rep, keys, vals = [0], [], [], [], [], []
    for ci, (clock, reset, evs) in enumerate(chunk_list if chunk_list is not None else chunks(spec, pushes)):
        if reset:
            state.clear()
        grouped = {}
        for e, t in evs:
            ev = [c[e] for c in cols]
            key = tuple(int(ev[g]) for g in gcols)
            st = state.get(key)
            if st is None:
                st = state[key] = _Key(spec)
            st.fold(spec, ev)
            v = st.values(spec)
            if having is None or evaluate(having, key, v):
                grouped[key] = (t, e, v)   # (a dict keeps the position of the key's first insertion)
        if on_chunk:
            on_chunk(ci, grouped)
        if not grouped:
            continue
        for key, (t, e, v) in grouped.items():
            ts.append(t); rep.append(e); keys.append(key); vals.append(v)
        fo.append(len(ts))
        fc.append(clock)
    n = len(ts)
    V = np.zeros((na, n), np.uint64)
    for a in range(na):
        colv = [v[a] for v in vals]
        V[a] = (np.array(colv, np.float64) if vt[a] in _FP else np.array(colv, np.int64)).view(np.uint64) \
            if n else np.zeros(0, np.uint64)
    return {
        "flush_offsets": np.array(fo, np.int64), "flush_clock": np.array(fc, np.int64),
        "val_types": np.array(vt, np.int32), "ts": np.array(ts, np.int64), "expired": np.zeros(n, np.uint8),
        "rep": np.array(rep, np.int64),
        "keys": np.array(keys, np.int64).reshape(n, nk).T.copy() if nk else np.zeros((0, n), np.int64),
        "vals": V, "nulls": np.zeros((na, n), np.uint8),
    }


# ---- the cases tests/test_having_model.py and tests/test_gpu_having.py share ------------------------------
SCHEMA = abi.Schema.parse("k int, v double, x long, ts long")
AGGS = [("count", None), ("sum", "v"), ("min", "v"), ("max", "x"), ("avg", "x"), ("sum", "x")]
FILTER = (">", "v", -180.0)
CUTS = [1, 777, 2499, 2500, 3300]

# window families: (name, window, param, extra QuerySpec fields)
WINDOWS = {
    "lengthBatch37": ("lengthBatch", 37, {}),
    "timeBatch700": ("timeBatch", 700, {}),
    "timeBatch333s": ("timeBatch", 333, {"start_time": 100}),
    "extTimeBatch700": ("externalTimeBatch", 700, {"ts_attr": "ts"}),
}
PREDICATES = {
    "count==2": ("==", ("agg", 0), ("long", 2)),
    "count<=3&sumv>-100": ("and", ("<=", ("agg", 0), 3), (">", ("agg", 1), -100.0)),
    "avgx>0|minv<-240": ("or", (">", ("agg", 4), 0.0), ("<", ("agg", 2), -240.0)),
    "sumx>=500000": (">=", ("agg", 5), 500000),
    "not(k==3)": ("not", ("==", ("key", 0), 3)),
}


def stream(n=4000, keys=12, seed=3):
    """The generator of tests/test_gpu_stream_current.py with its gap at event 2500."""
    rng = np.random.default_rng(seed)
    ts = np.cumsum(rng.integers(0, 40, n)).astype(np.int64) + 5_000
    ts[2500:] += 20_000
    k = rng.integers(0, keys, n).astype(np.int32)
    v = rng.integers(-4000, 4000, n).astype(np.float64) / 16.0
    x = rng.integers(-10**6, 10**6, n).astype(np.int64)
    return ts, [k, v, x, ts.copy()]


def make_pushes(ts, cols, send_size, cuts=CUTS):
    from tests.parity import split_batches
    pushes = split_batches(SCHEMA, ts, cols, cuts, send_size)
    pushes.insert(3, ("advance", int(ts[cuts[2]]) + 1_500))
    pushes.append(("advance", int(ts[-1]) + 5_000))
    return pushes


def make_spec(family, stream_current, grouped, having=None, keys=12, aggs=AGGS, **kw):
    window, param, extra = WINDOWS[family]
    return abi.QuerySpec(SCHEMA, window, param, group_by=["k"] if grouped else (), aggs=aggs, filter=FILTER,
                         stream_current=stream_current, key_capacity=max(16, 2 * keys), having=having, **extra, **kw)


def matrix():
    """(family, stream_current, grouped, send_size, predicate name) of the GPU matrix."""
    out = []
    for fam in WINDOWS:
        for sc in (False, True):
            if sc and fam == "extTimeBatch700":
                continue
            for grouped in (True, False):
                for ss in (1, 13, 0):
                    for pn in PREDICATES:
                        if pn == "not(k==3)" and not grouped:
                            continue  # (no group-by: there is no key to name)
                        out.append((fam, sc, grouped, ss, pn))
    return out
