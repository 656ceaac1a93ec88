"""Expected output of the sliding `#window.length(N)`.

The frozen oracle has no length window, so the window is restated here (as `having` is in
tests/having_model.py) from LengthWindowProcessor.process
(core/query/processor/stream/window/LengthWindowProcessor.java:106-142) and the selector
(QuerySelector.processInBatchGroupBy, core/query/selector/QuerySelector.java:315-374;
processInBatchNoGroupBy :271-313; processNoGroupBy :161-205 for `select *`):

  the window state is a count and one FIFO of the last N events that passed the filter. The first N passing
  events only enter; from then on every arrival first polls the head, re-stamps it with currentTime and
  inserts it before the current event. currentTime is read once per process call, so every expired copy of
  one send carries that send's playback clock — max(previous clock, the send's last event timestamp). One
  send is one chunk [exp, cur, exp, cur, ...] over its passing events; there is no RESET and no scheduler
  (`('advance', t)` only moves the clock).

  Per chunk event, in order: a CURRENT event is added to its key's aggregators, an EXPIRED one removed (the
  Java forms, tests/having_expired_model.KeyState); a key's state whose count reached 0 with every sum / avg
  running value equal to 0.0 is destroyed (AttributeAggregatorExecutor canDestroy) and the next one starts
  from +0.0. If the event's type is switched on, grouped[key] = row: one row per (chunk, key) at the place of
  the key's first such event with the content after its last, a key's CURRENT and EXPIRED rows sharing one
  slot. A chunk that keeps no row gives no flush. An EXPIRED row's timestamp is the clock, its `rep` the
  expired event.
"""
import collections

import numpy as np

from siddhi_amd import abi
from tests import having_model as hm
from tests.having_expired_model import KeyState

_FP = (abi.FLOAT, abi.DOUBLE)


def _filter_fn(schema, expr):
    """expr (abi.compile_filter's syntax) -> f(event values) with plain Python comparisons"""
    if expr is None:
        return lambda ev: True

    def operand(x):
        if isinstance(x, str):
            c = schema.col(x)
            return lambda ev: ev[c]
        if isinstance(x, tuple) and len(x) == 2 and x[0] in abi.TYPE_NAMES:
            return lambda ev: x[1]
        if isinstance(x, (bool, int, float)):
            return lambda ev: x
        return walk(x)

    def walk(e):
        head = e[0]
        if head == "and":
            a, b = walk(e[1]), walk(e[2])
            return lambda ev: a(ev) and b(ev)
        if head == "or":
            a, b = walk(e[1]), walk(e[2])
            return lambda ev: a(ev) or b(ev)
        if head == "not":
            a = walk(e[1])
            return lambda ev: not a(ev)
        a, b = operand(e[1]), operand(e[2])
        return {">": lambda ev: a(ev) > b(ev), ">=": lambda ev: a(ev) >= b(ev), "<": lambda ev: a(ev) < b(ev),
                "<=": lambda ev: a(ev) <= b(ev), "==": lambda ev: a(ev) == b(ev), "!=": lambda ev: a(ev) != b(ev)}[head]

    return walk(expr)


def _destroyable(spec, st):
    """canDestroy: count 0 and every sum / avg running value == 0.0 (a residue keeps the state alive)"""
    return st.c == 0 and all(st.s[a] is None or st.s[a] == 0 for a, (fn, _) in enumerate(spec.aggs)
                             if fn in ("sum", "avg"))


def run_model(spec, pushes, counters=None):
    """out_arrays-shaped expected output of the length(N) query `spec` over `pushes` (HostBatch or
    ('advance', t)). counters (a dict) receives the coverage counts tests/test_length_model.py asserts."""
    assert spec.window == "length" and spec.param >= 1
    cnt = counters if counters is not None else {}
    for k in ("expired_rows", "null_in_row", "current_replaces_expired", "non_front", "push_without_pass",
              "destroyed", "residue_kept"):
        cnt.setdefault(k, 0)
    N = spec.param
    cur_on, exp_on = spec.output in ("current", "all"), spec.output in ("expired", "all")
    cols = hm._events(spec, pushes) if any(not isinstance(p, tuple) for p in pushes) else []
    passes = _filter_fn(spec.schema, spec.filter)
    gcols = [spec.schema.col(g) for g in spec.group_by]
    vt = hm.val_types(spec)
    na, nk = len(spec.aggs), len(gcols)
    pass_through = na == 0 and nk == 0
    state, fifo = {}, collections.deque()
    clock, base = None, 0
    fo, fc, ts, rep, exp, keys, vals = [0], [], [], [], [], [], []
    for p in pushes:
        if isinstance(p, tuple) and p[0] == "advance":
            if clock is None or p[1] >= clock:   # TimestampGeneratorImpl: the clock only moves forward
                clock = p[1]
            continue
        n = len(p.ts)
        ss = p.b.send_size if p.b.send_size > 0 else max(n, 1)
        any_pass = False
        for lo in range(0, n, ss):
            hi = min(n, lo + ss)
            last = int(p.ts[hi - 1])
            clock = last if clock is None else max(clock, last)
            # ---- the window: one chunk per send
            chunk = []   # (stream index, timestamp, expired)
            for e in range(base + lo, base + hi):
                ev = [c[e] for c in cols]
                if not passes(ev):
                    continue
                any_pass = True
                if len(fifo) >= N:
                    chunk.append((fifo.popleft(), clock, 1))
                fifo.append(e)
                chunk.append((e, int(p.ts[e - base]), 0))
            # ---- the selector
            grouped, rows = {}, []
            for e, t, x in chunk:
                ev = [c[e] for c in cols]
                key = tuple(int(ev[g]) for g in gcols)
                v = []
                if not pass_through:
                    st = state.get(key)
                    if st is None:
                        st = state[key] = KeyState(spec, cnt)
                    if x:
                        st.remove(ev)
                    else:
                        st.add(ev)
                    v = st.values()
                    if st.c == 0:
                        if _destroyable(spec, st):
                            del state[key]
                            cnt["destroyed"] += 1
                        else:
                            cnt["residue_kept"] += 1
                if not (exp_on if x else cur_on):
                    continue
                if pass_through:
                    rows.append((t, e, x, key, v))
                else:
                    if not x and key in grouped and grouped[key][2]:
                        cnt["current_replaces_expired"] += 1
                    grouped[key] = (t, e, x, key, v)
            rows = rows if pass_through else list(grouped.values())
            if not rows:
                continue
            for t, e, x, key, v in rows:
                ts.append(t); rep.append(e); exp.append(x); keys.append(key); vals.append(v)
                cnt["expired_rows"] += x
                cnt["null_in_row"] += any(y is None for y in v)
            fo.append(len(ts))
            fc.append(clock)
        cnt["push_without_pass"] += not any_pass
        base += n
    n = len(ts)
    V = np.zeros((na, n), np.uint64)
    NL = np.zeros((na, n), np.uint8)
    for a in range(na):
        colv = [0 if v[a] is None else v[a] for v in vals]
        NL[a] = [v[a] is None for v in vals]
        if n:
            V[a] = (np.array(colv, np.float64) if vt[a] in _FP else np.array(colv, np.int64)).view(np.uint64)
    return {
        "flush_offsets": np.array(fo, np.int64), "flush_clock": np.array(fc, np.int64),
        "val_types": np.array(vt, np.int32), "ts": np.array(ts, np.int64), "expired": np.array(exp, np.uint8),
        "rep": np.array(rep, np.int64),
        "keys": np.array(keys, np.int64).reshape(n, nk).T.copy() if nk else np.zeros((0, n), np.int64),
        "vals": V, "nulls": NL,
    }


class ModelQuery:
    """run_model behind the push / advance_time interface of tests/kat_runner.py (every call re-runs the
    model over all pushes so far and returns the new flushes)."""

    def __init__(self, spec):
        self.spec, self.pushes, self.nf = spec, [], 0

    def _step(self, p):
        self.pushes.append(p)
        A = run_model(self.spec, self.pushes)
        out = []
        for f in range(self.nf, len(A["flush_clock"])):
            lo, hi = int(A["flush_offsets"][f]), int(A["flush_offsets"][f + 1])
            rows = []
            for r in range(lo, hi):
                vs = []
                for a in range(A["vals"].shape[0]):
                    if A["nulls"][a, r]:
                        vs.append(None)
                    elif A["val_types"][a] in _FP:
                        vs.append(float(A["vals"][a, r:r + 1].view(np.float64)[0]))
                    else:
                        vs.append(int(A["vals"][a, r:r + 1].view(np.int64)[0]))
                rows.append((int(A["ts"][r]), int(A["expired"][r]), tuple(int(k) for k in A["keys"][:, r]), tuple(vs)))
            out.append(abi.Flush(int(A["flush_clock"][f]), rows, [int(x) for x in A["rep"][lo:hi]]))
        self.nf = len(A["flush_clock"])
        return out

    def push(self, batch):
        return self._step(batch)

    def advance_time(self, now):
        return self._step(("advance", now))

    def close(self):
        pass


# ---- the cases tests/test_length_model.py and tests/test_gpu_length.py share -------------------------------
# `ord` is the ordinal of the event among the passing ones (the oracle's externalTime(ord, N) is the
# independent route of tests/test_length_model.py; the length query ignores the column)
SCHEMA = abi.Schema.parse("k int, v double, x long, ord long, ts long")
AGGS = [("count", None), ("sum", "v"), ("min", "v"), ("max", "x"), ("avg", "x"), ("sum", "x")]
FILTER = (">", "v", -180.0)
# few values: duplicates abound in a key's deque (-190 fails the filter) ...
V_DEQUE = np.array([-190.0, -7.5, -2.0, 0.0, 1.5, 3.0, 8.25])
# ... and values whose sums leave residues, with -0.0 and cancelling giants
V_RESIDUE = np.array([-190.0, 0.1, 0.7, -0.0, 1e16, -1e16, 3.3, -0.3])


def stream(n, keys, seed, values=V_DEQUE, filtered=True):
    """tests/having_model.stream's timestamps and x, v drawn from `values`, `ord` filled in"""
    rng = np.random.default_rng(seed)
    ts = np.cumsum(rng.integers(0, 40, n)).astype(np.int64) + 5_000
    k = rng.integers(0, keys, n).astype(np.int32)
    v = values[rng.integers(0 if filtered else 1, len(values), n)]
    x = rng.integers(-10**6, 10**6, n).astype(np.int64)
    return ts, with_ord([k, v, x, None, ts.copy()], filtered)


def with_ord(cols, filtered=True):
    ok = cols[1] > FILTER[2] if filtered else np.ones(len(cols[1]), bool)
    cols[3] = (np.cumsum(ok) - 1).astype(np.int64)
    return cols


def make_spec(N, grouped, output, filtered=True, aggs=AGGS, keys=12, window="length", **kw):
    if window == "externalTime":
        kw["ts_attr"] = "ord"
    return abi.QuerySpec(SCHEMA, window, N, group_by=["k"] if grouped else (), aggs=aggs,
                         filter=FILTER if filtered else None, output=output, key_capacity=max(16, 2 * keys), **kw)


def cut_pushes(ts, cols, cuts, send_size, advance_after=None):
    """pushes cut at the stream indices `cuts`; advance_after: {push number: clock} — an ('advance', t) behind it"""
    from tests.parity import split_batches
    pushes = split_batches(SCHEMA, ts, cols, cuts, send_size)
    out = []
    for i, p in enumerate(pushes):
        out.append(p)
        if advance_after and i in advance_after:
            out.append(("advance", advance_after[i]))
    return out


def pass_cuts(cols, marks):
    """stream indices at which exactly `marks` (ascending counts) passing events lie before the cut"""
    ok = np.asarray(cols[1]) > FILTER[2]
    c = np.cumsum(ok)
    return [int(np.searchsorted(c, m, side="left")) + 1 for m in marks if m <= c[-1]]


# ---- the GPU matrix (tests/test_gpu_length.py; its coverage is asserted in tests/test_length_model.py) ------
# N edges: 1 expires the previous arrival every time; 63 / 64 / 65 and 2048 / 2049 straddle a wave and the scan
# tile; 5000 is larger than some pushes (a push expires only carried events); 10^6 is larger than the stream
N_EDGES = [1, 2, 63, 64, 65, 2048, 2049, 5000, 10**6]
GPU_EVENTS = 12_000
PASS_MARKS = [1, 2047, 2048, 2049, 4100, 9000]   # pushes are cut where this many passing events lie behind
DEAD_PUSH = (3000, 3005)                          # a push of events that all fail the filter
DAGGS = [("count", None), ("sum", "v"), ("min", "v"), ("max", "v"), ("avg", "v")]  # the wave replay's shape


def gpu_stream(keys, filtered, values=V_DEQUE, seed=7, n=GPU_EVENTS):
    ts, cols = stream(n, keys, seed, values, filtered)
    if filtered:
        cols[1] = cols[1].copy()
        cols[1][DEAD_PUSH[0]:DEAD_PUSH[1]] = -190.0
        with_ord(cols, True)
    return ts, cols


def gpu_pushes(ts, cols, send_size, filtered):
    """cuts at the PASS_MARKS, the dead push, and an ('advance', t) 3 s ahead behind the third push: no
    output, and the expired stamps / flush clocks of the next ~150 events stay at t"""
    cuts = set(pass_cuts(cols, PASS_MARKS) if filtered else PASS_MARKS)
    if filtered:
        cuts |= set(DEAD_PUSH)
    cuts = sorted(c for c in cuts if 0 < c < len(ts))
    return cut_pushes(ts, cols, cuts, send_size, {2: int(ts[cuts[2] - 1]) + 3_000})


def gpu_matrix():
    """(N, output, send size, keys, grouped, filtered): every N with every output and send size; the key
    counts (1 without and with group-by, 12, 200) and the filter rotate so that each meets every N, every
    output and every send size"""
    shapes = [(1, False), (1, True), (12, True), (200, True)]
    out = []
    for a, N in enumerate(N_EDGES):
        for b, output in enumerate(("current", "all", "expired")):
            for c, ss in enumerate((1, 7, 0)):
                keys, grouped = shapes[(a + b + c) % 4]
                out.append((N, output, ss, keys, grouped, (a + b + 2 * c) % 2 == 0))
    return out


_cache = {}


def gpu_case(N, output, ss, keys, grouped, filtered, aggs=None, values=None):
    """(spec, pushes, expected output, counters) of one matrix case; computed once per process"""
    key = (N, output, ss, keys, grouped, filtered, None if aggs is None else tuple(aggs), values)
    if key not in _cache:
        ts, cols = gpu_stream(keys, filtered, V_RESIDUE if values == "residue" else V_DEQUE)
        spec = make_spec(N, grouped, output, filtered, aggs=AGGS if aggs is None else aggs, keys=keys)
        pushes = gpu_pushes(ts, cols, ss, filtered)
        cnt = {}
        _cache[key] = (spec, pushes, run_model(spec, pushes, cnt), cnt)
    return _cache[key]


def load_kats():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_length.json")) as f:
        return json.load(f)["cases"]


def check_kat_extras(case, flushes):
    """the expectations tests/kat_runner.check_query does not know: row timestamps, types, flush clocks"""
    e = case["expect"]
    rows = [r for f in flushes for r in f.rows]
    if "row_ts" in e:
        assert [r[0] for r in rows] == e["row_ts"], [r[0] for r in rows]
    if "row_expired" in e:
        assert [r[1] for r in rows] == e["row_expired"], [r[1] for r in rows]
    if "flush_clocks" in e:
        assert [f.clock for f in flushes] == e["flush_clocks"], [f.clock for f in flushes]
