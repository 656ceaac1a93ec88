"""Expected output of lengthBatch(L, true) / timeBatch(T, true) with `having` and expired / all-events output.

As tests/having_model.py, every window behaviour comes from the frozen oracle and only the selector is
restated — here with the EXPIRED half of it (QuerySelector.processInBatchGroupBy,
core/query/selector/QuerySelector.java:315-374; processInBatchNoGroupBy :271-313):

  the chunks come from the spec's window run as a pass-through query (no group-by, no aggregators) with
  `insert all events`: each flush is one chunk, its rows the chunk's events with their stream index, timestamp
  (an EXPIRED copy carries the chunk's clock) and type. Both windows put RESET directly after the chunk's last
  EXPIRED event: lengthBatch(L, true) sends [EXPIRED copies of the batch, RESET, the event that starts the next
  batch] (LengthBatchWindowProcessor.java:245-274), timeBatch(T, true) sends [EXPIRED copies of the window,
  RESET] from the scheduler's TIMER, before the crossing send's own chunk of CURRENT events
  (TimeBatchWindowProcessor.java:262-340).

  Per event, in chunk order: a CURRENT event is added to its key's aggregators, an EXPIRED event removed from
  them (the Java remove forms, class KeyState), the row is formed from the event (timestamp, stream index,
  type, the values after the operation), `having` is evaluated on it — a null operand makes a comparison false
  (CompareConditionExpressionExecutor.java:38-42) — and if it passes and the event's type is switched on,
  grouped.put(key, row). The map is keyed by the group key alone: a key's CURRENT and EXPIRED rows of one
  chunk share one slot, at the position of the key's first passing event with the content of its last. A chunk
  that keeps nothing gives no flush. With `insert expired events` CURRENT events fold and are tested, never kept.

Only predicates whose Python comparison is exact are meaningful (tests/having_model.py).
"""
import dataclasses
import struct

import numpy as np

from oracle.oracle import OracleQuery
from siddhi_amd import abi
from tests import having_model as hm
from tests.parity import run_pushes

_FP = (abi.FLOAT, abi.DOUBLE)


def java_d2l(x):
    """(long) of a double (JLS 5.1.3)"""
    if x != x:
        return 0
    if x >= 9.2233720368547758e18:
        return 2**63 - 1
    if x <= -9.2233720368547758e18:
        return -2**63
    return int(x)


def _boxed_equal(a, b, fp):
    if not fp:
        return a == b
    if a != a and b != b:
        return True
    return struct.pack("<d", a) == struct.pack("<d", b)   # Double.equals: 0.0 != -0.0


class KeyState:
    """One key's aggregators with the Java add and remove forms (expired output: min / max track future
    states in a deque). counters: the deque statistics the coverage conditions read."""

    def __init__(self, spec, counters=None):
        self.spec = spec
        self.c = 0
        self.s = [None] * len(spec.aggs)           # sum / avg: the running value; min / max: the current value
        self.dq = [[] for _ in spec.aggs]
        self.counters = counters if counters is not None else {}

    def _col(self, a):
        ci = self.spec.schema.col(self.spec.aggs[a][1])
        return ci, self.spec.schema.types[ci] in _FP

    def add(self, ev):
        self.c += 1
        for a, (fn, col) in enumerate(self.spec.aggs):
            if fn == "count":
                continue
            ci, fp = self._col(a)
            x, s = ev[ci], self.s[a]
            if fn == "sum":
                self.s[a] = (0.0 if s is None else s) + float(x) if fp else hm._wrap64((0 if s is None else s) + int(x))
            elif fn == "avg":
                self.s[a] = (0.0 if s is None else s) + float(x)
            else:
                worse = (lambda cur: cur > x) if fn == "min" else (lambda cur: cur < x)
                d = self.dq[a]
                while d and worse(d[-1]):
                    d.pop()
                d.append(x)
                if s is None or worse(s):
                    self.s[a] = x

    def remove(self, ev):
        self.c -= 1
        for a, (fn, col) in enumerate(self.spec.aggs):
            if fn == "count":
                continue
            ci, fp = self._col(a)
            x, s = ev[ci], self.s[a]
            if fn == "sum":
                if fp:
                    self.s[a] = (0.0 if s is None else s) - float(x)
                else:   # sum = (long) ((double) sum - (double) v), SumAttributeAggregatorExecutor.java:283-291
                    self.s[a] = java_d2l(float(0 if s is None else s) - float(int(x)))
            elif fn == "avg":
                self.s[a] = (0.0 if s is None else s) - float(x)
            else:       # removeFirstOccurrence(value); the value is the deque's front, or null
                d = self.dq[a]
                for i, y in enumerate(d):
                    if _boxed_equal(y, x, fp):
                        if i > 0:
                            self.counters["non_front"] = self.counters.get("non_front", 0) + 1
                        del d[i]
                        break
                self.s[a] = d[0] if d else None

    def values(self):
        """the row's values, None for Java null"""
        out = []
        for a, (fn, col) in enumerate(self.spec.aggs):
            if fn == "count":
                out.append(self.c)
            elif fn in ("sum", "avg"):
                out.append(None if self.c == 0 else self.s[a] if fn == "sum" else self.s[a] / float(self.c))
            else:
                out.append(self.s[a])
        return out


def evaluate(expr, keys, vals):
    """tests/having_model.evaluate with Java null (None): a comparison with a null operand is false."""
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
    if a is None or b is None:
        return False
    return {">": a > b, ">=": a >= b, "<": a < b, "<=": a <= b, "==": a == b, "!=": a != b}[head]


def chunks(spec, pushes):
    """[(flush clock, [(stream index, timestamp, expired)] in chunk order)] from the oracle."""
    q = OracleQuery(dataclasses.replace(spec, aggs=(), having=None, rate=None, group_by=(), output="all"))
    A = run_pushes(q, pushes)
    q.close()
    out = []
    for f in range(len(A["flush_clock"])):
        lo, hi = int(A["flush_offsets"][f]), int(A["flush_offsets"][f + 1])
        out.append((int(A["flush_clock"][f]),
                    list(zip(A["rep"][lo:hi].tolist(), A["ts"][lo:hi].tolist(), A["expired"][lo:hi].tolist()))))
    return out


def run_model(spec, pushes, having="spec", chunk_list=None, counters=None):
    """out_arrays-shaped expected output of `spec` (its `having`, or the one given; None = no having).
    counters (a dict) receives the coverage counts of tests/test_having_expired_model.py."""
    if having == "spec":
        having = spec.having
    cnt = counters if counters is not None else {}
    for k in ("kept_not_last_removal", "pass_then_fail", "key_without_row", "chunk_without_row", "null_in_row",
              "non_front", "current_replaces_expired", "current_follows_expired"):
        cnt.setdefault(k, 0)
    cur_on, exp_on = spec.output in ("current", "all"), spec.output in ("expired", "all")
    cols = hm._events(spec, pushes)
    gcols = [spec.schema.col(g) for g in spec.group_by]
    vt = hm.val_types(spec)
    na, nk = len(spec.aggs), len(gcols)
    state = {}
    fo, fc, ts, rep, exp, keys, vals = [0], [], [], [], [], [], []
    for clock, evs in (chunk_list if chunk_list is not None else chunks(spec, pushes)):
        last_exp = max((i for i, e in enumerate(evs) if e[2]), default=-1)
        grouped = {}
        removals = {}     # key -> [passed?] per removal of this chunk, in order
        for i, (e, t, x) in enumerate(evs):
            ev = [c[e] for c in cols]
            key = tuple(int(ev[g]) for g in gcols)
            st = state.get(key)
            if st is None:
                st = state[key] = KeyState(spec, cnt)
            if x:
                st.remove(ev)
            else:
                st.add(ev)
            v = st.values()
            ok = having is None or evaluate(having, key, v)
            if x:
                removals.setdefault(key, []).append(ok)
            if ok and (exp_on if x else cur_on):
                if not x and key in grouped:
                    cnt["current_replaces_expired"] += bool(grouped[key][2])
                elif not x and grouped:
                    cnt["current_follows_expired"] += 1
                grouped[key] = (t, e, int(bool(x)), v)
            if i == last_exp:
                state.clear()   # RESET
        if exp_on and removals:
            for key, oks in removals.items():
                if any(oks) and not oks[-1]:
                    cnt["kept_not_last_removal"] += 1
                if any(a and not b for a, b in zip(oks, oks[1:])):
                    cnt["pass_then_fail"] += 1
            none = [k for k in removals if k not in grouped]
            if grouped and none:
                cnt["key_without_row"] += len(none)
            if not grouped:
                cnt["chunk_without_row"] += 1
        if not grouped:
            continue
        for key, (t, e, x, v) in grouped.items():
            ts.append(t); rep.append(e); exp.append(x); keys.append(key); vals.append(v)
            cnt["null_in_row"] += any(y is None for y in v)
        fo.append(len(ts))
        fc.append(clock)
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


# ---- the cases tests/test_having_expired_model.py and tests/test_gpu_having_expired.py share ---------------
SCHEMA, AGGS, FILTER, CUTS = hm.SCHEMA, hm.AGGS, hm.FILTER, hm.CUTS
# few values, so that duplicates abound in a key's deque (-190 fails the filter)
V_VALUES = np.array([-190.0, -7.5, -2.0, 0.0, 1.5, 3.0, 8.25])

WINDOWS = {
    "lengthBatch37": ("lengthBatch", 37, {}),
    "lengthBatch1": ("lengthBatch", 1, {}),
    "timeBatch700": ("timeBatch", 700, {}),
    "timeBatch333s": ("timeBatch", 333, {"start_time": 100}),
}
# aggregates: 0 count, 1 sum(v), 2 min(v), 3 max(x), 4 avg(x), 5 sum(x)
PREDICATES = {
    "count==2": ("==", ("agg", 0), ("long", 2)),
    "count==0": ("==", ("agg", 0), ("long", 0)),
    "minv<0": ("<", ("agg", 2), 0.0),
    "not(minv<0)": ("not", ("<", ("agg", 2), 0.0)),
    "sumv>2|count==1": ("or", (">", ("agg", 1), 2.0), ("==", ("agg", 0), 1)),
}


def stream(n=4000, keys=12, seed=3):
    """tests/having_model.stream with v re-drawn from V_VALUES"""
    ts, cols = hm.stream(n, keys, seed)
    rng = np.random.default_rng(seed + 1000)
    cols[1] = V_VALUES[rng.integers(0, len(V_VALUES), n)]
    return ts, cols


make_pushes = hm.make_pushes


def make_spec(family, grouped, output, having=None, keys=12, aggs=AGGS, **kw):
    window, param, extra = WINDOWS[family]
    return abi.QuerySpec(SCHEMA, window, param, group_by=["k"] if grouped else (), aggs=aggs, filter=FILTER,
                         stream_current=True, output=output, key_capacity=max(16, 2 * keys), having=having,
                         **extra, **kw)


def matrix():
    """(family, grouped, output, send size, predicate name) of the GPU matrix"""
    return [(fam, grouped, output, ss, pn) for fam in WINDOWS for grouped in (True, False)
            for output in ("all", "expired") for ss in (1, 13, 0) for pn in PREDICATES]
