"""Every <sum, min, max> instantiation that a query can reach of the three double-column sliding replays,
bit-exact against the oracle: k_sl_wkey (time, current rows: the six shapes with a min or a max; the two
without one go to k_sl_own_d, so k_sl_wkey<*, 0, 0> is never launched), k_slx_wkey (time, `insert all
events`, all eight) and k_sl_own_d (externalTime, current rows, all eight). One small stream whose windows
hold ~270 events per key: more than one 64-record chunk, more than the 128 staged window heads and more
than the 64- / 32-entry LDS deque rings. By thirds its values are distinct (the parallel min / max), a
strictly descending ramp (the max deque holds the whole window and spills to its global ring, the min
deque has length 1) and the integers 0..5 (the deque quirk: sequential for the rest of the push)."""
import numpy as np
import pytest

from siddhi_amd import abi
from tests.parity import split_batches
from tests.test_gpu_sliding_expired import both, rt  # noqa: F401  (rt: the module's runtime fixture)

pytestmark = pytest.mark.gpu

SCHEMA = abi.Schema.parse("k int, v double, et long, ts long")
N, KEYS, T = 6_000, 3, 400
CUTS = [1_500, 1_501, 4_000]

AGG_SETS = {
    "none": [],
    "sum": ["sum"],
    "min": ["min"],
    "max": ["max"],
    "avg_min": ["avg", "min"],
    "sum_max": ["sum", "max"],
    "min_max": ["min", "max"],
    "sum_avg_min_max": ["sum", "avg", "min", "max"],
}
MODES = {  # window, output
    "time_current": ("time", "current"),
    "time_all": ("time", "all"),
    "external_current": ("externalTime", "current"),
}


def make_stream():
    rng = np.random.default_rng(0x51D)
    ts = 10_000 + np.arange(N, dtype=np.int64) // 2  # two events per ms
    k = rng.integers(0, KEYS, N).astype(np.int32)
    v = np.empty(N, dtype=np.float64)
    a, b = N // 3, 2 * N // 3
    v[:a] = rng.permutation(a) * 0.37 - 300.0
    v[a:b] = 5_000.0 - np.arange(b - a, dtype=np.float64)
    v[b:] = rng.integers(0, 6, N - b).astype(np.float64)
    return ts, [k, v, ts.copy(), ts.copy()]


TS, COLS = make_stream()


def run(rt, mode, aggs, send_size):
    window, output = MODES[mode]
    kw = {"ts_attr": "et"} if window == "externalTime" else {}
    spec = abi.QuerySpec(SCHEMA, window, T, group_by=["k"], output=output, key_capacity=8,
                         aggs=[("count", None)] + [(a, "v") for a in aggs], **kw)
    pushes = split_batches(SCHEMA, TS, COLS, CUTS, send_size)
    if output == "all":
        pushes.append(("advance", int(TS[-1]) + T + 1))  # the window drains: counts reach 0, nulls
    ref = both(rt, spec, pushes, f"{mode} {aggs} send {send_size}")
    assert ref["ts"].size > N // 3
    if output == "all":
        assert ref["expired"].sum() > 0
        assert ref["nulls"].any() == bool(aggs)


@pytest.mark.parametrize("aggs", list(AGG_SETS))
@pytest.mark.parametrize("mode", list(MODES))
def test_every_instantiation(rt, mode, aggs):
    run(rt, mode, AGG_SETS[aggs], 1)


def test_flagged_rows_of_the_keyed_replay(rt):
    """sends of 3 events: a (send, key) row is opened by the key's first record of the send and holds
    the values after its last (the flagged-rows path of k_sl_wkey)"""
    run(rt, "time_current", AGG_SETS["sum_avg_min_max"], 3)
