"""The Python restatement of the sliding length(N) window (tests/length_model.py) — the expected output of
tests/test_gpu_length.py — checked without a GPU:

  (1) the transcribed and hand-traced KATs of tests/golden/kat_length.json;
  (2) against the frozen oracle by an independent route: a length window is the sliding window whose clock
      is the count of passing events, so the oracle's externalTime(ord, N) over a column `ord` holding each
      passing event's ordinal must agree bit for bit in everything but the timestamp of EXPIRED rows
      (externalTime stamps the attribute of the expiring event, length stamps the send's playback clock);
  (3) the coverage of the streams the GPU tests use, so that none of them passes vacuously.
"""
import dataclasses

import numpy as np
import pytest

from oracle.oracle import OracleQuery
from tests import kat_runner
from tests import length_model as lm
from tests.parity import assert_same, run_pushes

KATS = lm.load_kats()


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_kat_through_the_model(case):
    schema, spec, dic, flushes = kat_runner.run_query(case, lm.ModelQuery)
    kat_runner.check_query(case, flushes, schema, dic)
    lm.check_kat_extras(case, flushes)


def test_kat_file_holds_the_cases():
    names = [c["name"] for c in KATS]
    assert names[:3] == ["lengthWindowTest1", "lengthWindowTest2", "lengthWindowTest3"]
    assert all(c["source"] for c in KATS) and len(names) >= 5


# ---- (2) model == oracle externalTime(ord, N) ----------------------------------------------------------------
def _cross(N, grouped, output, ss, values):
    ts, cols = lm.stream(4_000, 12, 3, values)
    pushes = lm.cut_pushes(ts, cols, [1, 777, 2499, 2500, 3300], ss, {2: int(ts[2498]) + 1_500})
    spec = lm.make_spec(N, grouped, output)
    cnt = {}
    got = lm.run_model(spec, pushes, cnt)
    o = OracleQuery(dataclasses.replace(spec, window="externalTime", ts_attr="ord"))
    ref = run_pushes(o, pushes)
    o.close()
    label = f"length({N}) grouped={grouped} {output} send {ss}"
    # EXPIRED rows: the model stamps the send's clock = the flush clock of the row's flush
    x = got["expired"] == 1
    assert np.array_equal(got["expired"], ref["expired"]), label
    flush_of = np.repeat(np.arange(len(got["flush_clock"])), np.diff(got["flush_offsets"]))
    assert np.array_equal(got["ts"][x], got["flush_clock"][flush_of[x]]), label
    ref = dict(ref)
    ref["ts"] = np.where(x, got["ts"], ref["ts"])
    assert_same(got, ref, label=label)
    return cnt


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("N", [1, 2, 7, 64, 1000])
def test_model_equals_oracle_external_time_over_ordinals(N, grouped):
    """N x grouped x current / all / expired x send size 1 / 13 / 0 x the two value sets: 180 combinations"""
    tot = {}
    for output in ("current", "all", "expired"):
        for ss in (1, 13, 0):
            for values in (lm.V_DEQUE, lm.V_RESIDUE):
                for k, v in _cross(N, grouped, output, ss, values).items():
                    tot[k] = tot.get(k, 0) + v
    assert tot["expired_rows"] > 0
    if N == 1 or (grouped and N <= 7):
        assert tot["null_in_row"] > 0    # a count reached 0 in an expired row
    if grouped and N in (2, 7):
        assert tot["residue_kept"] > 0   # a double sum's residue kept a count-0 state alive (V_RESIDUE)


# ---- (3) the GPU streams cover what the GPU tests are there for ----------------------------------------------
def test_gpu_matrix_shape():
    m = lm.gpu_matrix()
    assert len(m) == 81 and len(set(m)) == 81
    for N in lm.N_EDGES:
        mine = [c for c in m if c[0] == N]
        assert {c[1] for c in mine} == {"current", "all", "expired"} and {c[2] for c in mine} == {1, 7, 0}
        assert {c[5] for c in mine} == {True, False} and len({(c[3], c[4]) for c in mine}) >= 3
    for keys, grouped in ((1, False), (1, True), (12, True), (200, True)):
        mine = [c for c in m if (c[3], c[4]) == (keys, grouped)]
        assert {c[1] for c in mine} == {"current", "all", "expired"} and {c[2] for c in mine} == {1, 7, 0}
        assert {c[5] for c in mine} == {True, False}


def test_gpu_streams_cover_the_cases():
    # expired rows, nulls (a key's count reaches 0 in an expired row), the deque quirk, a dead push
    spec, pushes, out, cnt = lm.gpu_case(2, "all", 7, 12, True, True)
    assert cnt["expired_rows"] > 0 and out["expired"].sum() == cnt["expired_rows"]
    assert cnt["null_in_row"] > 0 and out["nulls"].any()
    assert cnt["current_replaces_expired"] > 0      # send size > 1, all events
    assert cnt["push_without_pass"] == 1
    spec, pushes, out, cnt = lm.gpu_case(64, "expired", 1, 12, True, True)
    assert cnt["non_front"] > 0                     # removeFirstOccurrence hit a non-front element
    assert cnt["expired_rows"] > 0
    # every filtered case has its dead push and the advance between pushes
    assert sum(isinstance(p, tuple) for p in pushes) == 1
    # N = 5000: at least one push smaller than the window expires events (only carried ones can leave)
    spec, pushes, out, cnt = lm.gpu_case(5000, "expired", 0, 12, True, False)
    sizes = [len(p.ts) for p in pushes if not isinstance(p, tuple)]
    assert cnt["expired_rows"] > 0 and min(sizes[-2:]) < 5000 < sum(sizes)
    # N = 10^6: nothing ever expires, so expired output has no flush at all
    spec, pushes, out, cnt = lm.gpu_case(10**6, "expired", 7, 12, True, True)
    assert len(out["flush_clock"]) == 0 and len(out["ts"]) == 0
    # the pushes are cut where 1, 2047, 2048 and 2049 passing events lie behind
    spec, pushes, out, cnt = lm.gpu_case(2048, "all", 1, 12, True, True)
    passed, seen = 0, []
    for p in pushes:
        if not isinstance(p, tuple):
            passed += int((p.cols[1] > lm.FILTER[2]).sum())
            seen.append(passed)
    assert {1, 2047, 2048, 2049} <= set(seen)
    # the residue value set leaves count-0 states alive (canDestroy is false) and destroys others
    spec, pushes, out, cnt = lm.gpu_case(2, "all", 1, 12, True, True, values="residue")
    assert cnt["residue_kept"] > 0 and cnt["destroyed"] > 0
