"""sh_having_check's verdicts for expired / all-events output (no context, no GPU): the two
stream.current.event batch windows run it, every other shape stays SH_ERR_UNSUPPORTED by name."""
import ctypes as C

import pytest

from siddhi_amd import abi

SCHEMA = abi.Schema.parse("k int, v double, x long, g long")
AGGS = [("count", None), ("sum", "v"), ("min", "x"), ("max", "v")]
COUNT2 = ("==", ("agg", 0), ("long", 2))
NOT_MIN = ("not", ("<", ("agg", 2), 0))


def check(sp, expr):
    from siddhi_amd import runtime
    L = runtime.lib()
    d = sp.desc()
    ops = abi.compile_having(sp, expr)
    arr = (abi.FilterOp * len(ops))(*ops)
    rc = L.sh_having_check(C.byref(d), arr, len(ops))
    return rc, (L.sh_last_error().decode() if rc else "")


def spec(window, output, grouped=True, **kw):
    return abi.QuerySpec(SCHEMA, window, 1000, group_by=["k"] if grouped else [], aggs=AGGS, key_capacity=64,
                         output=output, **kw)


@pytest.mark.parametrize("expr", [COUNT2, NOT_MIN], ids=["count==2", "not(min<0)"])
@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("output", ["all", "expired"])
@pytest.mark.parametrize("window", ["timeBatch", "lengthBatch"])
def test_accepts_the_stream_current_forms(window, output, grouped, expr):
    assert check(spec(window, output, grouped, stream_current=True), expr) == (abi.SH_OK, "")


@pytest.mark.parametrize("output", ["all", "expired"])
@pytest.mark.parametrize("window,kw", [("externalTimeBatch", {"ts_attr": "g"}), ("timeBatch", {}), ("lengthBatch", {})])
def test_plain_batch_windows_stay_refused_by_name(window, kw, output):
    rc, msg = check(spec(window, output, **kw), COUNT2)
    assert rc == abi.SH_ERR_UNSUPPORTED and "expired" in msg, (rc, msg)
    assert "lengthBatch(L, true)" in msg and "timeBatch(T, true)" in msg   # (says which forms do run)


def test_runtime_having_check_follows():
    from siddhi_amd import runtime
    runtime.having_check(spec("timeBatch", "all", stream_current=True, having=COUNT2))
    with pytest.raises(runtime.SiddhiError) as e:
        runtime.having_check(spec("timeBatch", "all", having=COUNT2))
    assert e.value.code == abi.SH_ERR_UNSUPPORTED
