"""The `having` entry points at the drop-in boundary: the header, the Python mirror and the built library
carry sh_query_set_having and sh_having_check, and sh_having_check (no context, no GPU) gives the accept /
SH_ERR_INVALID / SH_ERR_UNSUPPORTED verdicts the header documents."""
import ctypes as C
import os
import re
import subprocess

import pytest

from siddhi_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "siddhi_hip.h")
LIB = os.path.join(ROOT, "siddhi_amd", "libsiddhi_hip.so")
SYMS = ["sh_query_set_having", "sh_having_check"]

SCHEMA = abi.Schema.parse("k int, v double, x long, s string, b bool, g long, f float")
AGGS = [("count", None), ("sum", "v"), ("min", "x"), ("max", "f")]


def test_symbols_in_header_mirror_and_library():
    txt = open(HDR).read()
    declared = set(re.findall(r"^\s*int\s+(sh_\w+)\s*\(", txt, re.M))
    for s in SYMS:
        assert s in declared and s in abi.ABI_SYMBOLS
    assert re.search(r"#define SH_OP_KEY 12\b", txt) and re.search(r"#define SH_OP_AGG 13\b", txt)
    assert (abi.OP_KEY, abi.OP_AGG) == (12, 13)
    assert "#define SH_ABI_VERSION 16" in txt
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert all(s in exported for s in SYMS)


def spec(window="timeBatch", group_by=("k",), aggs=AGGS, **kw):
    return abi.QuerySpec(SCHEMA, window, 1000, group_by=list(group_by), aggs=list(aggs), key_capacity=64, **kw)


def check(sp, expr=None, ops=None):
    """(return code, message) of sh_having_check"""
    from siddhi_amd import runtime
    L = runtime.lib()
    d = sp.desc()
    if ops is None:
        ops = abi.compile_having(sp, expr)
    arr = (abi.FilterOp * max(1, len(ops)))(*ops)
    rc = L.sh_having_check(C.byref(d), arr, len(ops))
    return rc, (L.sh_last_error().decode() if rc else "")


COUNT2 = ("==", ("agg", 0), ("long", 2))

ACCEPT = [
    (spec(), COUNT2),
    (spec("lengthBatch"), (">=", ("agg", 1), 1.5)),
    (spec("externalTimeBatch", ts_attr="g"), ("<", ("agg", 2), 7)),
    (spec(stream_current=True), ("and", ("<=", ("agg", 0), 3), (">", ("agg", 1), -100.0))),
    (spec("lengthBatch", stream_current=True), ("or", COUNT2, ("not", ("==", ("key", 0), 3)))),
    (spec(group_by=()), COUNT2),
    (spec(group_by=("s",)), ("!=", ("key", 0), ("string", 4))),
    (spec(group_by=("b",)), ("and", ("key", 0), COUNT2)),
    (spec(group_by=("k", "f")), (">", ("key", 1), ("float", 0.5))),
    (spec(), (">", ("agg", 3), ("agg", 1))),
]


@pytest.mark.parametrize("i", range(len(ACCEPT)))
def test_accepts(i):
    sp, expr = ACCEPT[i]
    assert check(sp, expr) == (abi.SH_OK, "")


def _op(op, **kw):
    return abi.FilterOp(op=op, **kw)


AGG0, K0 = _op(abi.OP_AGG, col=0), _op(abi.OP_KEY, col=0)
LONG2 = _op(abi.OP_CONST, type=abi.LONG, ival=2)
INVALID = [
    ("underflow", spec(), [AGG0, _op(abi.OP_EQ)]),
    ("left on the stack", spec(), [AGG0, LONG2, _op(abi.OP_EQ), AGG0]),
    ("aggregate out of range", spec(), [_op(abi.OP_AGG, col=4), LONG2, _op(abi.OP_EQ)]),
    ("key out of range", spec(), [_op(abi.OP_KEY, col=1), LONG2, _op(abi.OP_EQ)]),
    ("key without group-by", spec(group_by=()), [K0, LONG2, _op(abi.OP_EQ)]),
    ("result not boolean", spec(), [AGG0]),
    ("boolean fed to a comparison", spec(), [AGG0, LONG2, _op(abi.OP_EQ), LONG2, _op(abi.OP_GT)]),
    ("relational on a string id", spec(group_by=("s",)), [K0, _op(abi.OP_CONST, type=abi.STRID, ival=1), _op(abi.OP_LT)]),
    ("relational on a bool", spec(group_by=("b",)), [K0, _op(abi.OP_CONST, type=abi.BOOL, ival=1), _op(abi.OP_GE)]),
    ("more than 32 ops", spec(), [AGG0, LONG2, _op(abi.OP_EQ)] + [_op(abi.OP_NOT)] * 30),
    ("empty", spec(), []),
    ("and of a number", spec(), [AGG0, LONG2, _op(abi.OP_AND)]),
    ("unknown opcode", spec(), [AGG0, LONG2, _op(99)]),
]


@pytest.mark.parametrize("i", range(len(INVALID)))
def test_invalid(i):
    _, sp, ops = INVALID[i]
    rc, msg = check(sp, ops=ops)
    assert rc == abi.SH_ERR_INVALID and msg


UNSUPPORTED = [
    (spec(None), COUNT2, "window"),
    (spec("time"), COUNT2, "sliding time"),
    (spec("externalTime", ts_attr="g"), COUNT2, "externalTime"),
    (spec(output="all"), COUNT2, "expired"),
    (spec(output="expired"), COUNT2, "expired"),
    (spec(partition="k"), COUNT2, "partition"),
    (spec(group_by=("k", "g")), COUNT2, "wide"),
    (spec(group_by=("k", "s", "b")), COUNT2, "wide"),
    (spec(group_by=(), aggs=()), ("==", 1, 1), "aggregator"),
    (spec(), (">", "x", 3), "stream attribute"),
]


@pytest.mark.parametrize("i", range(len(UNSUPPORTED)))
def test_unsupported_names_the_shape(i):
    sp, expr, word = UNSUPPORTED[i]
    rc, msg = check(sp, expr)
    assert rc == abi.SH_ERR_UNSUPPORTED and word in msg, (rc, msg)


def test_runtime_having_check_raises():
    from siddhi_amd import runtime
    runtime.having_check(spec(having=COUNT2))
    with pytest.raises(runtime.SiddhiError) as e:
        runtime.having_check(spec("time", having=COUNT2))
    assert e.value.code == abi.SH_ERR_UNSUPPORTED
