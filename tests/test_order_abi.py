"""The `order by` / `limit` / `offset` entry points at the drop-in boundary: the header, the Python mirror and the
built library carry sh_query_set_order and sh_order_check, and sh_order_check (no context, no GPU) gives the
accept / SH_ERR_INVALID / SH_ERR_UNSUPPORTED verdicts the header documents. Nothing here skips: a library
without the symbols fails these tests."""
import ctypes as C
import os
import re
import subprocess

import pytest

from siddhi_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "siddhi_hip.h")
LIB = os.path.join(ROOT, "siddhi_amd", "libsiddhi_hip.so")
SYMS = ["sh_query_set_order", "sh_order_check"]

SCHEMA = abi.Schema.parse("k int, v double, x long, s string, b bool, g long, f float")
AGGS = [("count", None), ("sum", "v"), ("min", "x"), ("max", "f")]


def test_symbols_in_header_mirror_and_library():
    txt = open(HDR).read()
    declared = set(re.findall(r"^\s*int\s+(sh_\w+)\s*\(", txt, re.M))
    for s in SYMS:
        assert s in declared and s in abi.ABI_SYMBOLS
    assert re.search(r"#define SH_ORD_KEY 0\b", txt) and re.search(r"#define SH_ORD_AGG 1\b", txt)
    assert (abi.ORD_KEY, abi.ORD_AGG) == (0, 1)
    assert "#define SH_ABI_VERSION 16" in txt
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert all(s in exported for s in SYMS)


def test_struct_layout_matches_c(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "siddhi_hip.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(sh_order_term), offsetof(sh_order_term, index),'
                   ' offsetof(sh_order_term, desc), offsetof(sh_order_term, pad));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    T = abi.OrderTerm
    assert got == [C.sizeof(T), T.index.offset, T.desc.offset, T.pad.offset] == [16, 4, 8, 12]


def test_compile_order():
    t = abi.compile_order([("agg", 1, "desc"), ("key", 0, "asc"), ("agg", 2)])
    assert [(x.kind, x.index, x.desc) for x in t] == [(1, 1, 1), (0, 0, 0), (1, 2, 0)]
    assert abi.compile_order(None) == []
    with pytest.raises(ValueError):
        abi.compile_order([("col", 0)])
    with pytest.raises(ValueError):
        abi.compile_order([("agg", 0, "down")])


def spec(window="timeBatch", group_by=("k",), aggs=AGGS, **kw):
    return abi.QuerySpec(SCHEMA, window, 1000, group_by=list(group_by), aggs=list(aggs), key_capacity=64, **kw)


def check(sp, order_by=None, limit=None, offset=None, terms=None):
    """(return code, message) of sh_order_check"""
    from siddhi_amd import runtime
    L = runtime.lib()
    d = sp.desc()
    if terms is None:
        terms = abi.compile_order(order_by)
    arr = (abi.OrderTerm * max(1, len(terms)))(*terms)
    rc = L.sh_order_check(C.byref(d), arr, len(terms), -1 if limit is None else limit, -1 if offset is None else offset)
    return rc, (L.sh_last_error().decode() if rc else "")


SUM_DESC = [("agg", 1, "desc")]

ACCEPT = [
    (spec(), SUM_DESC, 10, None),
    (spec(), None, 0, None),
    (spec(), None, None, 3),
    (spec(), [("agg", 0), ("agg", 1, "desc"), ("agg", 2), ("key", 0, "desc")], None, None),
    (spec("lengthBatch"), SUM_DESC, 1, 1),
    (spec("externalTimeBatch", ts_attr="g"), [("agg", 3)], None, 0),
    (spec(stream_current=True, output="all"), SUM_DESC, 2, None),
    (spec("lengthBatch", stream_current=True, output="expired"), [("agg", 2, "desc")], None, None),
    (spec("time", output="all"), SUM_DESC, 1, None),
    (spec("externalTime", ts_attr="g", output="expired"), [("key", 0)], None, None),
    (spec("length"), SUM_DESC, 5, 2),
    (spec(output="expired"), SUM_DESC, None, None),
    (spec(group_by=()), None, 1, 0),                        # a no-group-by aggregate: limit / offset alone decide
    (spec(group_by=()), [("agg", 0)], None, None),          # ... its terms are accepted (there is one row to order)
    (spec(group_by=(), aggs=()), None, 2, 1),               # a pass-through query: limit and offset alone
    (spec(group_by=("b",)), [("key", 0, "desc")], None, None),
    (spec(group_by=("f",)), [("key", 0)], None, None),
    (spec(group_by=("k", "f")), [("key", 1), ("key", 0)], None, None),
    (spec(group_by=("s",)), [("agg", 0, "desc")], 3, None),  # a string key that is not a term
    (spec(having=(">", ("agg", 0), 1)), SUM_DESC, 1, None),
    (spec(rate=("all", 4)), SUM_DESC, 1, None),
]


@pytest.mark.parametrize("i", range(len(ACCEPT)))
def test_accepts(i):
    sp, order_by, limit, offset = ACCEPT[i]
    assert check(sp, order_by, limit, offset) == (abi.SH_OK, "")


def _t(kind, index, desc=0):
    return abi.OrderTerm(kind=kind, index=index, desc=desc)


INVALID = [
    ("aggregate out of range", spec(), [_t(abi.ORD_AGG, 4)], -1, -1),
    ("aggregate below range", spec(), [_t(abi.ORD_AGG, -1)], -1, -1),
    ("key out of range", spec(), [_t(abi.ORD_KEY, 1)], -1, -1),
    ("key without group-by", spec(group_by=()), [_t(abi.ORD_KEY, 0)], -1, -1),
    ("unknown kind", spec(), [_t(2, 0)], -1, -1),
    ("more than 4 terms", spec(), [_t(abi.ORD_AGG, 0)] * 5, -1, -1),
    ("negative term count", spec(), None, -1, -1),
    ("limit below -1 (limitTest18)", spec(), [_t(abi.ORD_AGG, 0)], -2, 0),
    ("offset below -1 (limitTest19)", spec(), [_t(abi.ORD_AGG, 0)], 1, -2),
    ("nothing to do", spec(), [], -1, -1),
]


@pytest.mark.parametrize("i", range(len(INVALID)))
def test_invalid(i):
    from siddhi_amd import runtime
    _, sp, terms, limit, offset = INVALID[i]
    if terms is None:
        L = runtime.lib()
        d = sp.desc()
        rc = L.sh_order_check(C.byref(d), None, -1, limit, offset)
        msg = L.sh_last_error().decode()
    else:
        rc, msg = check(sp, terms=terms, limit=limit, offset=offset)
    assert rc == abi.SH_ERR_INVALID and msg


UNSUPPORTED = [
    (spec(group_by=("s",)), [("key", 0)], None, "string"),
    (spec(group_by=("k", "s")), [("key", 1, "desc")], 1, "string"),  # (two 32-bit columns: not interned)
    (spec(group_by=(), aggs=()), [("agg", 0)], None, "pass-through"),
    (spec(group_by=(), aggs=()), [("key", 0)], 3, "pass-through"),
    (spec(partition="k"), SUM_DESC, 1, "partition"),
    (spec("lengthBatch", partition="g", group_by=("k",)), None, 1, "partition"),
    (spec(group_by=("k", "g")), SUM_DESC, None, "wide"),
    (spec(group_by=("k", "s", "b")), None, 10, "wide"),
    (spec(None), SUM_DESC, 1, "window"),
]


@pytest.mark.parametrize("i", range(len(UNSUPPORTED)))
def test_unsupported_names_the_shape(i):
    sp, order_by, limit, word = UNSUPPORTED[i]
    rc, msg = check(sp, order_by, limit)
    assert rc == abi.SH_ERR_UNSUPPORTED and word in msg, (rc, msg)


def test_runtime_order_check_raises():
    from siddhi_amd import runtime
    runtime.order_check(spec(order_by=SUM_DESC, limit=10))
    runtime.order_check(spec(), order_by=SUM_DESC, limit=None, offset=1)
    with pytest.raises(runtime.SiddhiError) as e:
        runtime.order_check(spec(partition="k", order_by=SUM_DESC))
    assert e.value.code == abi.SH_ERR_UNSUPPORTED
    with pytest.raises(runtime.SiddhiError) as e:
        runtime.order_check(spec(limit=-3))
    assert e.value.code == abi.SH_ERR_INVALID


def test_spec_mirror_fields():
    sp = spec(order_by=SUM_DESC, limit=10, offset=None)
    assert sp.has_order() and not spec().has_order() and spec(offset=0).has_order()
    # the descriptor is unchanged by the order fields (no struct changed)
    a, b = sp.desc(), spec().desc()
    skip = C.sizeof(C.c_void_p)
    off = abi.QueryDesc.filter.offset
    ba, bb = bytes(a), bytes(b)
    assert ba[:off] == bb[:off] and ba[off + skip:] == bb[off + skip:]
