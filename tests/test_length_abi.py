"""The sliding length(N) window at the drop-in boundary (no GPU): the header and the Python mirror name it
without an ABI bump, and sh_having_check refuses `having` on it by name."""
import ctypes as C
import os
import re

from siddhi_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "siddhi_hip.h")
SCHEMA = abi.Schema.parse("k int, v double, x long")


def test_header_and_mirror_define_the_window():
    txt = open(HDR).read()
    assert re.search(r"#define SH_WIN_LENGTH 6\b", txt)
    assert "LengthWindowProcessor.java" in txt
    assert "#define SH_ABI_VERSION 16" in txt
    assert abi.WIN_LENGTH == 6
    d = abi.QuerySpec(SCHEMA, "length", 1000, group_by=["k"], aggs=[("avg", "v")]).desc()
    assert d.window == 6 and d.window_param == 1000


def test_having_check_refuses_a_length_window_by_name():
    from siddhi_amd import runtime
    L = runtime.lib()
    sp = abi.QuerySpec(SCHEMA, "length", 100, group_by=["k"], aggs=[("count", None), ("sum", "v")], key_capacity=64)
    ops = abi.compile_having(sp, ("==", ("agg", 0), ("long", 2)))
    arr = (abi.FilterOp * len(ops))(*ops)
    d = sp.desc()
    rc = L.sh_having_check(C.byref(d), arr, len(ops))
    assert rc == abi.SH_ERR_UNSUPPORTED
    assert "a sliding length window" in L.sh_last_error().decode()
