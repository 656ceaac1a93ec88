"""The multisplit fold's order check ("optimistic fold"): k_aggregate_own folds a unit without
step (e), the owner verifying its list's order on the way, and runs a unit that fails again in checked form.
SH_FOLD_CHECK=1 checks every unit at once (the form before); SH_FOLD_CHECK=2 folds optimistically and runs
every odd unit again, which exercises the second pass on hardware whose LDS atomics never ask for it.

Every case is one of tests/test_gpu_fold_chain.py (3,000 keys, P = 8, pushes of 300,001 or 262,144 events),
computed once on the oracle (shared with that module) and compared bit for bit (tests/parity.py, no
tolerance) with GPU runs under SH_FOLD_CHECK unset, 1 and 2 on fresh queries (the switch is read when a query
is created). The three runs give one output digest and the same query statistics (events, and the fold's
algorithmic bytes, which count the rows the host takes per segment).

  one_chunk      96 units per push, one chunk each: the base path; the first push starts at combined index 0,
                 pushes 2 and 3 start with pending events; also with host output, where the host reads
                 the rows per unit and the fold counts them
  four_chunks    four chunks per unit: the entry before a chunk's first one is the last of the chunk before;
                 a second pass that reads several chunks again
  many_units     about 700 units per push, more than the grid: a second pass followed by the next unit's
                 prefetch, and a workgroup's last unit run twice
  empty_units    a window with 7 of 8 units empty: an empty unit run twice, and an empty unit right behind a
                 unit that ran twice
  hashed         K = 2 (two keys per owner, one list; these instantiations take the checked form in every mode,
                 so the three runs show the switch leaves them alone); hashed_sparse: with windows of a
                 single key
  two_columns    lengthBatch, R = 4, one workgroup per unit; four_columns: R = 2, the table-driven fold
  all            output="all" (host output: the rows per unit are read by the host, so the fold counts them)
  SH_FOLD_GRID=0 one workgroup per unit, on one_chunk and many_units

Every multisplit unit leaves dense rows (run_closed), so no query shape reaches the kernel's non-dense row
path and none is covered here.
"""
import pytest

from siddhi_amd import abi, digest
from tests import test_gpu_fold_chain as fc
from tests.parity import assert_same, run_pushes

pytestmark = pytest.mark.gpu

MODES = (None, "1", "2")


@pytest.fixture(scope="module")
def rt():
    from siddhi_amd import runtime
    return runtime


def run_device(rt, spec, pushes):
    """The benchmark's path (batches in HBM, rows left in HBM); the output and the query's statistics."""
    import torch
    dev = torch.device("cuda", 0)
    g = rt.GpuQuery(spec)
    parts = []
    for p in pushes:
        ts = torch.from_numpy(p.ts).to(dev)
        cols = [torch.from_numpy(c).to(dev) for c in p.cols]
        torch.cuda.synchronize()
        out = g.push_device(len(p.ts), ts.data_ptr(), [c.data_ptr() for c in cols], p.b.send_size)
        torch.cuda.synchronize()
        parts.append(rt.device_out_arrays(out))
        del ts, cols
    s = g.stats()
    g.close()
    return abi.concat_arrays(parts), (s.events, s.main_kernel_bytes)


def run_host(rt, spec, pushes):
    g = rt.GpuQuery(spec)
    out = run_pushes(g, pushes)
    s = g.stats()
    g.close()
    return out, (s.events, s.main_kernel_bytes)


def check_modes(rt, monkeypatch, case, run=run_device, min_flushes=1):
    spec, pushes = fc.CASES[case]()
    want = fc.want_of(case, min_flushes)
    digests, stats = set(), set()
    for mode in MODES:
        if mode is None:
            monkeypatch.delenv("SH_FOLD_CHECK", raising=False)
        else:
            monkeypatch.setenv("SH_FOLD_CHECK", mode)
        out, st = run(rt, spec, pushes)
        assert_same(out, want, label=f"{case}, SH_FOLD_CHECK={mode}")
        digests.add(digest.output_digest(out))
        stats.add(st)
    monkeypatch.delenv("SH_FOLD_CHECK", raising=False)
    assert len(digests) == 1
    assert len(stats) == 1, stats


def test_one_chunk_per_unit(rt, monkeypatch):
    check_modes(rt, monkeypatch, "one_chunk")


def test_one_chunk_per_unit_host_output(rt, monkeypatch):
    check_modes(rt, monkeypatch, "one_chunk", run=run_host)


def test_four_chunks_per_unit(rt, monkeypatch):
    check_modes(rt, monkeypatch, "four_chunks")


def test_more_units_than_the_grid(rt, monkeypatch):
    check_modes(rt, monkeypatch, "many_units", min_flushes=80)


def test_empty_units(rt, monkeypatch):
    check_modes(rt, monkeypatch, "empty_units")


def test_hashed_keys_two_per_owner(rt, monkeypatch):
    check_modes(rt, monkeypatch, "hashed")


def test_hashed_keys_single_key_windows(rt, monkeypatch):
    check_modes(rt, monkeypatch, "hashed_sparse", min_flushes=80)


def test_two_value_columns(rt, monkeypatch):
    check_modes(rt, monkeypatch, "two_columns", min_flushes=250)


def test_four_value_columns(rt, monkeypatch):
    check_modes(rt, monkeypatch, "four_columns")


def test_all_events_output(rt, monkeypatch):
    check_modes(rt, monkeypatch, "all", run=run_host)


TRACE_CHILD = """
import os
from siddhi_amd import runtime
from tests import test_gpu_fold_chain as fc
from tests.parity import run_pushes
spec, pushes = fc.CASES["one_chunk"]()
for mode in (None, "1", "2"):
    os.environ.pop("SH_FOLD_CHECK", None)
    if mode:
        os.environ["SH_FOLD_CHECK"] = mode
    g = runtime.GpuQuery(spec)
    run_pushes(g, pushes[:1])
    g.close()
"""


def test_the_switch_reaches_the_fold():
    """SH_TRACE's run_closed line names the mode each query's fold was launched with (the trace switch is read
    once per process, hence the child): unset, 1 and 2 in that order, one push of the one-chunk case each."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SH_TRACE="1")
    env.pop("SH_FOLD_CHECK", None)
    r = subprocess.run([sys.executable, "-c", TRACE_CHILD], cwd=root, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    modes = [int(m) for m in re.findall(r"run_closed nseg=.* fold_check=(\d)", r.stderr)]
    assert [m for i, m in enumerate(modes) if i == 0 or m != modes[i - 1]] == [0, 1, 2], modes


@pytest.mark.parametrize("case", ["one_chunk", "many_units"])
def test_one_workgroup_per_unit(rt, monkeypatch, case):
    monkeypatch.setenv("SH_FOLD_GRID", "0")
    check_modes(rt, monkeypatch, case, min_flushes=80 if case == "many_units" else 1)
