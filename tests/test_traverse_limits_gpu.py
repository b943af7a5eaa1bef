"""g4s_bfs / g4s_sssp on the cases of tests/iteration_cases.py: all six instantiations of bfs_pull_kernel<4 | 16 | 64, VALUES> with the one hit of a row
at its first entry, its last, in a partial last trip, behind a stored 0.0 (no edge) and on a NaN (an edge); a graph of 8·cus·256 + 300 vertices, past the
cap of every row-wise grid; and a hub that a pull step finds and the next push step expands from the hub end of the queue. Every run goes through
_check_bfs / _check_sssp of tests/test_traverse_gpu.py — bit for bit against tests/traverse_ref.py, `reached` included — and the special vertices must have
the levels their descriptors claim. tests/test_iteration_cases_cpu.py proves that the cases stand on their limits for the CU count of the device."""
import numpy as np
import pytest
import torch

from tests import iteration_cases as ic
from tests.test_traverse_gpu import DIRECTIONS, _check_bfs, _check_sssp, _from_arrays

pytestmark = pytest.mark.gpu


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _handle(c):
    rp, ci, va = (a.copy() for a in c.arrays)                          # (the case's arrays are read-only; torch wants writable ones)
    return _from_arrays(rp, ci, va, len(rp) - 1), (rp, ci, va)


@pytest.mark.parametrize("name", ic.PULL_LANES)
def test_pull_lanes(name):
    cus = _cus()
    c = ic.build(name, cus)
    f = ic.tr_facts(c, cus)
    print(f"traverse limits {name}: cus {cus}, " + ", ".join(f"{k} {f[k]}" for k in ("rows", "nnz", "avg", "lpr", "values", "pull_grid", "pull_trips", "depth")))
    assert (f"pull_lanes_{f['lpr']}_{'values' if f['values'] else 'plain'}") == name
    A, arrays = _handle(c)
    l_ref, infos = _check_bfs(A, arrays, list(c.sources), directions=("pull", "auto"))
    for tag, s in c.special.items():
        assert l_ref[s.vertex] == s.level, (tag, s, int(l_ref[s.vertex]))
    if f["values"]:
        sp = c.special
        assert l_ref[sp["zero_hidden_never"].vertex] == -1 and l_ref[sp["zero_hidden_later"].vertex] == 3 and l_ref[sp["nan_edge"].vertex] == 2
    assert infos["pull"]["push_steps"] == 0 and infos["pull"]["pull_steps"] == f["depth"] + 1
    assert infos["pull"]["reached"] == infos["auto"]["reached"] == f["rows"] - f["unreachable"]


@pytest.fixture(scope="module")
def rows_wrap():
    """rows_wrap and its handle, built once for the module"""
    c = ic.build("rows_wrap", _cus())
    A, arrays = _handle(c)
    return c, A, arrays, ic.tr_facts(c, _cus())


def test_rows_wrap_bfs(rows_wrap):
    c, A, arrays, f = rows_wrap
    print(f"traverse limits rows_wrap: cus {_cus()}, " + ", ".join(f"{k} {f[k]}" for k in ("rows", "nnz", "lpr", "rows_grid", "rows_trips", "pull_grid", "pull_trips", "depth")))
    assert f["rows_trips"] == 2 and f["pull_trips"] == 5 and f["rows_capped"] and f["pull_capped"]
    l_ref, infos = _check_bfs(A, arrays, list(c.sources), directions=DIRECTIONS)
    assert int(l_ref.max()) == 3 and int(np.sum(l_ref < 0)) == 300 and np.all(l_ref[-300:] == -1)
    for info in infos.values():
        assert info["reached"] == f["rows"] - 300


def test_rows_wrap_sssp(rows_wrap):
    c, A, arrays, f = rows_wrap
    d_ref, infos = _check_sssp(A, arrays, list(c.sources), directions=DIRECTIONS)
    assert np.all(np.isinf(d_ref[-300:])) and np.all(np.isfinite(d_ref[:-300]))
    assert infos["auto"]["pull_steps"] > 0 and infos["auto"]["push_steps"] > 0, infos["auto"]     # sssp_combine_kernel wraps in "auto" as well


def test_a_hub_found_by_a_pull_step_is_pushed_next(monkeypatch):
    c = ic.build("pull_then_push_hub", _cus())
    A, arrays = _handle(c)
    rp, ci, _ = arrays
    monkeypatch.setenv("G4S_TRAVERSE_ALPHA", str(int(ic.HUB_ALPHA)))
    trace = ic.direction_trace(c.arrays, c.sources, ic.HUB_ALPHA)
    assert trace == ("push", "pull", "push", "push")                   # the source, the fan, H from the hub end of the queue, and the closing step
    H = c.special["hub"].vertex
    leaves = ci[rp[H]:rp[H + 1]]
    assert len(leaves) == 5000 > ic.HUB_CUT
    l_ref, infos = _check_bfs(A, arrays, list(c.sources), directions=("auto",))
    assert infos["auto"]["push_steps"] == trace.count("push") == 2 + 1 and infos["auto"]["pull_steps"] == trace.count("pull") == 1, infos
    assert l_ref[H] == 2 and np.all(l_ref[leaves] == 3)
    d_ref, infos = _check_sssp(A, arrays, list(c.sources), directions=("auto",))
    assert infos["auto"]["push_steps"] == 2 + 1 and infos["auto"]["pull_steps"] == 1, infos
    assert np.all(np.isfinite(d_ref[leaves])) and np.all(d_ref[leaves] > d_ref[H])


def test_direction_trace_is_what_the_device_counts(monkeypatch):
    """the hand-worked graph of tests/test_iteration_cases_cpu.py: push, pull, pull, push and the closing push under alpha = 4"""
    arrays, sources = ic.hand_worked()
    rp, ci, va = (a.copy() for a in arrays)
    A = _from_arrays(rp, ci, va, 8)
    for alpha in (4, 1, 100):
        monkeypatch.setenv("G4S_TRAVERSE_ALPHA", str(alpha))
        trace = ic.direction_trace(arrays, sources, float(alpha))
        _, infos = _check_bfs(A, (rp, ci, va), list(sources), directions=("auto",))
        info = infos["auto"]
        assert (info["push_steps"], info["pull_steps"], info["iterations"]) == (trace.count("push"), trace.count("pull"), len(trace)), (alpha, trace, info)
