"""The C++ forms of the edge-list front door (include/g4s/csr.hpp: graph, FromGraph, SortAndMerge) in a small program, examples/graph_to_csr.cpp: built
with the helper of tests/test_cpp_host.py everywhere; on the GPU box it runs on a graph with integer weights and repeats, and what it prints is compared
with tests/coo_ref.py."""
import subprocess

import numpy as np
import pytest

from tests import coo_ref as ref
from tests.test_cpp_host import _build_example


def test_graph_to_csr_compiles(tmp_path):
    _build_example("graph_to_csr.cpp", str(tmp_path / "graph_to_csr"))


def _parse(lines):
    rows, cols, nnz = (int(x) for x in lines[0].split())
    rp, ci, va = np.array(lines[1].split(), np.int32), np.array(lines[2].split(), np.int32), np.array(lines[3].split(), np.float64)
    assert len(rp) == rows + 1 and len(ci) == len(va) == nnz and rows == cols
    return rp, ci, va


@pytest.mark.gpu
def test_from_graph_and_sort_and_merge(tmp_path):
    exe = str(tmp_path / "graph_to_csr")
    _build_example("graph_to_csr.cpp", exe)
    rng = np.random.default_rng(21)
    n, m = 60, 5000                                                     # 3 600 positions for 5 000 edges: repeats, and more than one tile
    start, end, w = rng.integers(0, n, m), rng.integers(0, n, m), rng.integers(-50, 51, m).astype(np.float64)
    start[start == 7] = 8                                               # a vertex without out-edges
    edges = tmp_path / "edges.txt"
    edges.write_text(f"{m} {n}\n" + "".join(f"{s} {e} {int(x)}\n" for s, e, x in zip(start, end, w)))
    out = subprocess.run([exe, str(edges)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = out.stdout.splitlines()
    for got, dup in ((_parse(lines[0:4]), "keep"), (_parse(lines[4:8]), "plus")):
        want = ref.from_coo(start, end, w, n, n, dup)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), dup
        assert np.array_equal(got[2].view(np.int64), want[2].view(np.int64)), dup
    assert lines[8] == f"longest_run {ref.from_coo(start, end, w, n, n, 'plus')[4]}"
