"""The C++ forms of extract (include/g4s/csr.hpp: Extract, Permute) in a small program, examples/induced_subgraph.cpp: built with the helper of
tests/test_cpp_host.py everywhere; on the GPU box it runs on a 60-vertex graph with integer weights and repeats, and what it prints is compared with
tests/coo_ref.py (the graph) followed by tests/extract_ref.py (the two extractions)."""
import subprocess

import numpy as np
import pytest

from tests import coo_ref, extract_ref as ref
from tests.test_cpp_host import _build_example


def test_induced_subgraph_compiles(tmp_path):
    _build_example("induced_subgraph.cpp", str(tmp_path / "induced_subgraph"))


def _parse(lines):
    rows, cols, nnz = (int(x) for x in lines[0].split())
    rp, ci, va = np.array(lines[1].split(), np.int32), np.array(lines[2].split(), np.int32), np.array(lines[3].split(), np.float64)
    assert len(rp) == rows + 1 and len(ci) == len(va) == nnz and rows == cols
    return rp, ci, va


@pytest.mark.gpu
def test_induced_subgraph_and_reversed_relabelling(tmp_path):
    exe = str(tmp_path / "induced_subgraph")
    _build_example("induced_subgraph.cpp", exe)
    rng = np.random.default_rng(22)
    n, m = 60, 900
    start, end, w = rng.integers(0, n, m), rng.integers(0, n, m), rng.integers(-50, 51, m).astype(np.float64)
    start[start == 7] = 8                                               # a vertex without out-edges
    ids = np.concatenate([rng.permutation(n)[:25], [7, 3, 3]])          # any order, a repeat, the vertex without out-edges
    edges, idfile = tmp_path / "edges.txt", tmp_path / "ids.txt"
    edges.write_text(f"{m} {n}\n" + "".join(f"{s} {e} {int(x)}\n" for s, e, x in zip(start, end, w)))
    idfile.write_text(f"{len(ids)}\n" + " ".join(str(int(v)) for v in ids) + "\n")
    out = subprocess.run([exe, str(edges), str(idfile)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = out.stdout.splitlines()
    rp, ci, va, _, _ = coo_ref.from_coo(start, end, w, n, n, "plus")
    backwards = np.arange(n)[::-1]
    for got, (I, J) in ((_parse(lines[0:4]), (ids, ids)), (_parse(lines[4:8]), (backwards, backwards))):
        want = ref.extract(rp, ci, va, n, n, I, J)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[2].view(np.int64), want[2].view(np.int64))
