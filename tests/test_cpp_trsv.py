"""The C++ form of the triangular solve (include/g4s/csr.hpp: TriangularSolve) in a small program, examples/trsv.cpp: built with the helper of
tests/test_cpp_host.py everywhere; on the GPU box it runs on a whole five-point grid matrix written as a MatrixMarket file, as lower and as upper, and
what it prints is compared with tests/trsv_ref.py: the counts with ==, the levels with ==, x bit for bit."""
import subprocess

import numpy as np
import pytest

from tests import trsv_ref as ref
from tests.test_cpp_host import _build_example


def test_trsv_example_compiles(tmp_path):
    _build_example("trsv.cpp", str(tmp_path / "trsv"))


@pytest.mark.gpu
def test_trsv_example_prints_the_reference_solution(tmp_path):
    exe = str(tmp_path / "trsv")
    _build_example("trsv.cpp", exe)
    n, rp, ci, va = ref.grid5(8)
    rows = np.repeat(np.arange(n), np.diff(rp))
    f = tmp_path / "grid8.mtx"
    f.write_text(f"%%MatrixMarket matrix coordinate real general\n{n} {n} {ci.size}\n" + "".join(f"{i + 1} {j + 1} {x!r}\n" for i, j, x in zip(rows.tolist(), ci.tolist(), va.tolist())))
    for lower in (True, False):
        out = subprocess.run([exe, str(f)] + ([] if lower else ["upper"]), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
        lines = out.stdout.splitlines()
        info = ref.info(n, rp, ci, va, lower)
        assert lines[0] == (f"n {n}, nnz_triangle {info['nnz_triangle']}, {info['levels']} levels, widest {info['widest_level']}, "
                            f"{info['launches_per_solve']} launches per solve, {info['chains']} chains")
        assert lines[1].startswith("residual ") and float(lines[1].split()[1]) <= 5 * 2.0**-53 / (1 - 5 * 2.0**-53)   # at most 3 entries a row: Higham's bound
        got = [l.split() for l in lines[2:]]
        assert [int(i) for i, _, _ in got] == list(range(n))
        assert [int(l) for _, l, _ in got] == ref.levels(n, rp, ci, va, lower).tolist()
        # the reader keeps each row's entries in file order, so b = T·1 is the sum the example forms left to right and the rows keep their stored order
        b = np.zeros(n)
        for i, c, v in zip(rows.tolist(), ci.tolist(), va.tolist()):
            if (c <= i) if lower else (c >= i):
                b[i] += v
        want = ref.solve(n, rp, ci, va, b, lower)
        assert np.array_equal(np.array([float(x) for _, _, x in got]).view(np.int64), want.view(np.int64))
