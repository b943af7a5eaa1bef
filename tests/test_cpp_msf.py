"""The C++ form of the spanning forest (include/g4s/csr.hpp: MinimumSpanningForest, MaximumSpanningForest) in a small program, examples/msf.cpp: built with
the helper of tests/test_cpp_host.py everywhere; on the GPU box it runs on the two cliques with a light and a heavy bridge, written as a MatrixMarket
file, and what it prints is compared with tests/msf_ref.py."""
import subprocess

import numpy as np
import pytest

from tests import msf_ref as ref
from tests.test_cpp_host import _build_example


def test_msf_example_compiles(tmp_path):
    _build_example("msf.cpp", str(tmp_path / "msf"))


@pytest.mark.gpu
def test_msf_example_prints_the_reference_forest(tmp_path):
    exe = str(tmp_path / "msf")
    _build_example("msf.cpp", exe)
    n, rp, ci, w, _ = ref.case("two_k6")
    rows = np.repeat(np.arange(n), np.diff(rp))
    f = tmp_path / "two_k6.mtx"
    f.write_text(f"%%MatrixMarket matrix coordinate real general\n{n} {n} {ci.size}\n" + "".join(f"{i + 1} {j + 1} {x!r}\n" for i, j, x in zip(rows.tolist(), ci.tolist(), w.tolist())))
    for maximum in (False, True):
        r = ref.case("two_k6", maximum)[4]
        out = subprocess.run([exe, str(f)] + (["max"] if maximum else []), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr
        lines = out.stdout.splitlines()
        assert lines[0].startswith(f"{r['edges']} edges, {r['components']} components, weight {r['weight']:.17g}, ")
        # no pair is stored twice in one direction, so the forest as a set of pairs does not depend on the order the reader gives a row
        got = [tuple(int(x) for x in l.split()[:3]) for l in lines[1:]]
        assert [k for k, _, _ in got] == sorted(k for k, _, _ in got)
        assert {(min(i, j), max(i, j)) for _, i, j in got} == ref.pairs(rp, ci, r["positions"], n)
