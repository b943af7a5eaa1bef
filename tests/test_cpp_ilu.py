"""The C++ form of the ILU(0) factorisation (include/g4s/csr.hpp: ILU0) in a small program, examples/ilu.cpp: built with the helper of
tests/test_cpp_host.py everywhere; on the GPU box it factorises the five-point Laplacian of an 8 × 8 grid, and what it prints is compared with
tests/ilu_ref.py: the counts with ==, the factors, z and the factors of the doubled matrix bit for bit."""
import subprocess

import numpy as np
import pytest

from tests import ilu_ref as ref
from tests.test_cpp_host import _build_example


def test_ilu_example_compiles(tmp_path):
    _build_example("ilu.cpp", str(tmp_path / "ilu"))


@pytest.mark.gpu
def test_ilu_example_prints_the_reference_factors(tmp_path):
    exe = str(tmp_path / "ilu")
    _build_example("ilu.cpp", exe)
    n, rp, ci, va = ref.laplace5(8)
    out = subprocess.run([exe, "8"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = out.stdout.splitlines()
    info = ref.info(n, rp, ci, va)
    assert lines[0] == (f"n {n}, nnz {info['nnz']}, {info['levels']} levels, widest {info['widest_level']}, {info['launches_per_factor']} launches per factor, "
                        f"{info['chains']} chains, {info['launches_per_apply']} launches per apply, bad pivot -1")
    # at most 3 terms a position, all of one sign, so Σ|terms| = |a_ij| up to rounding: γ_3 for the factorisation (Higham, Lemma 8.4) and γ_3 for the
    # sum the example forms itself, 6u and a little — 8u
    assert lines[1].startswith("defect ") and float(lines[1].split()[1]) <= 8 * 2.0**-53
    assert lines[2] == "refactor -1"
    f, _ = ref.factor(n, rp, ci, va)
    g, _ = ref.factor(n, rp, ci, 2.0 * va)
    z = ref.apply(n, rp, ci, f, ref.dense(n, rp, ci, va) @ np.ones(n))       # every row sum is a small integer: r is exact in any order
    got = {tag: np.array([float(l.split()[2]) for l in lines[3:] if l.split()[0] == tag]) for tag in "fzg"}
    for tag, want in (("f", f), ("z", z), ("g", g)):
        assert got[tag].size == want.size and np.array_equal(got[tag].view(np.int64), want.view(np.int64)), tag
