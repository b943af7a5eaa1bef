"""Value reference for the semiring SpMV (include/g4s.h, g4s_spmv_semiring), numpy only: every product a_ij ⊗ x_j of a row, reduced by ⊕ per row, an
empty row at the identity, then — accumulate — combined with y (normalised to 1.0 / 0.0 for or-and). min, max and or do not depend on the order of the
products, so the device must match this bit for bit (compare with semiring_ref.same_values)."""
import numpy as np

from tests.semiring_ref import _mul, same_values  # noqa: F401  (same_values: re-exported for the tests)

NEW = ("min_plus", "max_plus", "or_and")
IDENTITY = {"plus_times": 0.0, "min_plus": np.inf, "max_plus": -np.inf, "or_and": 0.0}


def _combine(name, a, b):
    return np.minimum(a, b) if name == "min_plus" else np.maximum(a, b)


def spmv(rp, ci, va, x, semiring, y=None):
    """y := A ⊗ x (y None) or y ⊕ (A ⊗ x) over one of NEW; returns a new array."""
    assert semiring in NEW
    rp, ci, va, x = (np.asarray(a) for a in (rp, ci, va, x))
    rows = len(rp) - 1
    row = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp).astype(np.int64))
    prod = _mul(semiring, va.astype(np.float64), x[ci.astype(np.int64)].astype(np.float64))
    out = np.full(rows, IDENTITY[semiring])
    if semiring == "min_plus":
        np.minimum.at(out, row, prod)
    else:
        np.maximum.at(out, row, prod)
    if y is not None:
        old = np.asarray(y, np.float64)
        if semiring == "or_and":
            old = (old != 0).astype(np.float64)
        out = _combine(semiring, out, old)
    return out
