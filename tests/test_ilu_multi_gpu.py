"""g4s_ilu0_apply_multi on the device (include/g4s.h): Z = U⁻¹ (L⁻¹ R) for a block of k vectors on the launches of one apply. Column j
of Z is compared, bit for bit, with tests/ilu_ref.py's apply of column j on the reference's factors and with g4s_ilu0_apply of column j on the same
handle; in both layouts, with padding that must keep its sentinel, in place, and captured into a graph behind a factorisation of new values."""
import functools

import numpy as np
import pytest
import torch

from tests import ilu_ref as ref
from tests import test_trsv_multi_gpu as tm

pytestmark = pytest.mark.gpu

CASE_NAMES = ("tridiagonal_cap_plus_1", "grid40", "blocks", "arrow_wave_plus_1", "two_long_rows", "messy", "specials")


def _ks():
    kt = tm._kt()
    return sorted({1, kt, kt + 1, 2 * kt + 3})


@functools.lru_cache(maxsize=None)
def rhs(name):
    """(R, Z) for a named case of ilu_ref: R of n × (2·KT + 3) random columns, shared by every k, and the reference's applies of the first KT + 1 of
    them on its own factors; the other columns are compared with the device's single applies alone. Built once, read-only."""
    (n, rp, ci, va), f, _, _, _ = ref.case(name)
    kt = tm._kt()
    R = np.random.default_rng(9 + len(name)).uniform(-1.0, 1.0, (n, 2 * kt + 3))
    Z = np.stack([ref.apply(n, rp, ci, f, R[:, j]) for j in range(kt + 1)], axis=1)
    R.setflags(write=False)
    Z.setflags(write=False)
    return R, Z


def _ilu(mat):
    from g4s_amd import host
    n, rp, ci, va = mat
    return host.ilu0((tm._dev(rp, np.int32), tm._dev(ci, np.int32), tm._dev(va, np.float64)))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_block_apply_equals_reference_and_single_applies(name):
    kt = tm._kt()
    mat, f, info, _, _ = ref.case(name)
    R, Z = rhs(name)
    M = _ilu(mat)
    assert {k: M.info[k] for k in info} == info
    tm._same_bits(M.factors().cpu().numpy(), f, (name, "factors"))
    one = tm.singles(M.apply, R)
    tm._same_bits(one[:, :kt + 1], Z, (name, "single applies against the reference"))
    for k in _ks():
        tm.solve_checked(lambda r, z: M.apply(r, out=z), R[:, :k], one[:, :k], (name, k))
    fresh = M.apply(torch.from_numpy(np.array(R[:, :kt + 1])).cuda())        # a new out: allocated in r's layout
    assert fresh.stride() == (kt + 1, 1)
    tm._same_bits(fresh.cpu().numpy(), Z)
    fresh = M.apply(torch.from_numpy(np.array(R[:, :kt + 1].T, order="C")).cuda().t())
    assert fresh.stride() == (1, mat[0])
    tm._same_bits(fresh.cpu().numpy(), Z)
    M.close()


def test_factor_and_block_apply_in_a_captured_graph():
    """factor(new values) and the block apply captured together: replays on changed values equal the eager bits and the reference's"""
    from g4s_amd import host
    kt = tm._kt()
    k = kt + 1
    for name, layout in (("blocks", "row"), ("grid40", "col")):
        (n, rp, ci, va), f, info, _, _ = ref.case(name)
        R, _ = rhs(name)
        M = _ilu((n, rp, ci, va))
        vals = tm._dev(va, np.float64)
        rst, r = tm.block(R[:, :k], layout, 2)
        zst, z = tm.empty_block((n, k), layout, 2)
        word = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                host.capi.check(host.capi.load().g4s_ilu0_factor(M._handle, host._ptr_nn(vals), host.capi.DEVICE_POINTERS, host._ptr_nn(word), host._stream()))
                M.apply(r, out=z)
        torch.cuda.current_stream().wait_stream(side)
        rowid = np.repeat(np.arange(n), np.diff(rp))
        for it in range(2):
            new = np.random.default_rng(30 + it).uniform(1.0, 2.0, va.size) * np.where(ci == rowid, 16.0 + np.diff(rp)[rowid], 0.125)
            vals.copy_(torch.from_numpy(new))
            word.fill_(-7)
            g.replay()
            torch.cuda.synchronize()
            want, bad = ref.factor(n, rp, ci, new)
            assert int(word.item()) == bad == -1
            tm._same_bits(M.factors().cpu().numpy(), want, (name, it))
            eager = M.apply(r).cpu().numpy()
            tm.check_block(zst, (n, k), layout, 2, eager, (name, it, "eager"))
            tm._same_bits(eager[:, 0], ref.apply(n, rp, ci, want, R[:, 0]), (name, it, "reference"))
            tm._same_bits(eager[:, k - 1], ref.apply(n, rp, ci, want, R[:, k - 1]), (name, it, "reference, the tail tile"))
        M.close()
