"""g4s_ilu0_* on the ILU cases of tests/level_cases.py, which sit on the edges of the shared level frame (level_schedule.hpp, level_tile.hpp): every
stride of ilu_stride in a level launch of several workgroups, tiles that hold lane, wave and workgroup rows at once with the workgroup rows owned by
threads other than 0 in a workgroup other than 0, every chain stride, a chain whose workgroup row pivots on rows its own workgroup factorised a level
earlier, and a handle both of whose analyses meet a hub column. tests/test_level_cases_cpu.py proves that each case stands on its edge; this file runs
them. Every comparison is == on bits against tests/ilu_ref.py, through the checks of test_ilu_gpu.py and test_trsv_multi_gpu.py; every output is
pre-filled with their sentinels."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ilu_ref as ref
from tests import level_cases as lc
from tests import test_trsv_multi_gpu as tm
from tests.test_ilu_gpu import FILL, WORD, Fact, _dev, _same_bits, check_case
from tests.test_ilu_multi_gpu import _ilu

pytestmark = pytest.mark.gpu


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("name", sorted(lc.ILU))
def test_case_equals_reference(name):
    """the checks of test_ilu_gpu.test_case_equals_reference: factors, pivot word and z by bits, both pointer kinds, chains and one launch per level, r
    aliasing z, a second and a third factorisation of what is held; and the launch counts of the model"""
    mat, f, bad, r, z = lc.factored(name)
    info = ref.info(*mat)
    assert info["bad_pivot"] == bad == -1
    check_case(name, mat, f, info, r, z)
    facts = lc.facts(name, _cus())
    assert info["launches_per_factor"] == len(facts["launches"]) and info["chains"] == sum(l[0] == "chain" for l in facts["launches"])
    assert info["levels"] == facts["levels"] == len(facts["launches_no_chains"]) and info["widest_level"] == max(facts["widths"])


@pytest.mark.parametrize("name", sorted(lc.ILU))
def test_block_apply_equals_single_applies_and_reference(name):
    """k = G4S_TRSV_RHS_TILE + 1 columns in both layouts with a padded leading dimension, out of place and in place, chains and one launch per level: every
    column is the device's own single apply by bits; the first column and the one of the tail tile are the reference's as well"""
    from g4s_amd import host
    k = tm._kt() + 1
    mat, f, _, r, z = lc.factored(name)
    n, rp, ci, va = mat
    Rb = np.random.default_rng(60 + len(name)).uniform(-1.0, 1.0, (n, k))
    Rb[:, 0] = r
    for no_chains in (False, True):
        M = host.ilu0((_dev(rp, np.int32), _dev(ci, np.int32), _dev(va, np.float64)), no_chains=True) if no_chains else _ilu(mat)
        _same_bits(M.factors().cpu().numpy(), f, (name, no_chains, "factors"))
        one = tm.singles(M.apply, Rb)
        _same_bits(one[:, 0], z, (name, no_chains, "column 0 against the reference"))
        if not no_chains:
            _same_bits(one[:, k - 1], ref.apply(n, rp, ci, f, Rb[:, k - 1]), (name, "the tail tile against the reference"))
        tm.solve_checked(lambda r_, z_: M.apply(r_, out=z_), Rb, one, (name, no_chains), layouts=(("row", 3), ("col", 5)))
        M.close()


@pytest.mark.parametrize("name", ["arrow_both", "ilu_hub_in_tile_s16"])
def test_factor_with_new_values_equals_a_fresh_analysis(name):
    (n, rp, ci, va), f, _, r, z = lc.factored(name)
    rowid = np.repeat(np.arange(n), np.diff(rp))
    new = np.random.default_rng(11).uniform(1.0, 2.0, va.size) * np.where(ci == rowid, 16.0 + np.diff(rp)[rowid], 0.125)
    want, bad = ref.factor(n, rp, ci, new)
    want_z = ref.apply(n, rp, ci, want, r)
    assert bad == -1 and not np.array_equal(want, f)
    for device in (True, False):
        p = Fact((n, rp, ci, va), device=device)
        assert p.factor(new) == -1
        _same_bits(p.factors(), want, (name, device))
        _same_bits(p.apply(r), want_z, (name, device))
        assert p.factor() == -1                                             # what is held is the new values
        _same_bits(p.factors(), want, (name, device, "held"))
        fresh = Fact((n, rp, ci, new), device=device)
        _same_bits(fresh.factors(), want)
        _same_bits(fresh.apply(r), want_z)
        got, again = C.create_string_buffer(48), C.create_string_buffer(48)
        p.capi.check(p.lib.g4s_ilu0_get_info(p.handle, C.cast(got, C.POINTER(p.capi.ILU0Info))))
        p.capi.check(p.lib.g4s_ilu0_get_info(fresh.handle, C.cast(again, C.POINTER(p.capi.ILU0Info))))
        assert got.raw[:40] == again.raw[:40]                              # everything but the analysis's own launch counts
        p.close()
        fresh.close()


def test_arrow_both_meets_a_hub_column_in_both_analyses():
    """column 0 has 4098 dependents in the lower plan's peel, column n − 1 in the upper plan's: neither resumes, and the handle's counts are the two
    analyses of the model and the factorisation's own launches and waits (ilu.hip, analyse)"""
    mat, f, _, r, z = lc.factored("arrow_both")
    facts = lc.facts("arrow_both", _cus())
    assert facts["frontier_hubs"] == {0: 1} and facts["upper"]["frontier_hubs"] == {0: 1}
    p = Fact(mat)
    low, up = lc.ilu_analyses("arrow_both", _cus())
    print(p.info, low["launches"], up["launches"])
    # `li.launches + ui.launches + launches + 1 + li.launches_per_solve + 2`, launches = 2 opening kernels; `li.host_waits + ui.host_waits + waits`, waits = 3
    assert p.info["launches"] == low["launches"] + up["launches"] + 2 + 1 + len(facts["launches"]) + 2
    assert p.info["host_waits"] == low["host_waits"] + up["host_waits"] + 3
    _same_bits(p.factors(), f)
    _same_bits(p.apply(r), z)
    p.close()


def test_chain_mixed_in_a_captured_graph():
    """factor(new values) and apply of the chain whose workgroup row pivots on rows of the chain's previous level, captured together: two replays on
    changed values equal the eager bits and the reference's"""
    from g4s_amd import host
    (n, rp, ci, va), f, _, r0, z0 = lc.factored("ilu_chain_mixed")
    M = host.ilu0((_dev(rp, np.int32), _dev(ci, np.int32), _dev(va, np.float64)))
    assert M.info["chains"] == 1 and M.info["launches_per_factor"] == 2
    vals, r = _dev(va, np.float64), _dev(r0, np.float64)
    z = torch.full((n,), FILL, dtype=torch.float64, device="cuda")
    word = torch.full((1,), WORD, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            host.capi.check(host.capi.load().g4s_ilu0_factor(M._handle, host._ptr_nn(vals), host.capi.DEVICE_POINTERS, host._ptr_nn(word), host._stream()))
            M.apply(r, out=z)
    torch.cuda.current_stream().wait_stream(side)
    rowid = np.repeat(np.arange(n), np.diff(rp))
    for k in range(2):
        new = np.random.default_rng(30 + k).uniform(1.0, 2.0, va.size) * np.where(ci == rowid, 16.0 + np.diff(rp)[rowid], 0.125)
        vals.copy_(torch.from_numpy(new))
        z.fill_(FILL)
        word.fill_(WORD)
        g.replay()
        torch.cuda.synchronize()
        want, bad = ref.factor(n, rp, ci, new)
        assert int(word.item()) == bad == -1
        _same_bits(M.factors().cpu().numpy(), want, k)
        _same_bits(z.cpu().numpy(), ref.apply(n, rp, ci, want, r0), (k, "reference"))
        _same_bits(z.cpu().numpy(), M.apply(r).cpu().numpy(), (k, "eager"))
    M.close()
