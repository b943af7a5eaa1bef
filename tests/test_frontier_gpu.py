"""The frontier walk that g4s_sssp / g4s_bfs, g4s_betweenness, g4s_connected_components and g4s_kcore share (g4s_amd/csrc/frontier.hpp), on one graph
made for its edges. The "fan" is directed, 6262 vertices and 25 805 entries:
  vertex 0 → 257 mid vertices 1 … 257: one full tile of 256 rows plus one row;
  mid 1 has exactly 4096 out-edges (the hub cut: not a hub), mid 2 has 4097 (a hub whose last chunk holds one edge), mid 3 has 6000, mid 4 has 5000:
  three hubs in one frontier, so chunk ownership runs with h >= 1; mids 5 … 20 have none and mid i of 21 … 257 has i % 4, so 75 rows of length
  zero sit inside the tile; every one of the 6000 leaves → one sink: a level of 23.4 tiles whose edges all land on one vertex; three isolated
  vertices at the end. Source 3 makes the source itself a hub; symmetrised, the sink is a fourth hub.
Compared with the references of tests/traverse_ref.py, betweenness_ref.py, components_ref.py and kcore_ref.py as the features' own test files compare."""
import os

import numpy as np
import pytest

from tests import betweenness_ref as bref
from tests import components_ref as cref
from tests import kcore_ref as kref
from tests import traverse_ref
from tests.traverse_ref import same_values

pytestmark = pytest.mark.gpu

N_MID, N_LEAF = 257, 6000
N = 1 + N_MID + N_LEAF + 1 + 3


def _fan():
    """(rowptr, colids, values): weights U[0.05, 1)."""
    leaves = 1 + N_MID + np.arange(N_LEAF)
    sink = 1 + N_MID + N_LEAF
    rows = [np.empty(0, np.int64) for _ in range(N)]
    rows[0] = 1 + np.arange(N_MID)
    rows[1], rows[2], rows[3], rows[4] = leaves[:4096], leaves[:4097], leaves, leaves[1000:]
    for i in range(21, N_MID + 1):
        rows[i] = leaves[(7 * i + np.arange(i % 4)) % N_LEAF]
    for v in leaves:
        rows[v] = np.array([sink])
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    return rp, ci, np.random.default_rng(20261018).uniform(0.05, 1.0, ci.size)


@pytest.fixture(scope="module")
def fan():
    rp, ci, va = _fan()
    deg = np.diff(rp)
    assert (len(rp) - 1, ci.size) == (6262, 25805)
    assert deg[1] == 4096 and deg[2] == 4097 and (deg > 4096).sum() == 3 and (deg[1:N_MID + 1] == 0).sum() == 75
    return rp, ci, va


@pytest.fixture(scope="module")
def handle(fan):
    from g4s_amd import host
    rp, ci, va = fan
    return host.CSR.from_host(rp, ci, va, N, N)


@pytest.mark.parametrize("source", [0, 3])
def test_sssp_and_bfs_from_the_root_and_from_a_hub(fan, handle, source):
    d_ref, _, converged, _ = traverse_ref.sssp(*fan, N, [source])
    assert converged
    for direction in ("push", "auto"):
        d, info = handle.sssp([source], direction=direction)
        d = d.cpu().numpy()
        print(f"fan sssp {direction} from {source}: {info}")
        assert same_values(d, d_ref), (direction, int(np.sum(d != d_ref)), info)
        assert info["converged"] == 1 and info["reached"] == int(np.isfinite(d_ref).sum()), (direction, info)
    l_ref, depth = traverse_ref.bfs(*fan, N, [source])
    lv, info = handle.bfs([source], direction="push")
    lv = lv.cpu().numpy()
    print(f"fan bfs push from {source}: {info}")
    assert np.array_equal(lv, l_ref), (int(np.sum(lv != l_ref)), info)
    assert info["converged"] == 1 and info["reached"] == int((l_ref >= 0).sum()) and info["iterations"] == depth + 1, info
    assert info["pull_steps"] == 0 and info["edges_relaxed"] == int(np.diff(fan[0])[l_ref >= 0].sum()), info   # BFS walks a reached vertex's row once


def test_betweenness_with_three_hubs_in_one_frontier(fan, handle):
    sources = [0, 3]
    ref = bref.betweenness(*fan, N, sources)
    assert (ref.levels, ref.reached, ref.max_depth) == (7, 12261, 3)
    bc, info = handle.betweenness(sources)
    print(f"fan betweenness: {info}")
    assert (info["levels"], info["reached"], info["max_depth"]) == (ref.levels, ref.reached, ref.max_depth), info
    bref.check_parity("fan", bc.cpu().numpy(), ref.bc)


@pytest.fixture(scope="module")
def sym_fan(fan):
    """(rowptr, colids) of the fan's pattern with both directions of every edge, rows ascending"""
    import scipy.sparse as sp
    rp, ci, _ = fan
    G = sp.csr_matrix((np.ones(ci.size), ci, rp), shape=(N, N))
    S = (G + G.T).tocsr()
    S.sort_indices()
    return S.indptr.astype(np.int32), S.indices.astype(np.int32)


@pytest.mark.parametrize("rounds", [0, 2])
def test_components_of_the_symmetrised_fan(sym_fan, rounds):
    import torch
    from g4s_amd import host
    srp, sci = sym_fan
    deg = np.diff(srp)
    assert deg[N - 4] == N_LEAF and (deg - rounds > 4096).sum() == (5 if rounds == 0 else 3)     # the sink is a hub too
    want, _ = cref.labels(srp, sci, N)
    saved = os.environ.get("G4S_CC_SAMPLE_ROUNDS")
    os.environ["G4S_CC_SAMPLE_ROUNDS"] = str(rounds)
    try:
        for symmetric in (False, True):
            lab, info = host.connected_components((torch.from_numpy(srp).cuda(), torch.from_numpy(sci).cuda()), symmetric=symmetric, return_info=True)
            print(f"fan components rounds={rounds} symmetric={symmetric}: {info}")
            assert np.array_equal(lab.cpu().numpy(), want), (rounds, symmetric)
            assert (info["components"], info["largest"], info["largest_label"]) == cref.stats(want) == (4, N - 3, 0), info
            assert info["sample_rounds"] == rounds and info["host_waits"] == 1 and info["skipped"] == int(symmetric), info
            if not symmetric:
                assert info["edges_linked"] == int(np.maximum(deg - rounds, 0).sum()), info
    finally:
        if saved is None:
            os.environ.pop("G4S_CC_SAMPLE_ROUNDS", None)
        else:
            os.environ["G4S_CC_SAMPLE_ROUNDS"] = saved


@pytest.mark.parametrize("max_k", [None, 2])
def test_kcore_of_the_symmetrised_fan(sym_fan, max_k):
    """Five hubs (mid 1 has 4096 leaves and the root here): the full peel takes them with the 5-core, its last level; max_k = 2 leaves them standing."""
    import torch
    from g4s_amd import host
    srp, sci = sym_fan
    assert (np.diff(srp) > 4096).sum() == 5
    core, rnd, levels, rounds, capped = kref.kcore(srp, sci, N, max_k)
    assert (int(core.max()), levels, rounds, capped, int((rnd < 0).sum())) == ((5, 6, 8, 0, 0) if max_k is None else (2, 2, 2, 1, 6184))
    assert np.all(core[np.diff(srp) > 4096] == int(core.max()))
    for _ in range(2):
        c, r, info = host.kcore((torch.from_numpy(srp).cuda(), torch.from_numpy(sci).cuda()), max_k=max_k, return_round=True, return_info=True)
        print(f"fan kcore max_k={max_k}: {info}")
        assert np.array_equal(c.cpu().numpy(), core) and np.array_equal(r.cpu().numpy(), rnd), (max_k, info)
        assert (info["degeneracy"], info["top_core_size"], info["levels"], info["rounds"], info["capped"]) == (*kref.top_core(core), levels, rounds, capped), info
