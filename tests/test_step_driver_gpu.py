"""A frontier that outgrows the launch grid of its batch, for g4s_sssp, g4s_bfs and g4s_betweenness: the stop-at-4-and-resume path of the stepped
driver they share with g4s_kcore (frontier.hpp: step_runs, turn_page; step_batch.hpp), which tests/test_kcore_gpu.py reaches for k-core only.

The graph is symmetric: a path of 20 vertices, 0 … 19, whose last vertex is tied to the root (vertex 20) of a complete binary tree of depth 17 —
262 163 vertices. From vertex 0 every frontier is one vertex for 20 steps, then tree level L at step 20 + L with 3 · 2^L entries (a leaf level of
2^17 entries at the end). The first batch of 16 launches runs on the largest grid; every read after it, up to tree level 12, sees a frontier of at
most 4096 vertices and 12 288 entries, (12 288 + 4096) / 2048 = 8, so the batch that follows runs on 8 workgroups with a cap of 8 · 2048 · 8 =
131 072 entries. Batches are 16, 16, 32 launches, so that batch reaches tree level 16, whose 3 · 2^16 = 196 608 entries are above the cap: the step
that builds it sets stop = 4, the launches behind it return at once, and the next batch resumes on a grid sized for what the host then sees.

Everything hangs on the read after 32 steps (the third of a call: 16 + 16 launches), which sees tree level 12; a read one level later would size a
grid of 16 with a cap of 262 144 and stop = 4 would never be set. The info structs carry no resume counter, but the stop costs a read, and
host_waits tells the two paths apart: the 38 steps of a traversal from vertex 0 fit the batches 16 + 16 + 32, three reads, and the batch cut short
at tree level 16 makes them four (WAITS_RESUMED). From the leaf no frontier passes 2^16 + 2^15 entries, below the cap: three reads."""
import numpy as np
import pytest

from tests import betweenness_ref as bref
from tests import traverse_ref
from tests.traverse_ref import same_values

pytestmark = pytest.mark.gpu

PATH, DEPTH = 20, 17
TREE = (1 << (DEPTH + 1)) - 1
N = PATH + TREE
LEAF = N - 1
WAITS_PLAIN, WAITS_RESUMED = 3, 4                                        # state reads of one traversal of 38 steps: batches 16, 16, 32 | 16, 16, 32 cut short, 64


@pytest.fixture(scope="module")
def graph():
    """(rowptr, colids, values): weights U[0.05, 1), the same in both directions of an edge or not — nothing here needs them symmetric."""
    from g4s_amd import capi
    child = np.arange(1, TREE)
    src = np.concatenate([np.arange(PATH), PATH + (child - 1) // 2])      # path edges i — i + 1 (19 — 20 is the tie to the root), then parent — child
    dst = np.concatenate([np.arange(1, PATH + 1), PATH + child])
    rp, ci, _ = bref.symmetrise(N, src, dst)
    deg = np.diff(rp)
    # the premises of the arithmetic above
    assert capi.TRAVERSE_BATCH == capi.BC_BATCH == 16
    assert N == 262163 and ci.size == 2 * (N - 1)
    assert deg[0] == 1 and np.all(deg[1:PATH] == 2) and np.all(deg[PATH:PATH + (1 << DEPTH) - 1] == 3) and np.all(deg[PATH + (1 << DEPTH) - 1:] == 1)
    assert 3 << 16 > 8 * 2048 * 8 >= 3 << 15 and ((3 << 12) + (1 << 12)) // 2048 == 8
    return rp.astype(np.int32), ci.astype(np.int32), np.random.default_rng(20261019).uniform(0.05, 1.0, ci.size)


@pytest.fixture(scope="module")
def handle(graph):
    from g4s_amd import host
    return host.CSR.from_host(*graph, N, N)


def test_sssp_push_resumes_on_a_larger_grid(graph, handle):
    d_ref, _, converged, _ = traverse_ref.sssp(*graph, N, [0])
    assert converged and np.isfinite(d_ref).all()
    d, info = handle.sssp([0], direction="push")
    d = d.cpu().numpy()
    print(f"path into tree, sssp push: {info}")
    assert same_values(d, d_ref), (int(np.sum(d != d_ref)), info)
    assert info["converged"] == 1 and info["reached"] == N and info["pull_steps"] == 0, info
    assert info["host_waits"] == WAITS_RESUMED, info


def test_bfs_push_resumes_on_a_larger_grid(graph, handle):
    l_ref, depth = traverse_ref.bfs(*graph, N, [0])
    assert depth == PATH + DEPTH and int(np.sum(l_ref == PATH + 16)) == 1 << 16
    lv, info = handle.bfs([0], direction="push")
    lv = lv.cpu().numpy()
    print(f"path into tree, bfs push: {info}")
    assert np.array_equal(lv, l_ref), (int(np.sum(lv != l_ref)), info)
    assert info["converged"] == 1 and info["reached"] == N and info["iterations"] == depth + 1, info
    assert info["pull_steps"] == 0 and info["edges_relaxed"] == graph[1].size, info
    assert info["host_waits"] == WAITS_RESUMED, info                      # the zero scan ran with the reservation: it adds no wait here


def test_betweenness_resumes_on_the_full_grid(graph, handle):
    sources = [0, LEAF]                                                   # the far end of the path; a leaf, whose frontiers stay below the cap
    ref = bref.betweenness(*graph, N, sources)
    assert (ref.max_depth, ref.levels, ref.reached) == (PATH + DEPTH, 2 * (PATH + DEPTH + 1), 2 * N)
    bc, info = handle.betweenness(sources)
    print(f"path into tree, betweenness: {info}")
    assert (info["levels"], info["reached"], info["max_depth"], info["sigma_exact"]) == (ref.levels, ref.reached, ref.max_depth, 1), info
    bref.check_parity("path into tree", bc.cpu().numpy(), ref.bc)
    assert info["host_waits"] == WAITS_RESUMED + WAITS_PLAIN + 1, info   # the two forward halves and the wait for the epilogue
