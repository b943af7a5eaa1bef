"""The batch loop that g4s_kcore and g4s_ktruss share (g4s_amd/csrc/level_peel.hpp; its schedule is pinned on the host by tests/test_step_batch_cpu.py),
on a call that ends inside its first batch: the triangle, n = 3 with six stored entries — the smallest pattern that has a scan, a peel and a non-zero
support. The other GPU tests bound the launch counts by inequalities; here they are exact, and they follow from the text of the loop:
  g4s_kcore    3 opening launches + a first batch of G4S_KCORE_BATCH = 16 steps + the finish kernel = 20; one wait for the batch's read, and with
               host pointers one more for the copy back.
  g4s_ktruss   the row check + 9 opening launches (the exclusive scan is three) + 16 steps + the finish kernel = 27; with device pointers the waits
               are the opening read (the call sizes its work block from rowptr[n]) and the batch's read, with host pointers the batch's read and the
               copy back.
No batch is resumed. The values were confirmed on the commit before the loop was shared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWPTR = np.array([0, 2, 4, 6], np.int32)
COLIDS = np.array([1, 2, 0, 2, 0, 1], np.int32)


def _pattern(kind):
    import torch
    if kind == "host":
        return ROWPTR.copy(), COLIDS.copy()
    return torch.from_numpy(ROWPTR).cuda(), torch.from_numpy(COLIDS).cuda()


@pytest.mark.parametrize("kind,waits", [("device", 1), ("host", 2)])
def test_kcore_of_a_triangle_ends_in_its_first_batch(kind, waits):
    from g4s_amd import host
    core, rnd, info = host.kcore(_pattern(kind), return_round=True, return_info=True)
    assert core.cpu().tolist() == [2, 2, 2] and rnd.cpu().tolist() == [0, 0, 0]
    assert (info["launches"], info["host_waits"], info["resumes"]) == (3 + 16 + 1, waits, 0), info
    assert (info["levels"], info["rounds"], info["scans"], info["edges_walked"], info["degeneracy"], info["top_core_size"]) == (1, 1, 2, 6, 2, 3), info


@pytest.mark.parametrize("kind", ["device", "host"])
def test_ktruss_of_a_triangle_ends_in_its_first_batch(kind):
    from g4s_amd import host
    truss, rnd, sup, info = host.ktruss(_pattern(kind), return_round=True, return_support=True, return_info=True)
    assert truss.cpu().tolist() == [3] * 6 and rnd.cpu().tolist() == [0] * 6 and sup.cpu().tolist() == [1] * 6
    assert (info["launches"], info["host_waits"], info["resumes"]) == (1 + 9 + 16 + 1, 2, 0), info
    assert (info["levels"], info["rounds"], info["scans"], info["edges_walked"], info["support_walked"], info["triangles"], info["max_truss"],
            info["top_truss_edges"]) == (1, 1, 2, 6, 6, 1, 3, 3), info
