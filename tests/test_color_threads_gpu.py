"""g4s_color from different host threads at the same time (include/g4s.h: no process-wide state, so threads may call side by side): four threads, each
with a stream of its own and a graph and an order of its own — a long chain of small steps, a hub behind a full mask, a deep tree, an R-MAT — repeat the
call with device and with host pointers; every result is compared with tests/color_ref.py with ==. The scratch of a call is its own and the read-back
ledger is per thread."""
import threading

import numpy as np
import pytest
import torch

from tests import color_ref as ref
from tests import test_color_gpu as tcg

pytestmark = pytest.mark.gpu

JOBS = (("path", "smallest_last"), ("clique65_hub", "own"), ("doubling_tree", "largest_first"), ("rmat13", "hash"))


def test_host_threads_on_streams_of_their_own():
    jobs = [ref.case(*job) for job in JOBS]
    errors = []

    def work(k):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            n, rp, ci, key, col, rnd, over = jobs[k]
            largest = JOBS[k][1] == "largest_first"
            with torch.cuda.stream(s):
                rp_t, ci_t = tcg._dev(rp), tcg._dev(ci)
                key_t = None if key is None or largest else tcg._dev(key)
                for it in range(6):
                    device = it % 2 == 0
                    c, r, info, _ = tcg._call(rp_t if device else rp, ci_t if device else ci, n, key=key_t if device else (None if largest else key),
                                              largest=largest, device=device, with_round=it % 3 != 2, stream=s)
                    assert np.array_equal(c, col) and (r is None or np.array_equal(r, rnd)), (JOBS[k], it)
                    tcg._check_info(info, rp, ci, n, col, rnd, over)
        except BaseException as e:                                        # noqa: BLE001 - reported by the main thread
            errors.append((JOBS[k], repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(len(JOBS))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
