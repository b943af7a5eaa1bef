"""g4s_kcore from different host threads at the same time (include/g4s.h: no process-wide state, so threads may call side by side): four threads, each
with a stream of its own and a graph of its own — many small rounds, hubs, a frontier that doubles, many levels — repeat the call with device and with
host pointers; every result is compared with tests/kcore_ref.py with ==. The scratch of a call is its own and the read-back ledger is per thread."""
import threading

import numpy as np
import pytest
import torch

from tests import kcore_ref as ref
from tests import test_kcore_gpu as tkg

pytestmark = pytest.mark.gpu

JOBS = ("path", "hub_leaves_clique", "doubling_tree", "rmat13")


def test_host_threads_on_streams_of_their_own():
    jobs = [ref.case(name) for name in JOBS]
    errors = []

    def work(k):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            n, rp, ci, core, rnd, levels, rounds = jobs[k]
            with torch.cuda.stream(s):
                rp_t, ci_t = tkg._dev(rp), tkg._dev(ci)
                for it in range(6):
                    device = it % 2 == 0
                    c, r, info, _ = tkg._call(rp_t if device else rp, ci_t if device else ci, n, device=device, with_round=it % 3 != 2, stream=s)
                    assert np.array_equal(c, core) and (r is None or np.array_equal(r, rnd)), (JOBS[k], it)
                    tkg._check_info(info, rp, ci, n, core, levels, rounds)
        except BaseException as e:                                        # noqa: BLE001 - reported by the main thread
            errors.append((JOBS[k], repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(len(JOBS))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
