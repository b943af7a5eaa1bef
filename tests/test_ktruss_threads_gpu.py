"""g4s_ktruss from different host threads at the same time (include/g4s.h: no process-wide state, so threads may call side by side): four threads, each
with a stream of its own and a graph of its own — many levels, a long run of dependent rounds, a hub edge peeled alone, a hub edge in the support
pass — repeat the call with device and with host pointers; every result is compared with tests/ktruss_ref.py with ==, which is also what the
single-threaded runs of tests/test_ktruss_gpu.py give. The scratch of a call is its own and the read-back ledger is per thread."""
import threading

import numpy as np
import pytest
import torch

from tests import ktruss_ref as ref
from tests import test_ktruss_gpu as tkg

pytestmark = pytest.mark.gpu

JOBS = ("rmat10", "tri_grid", "hub_bridge", "hub_pair")


def test_host_threads_on_streams_of_their_own():
    jobs = [ref.case(name) for name in JOBS]
    single = []
    for n, rp, ci, *_ in jobs:                                            # the single-threaded results, on the default stream
        t, r, s, _, _ = tkg._call(rp, ci, n)
        single.append((t, r, s))
    errors = []

    def work(k):
        try:
            torch.cuda.set_device(0)
            st = torch.cuda.Stream()
            n, rp, ci, support, truss, rnd, levels, rounds = jobs[k]
            with torch.cuda.stream(st):
                rp_t, ci_t = tkg._dev(rp), tkg._dev(ci)
                for it in range(6):
                    device = it % 2 == 0
                    t, r, s, info, _ = tkg._call(rp_t if device else rp, ci_t if device else ci, n, device=device, with_round=it % 3 != 2,
                                                 with_support=it % 3 != 1, stream=st)
                    assert np.array_equal(t, single[k][0]) and (r is None or np.array_equal(r, single[k][1])), (JOBS[k], it)
                    assert s is None or np.array_equal(s, single[k][2]), (JOBS[k], it)
                    assert np.array_equal(t, truss), (JOBS[k], it)
                    tkg._check_info(info, rp, ci, n, support, truss, levels, rounds)
        except BaseException as e:                                        # noqa: BLE001 - reported by the main thread
            errors.append((JOBS[k], repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(len(JOBS))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
