"""g4s_strongly_connected_components from different host threads at the same time (include/g4s.h: no process-wide state, so threads may call side by
side): four threads, each with a stream of its own and a graph of its own — thousands of one-vertex steps, hub rows through every phase, many classes
reached at once, a real bow-tie — repeat the call with device and with host pointers, the transpose given and built; every result is compared with
tests/scc_ref.py with ==. The scratch of a call is its own and the read-back ledger is per thread."""
import threading

import numpy as np
import pytest
import torch

from tests import scc_ref as ref
from tests import test_scc_gpu as tsg

pytestmark = pytest.mark.gpu

JOBS = ("cycle", "two_hubs", "cycles_dag", "rmat13")


def test_host_threads_on_streams_of_their_own():
    jobs = [ref.case(name) for name in JOBS]
    errors = []

    def work(k):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            n, rp, ci, trp, tci, r = jobs[k]
            with torch.cuda.stream(s):
                dev = tuple(tsg._dev(a) for a in (rp, ci, trp, tci))
                for it in range(6):
                    device, given = it % 2 == 0, it % 3 != 2
                    a = dev if device else (rp, ci, trp, tci)
                    labels, info, _ = tsg._call(a[0], a[1], n, tr=(a[2], a[3]) if given else None, device=device, stream=s)
                    assert np.array_equal(labels, r["labels"]), (JOBS[k], it)
                    tsg._check_info(info, r, not given)
        except BaseException as e:                                        # noqa: BLE001 - reported by the main thread
            errors.append((JOBS[k], repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(len(JOBS))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
