"""g4s_minimum_spanning_forest from different host threads at the same time (include/g4s.h: no process-wide state, so threads may call side by side): six
threads, each with a stream of its own and a graph of its own — a long hook chain, the most rounds, a hub of several chunks, heavy ties, a random graph
with many components, all ties without values — repeat the call with device and with host pointers, minimum and maximum; every result is compared with
tests/msf_ref.py with ==. The scratch of a call is its own and the read-back ledger is per thread."""
import threading

import pytest
import torch

from tests import msf_ref as ref
from tests import test_msf_gpu as tmg

pytestmark = pytest.mark.gpu

JOBS = ("path_inc", "path_alt", "star10000", "star4097_tied", "tri_full", "grid64_null")


def test_host_threads_on_streams_of_their_own():
    jobs = [(ref.case(name), ref.case(name, True)) for name in JOBS]
    errors = []

    def work(k):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            n, rp, ci, w, _ = jobs[k][0]
            with torch.cuda.stream(s):
                dev = (tmg._dev(rp), tmg._dev(ci), None if w is None else tmg._dev(w, "float64"))
                for it in range(6):
                    device, maximum = it % 2 == 0, it % 3 == 2
                    a = dev if device else (rp, ci, w)
                    got = tmg._call(a[0], a[1], a[2], n, maximum=maximum, device=device, stream=s)
                    tmg._check(got, jobs[k][int(maximum)][4], n, (JOBS[k], it))
        except BaseException as e:                                        # noqa: BLE001 - reported by the main thread
            errors.append((JOBS[k], repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(len(JOBS))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
