"""g4s_ilu0_* from different host threads at the same time (include/g4s.h, "Threads and streams": an apply only reads its handle, different handles
are independent): four threads apply on ONE shared handle, each into a z of its own on a stream of its own; two more threads, each with a stream of its
own, analyse different matrices with device and with host pointers, refactorise and apply. Every factor array and every z is compared with
tests/ilu_ref.py bit for bit — which is also what the single-threaded tests of test_ilu_gpu.py get."""
import threading

import pytest
import torch

from tests import ilu_ref as ref
from tests import test_ilu_gpu as tig

pytestmark = pytest.mark.gpu

JOBS = ("grid40", "blocks")


def test_four_threads_on_one_handle_and_two_threads_analysing():
    cases = [ref.case(name) for name in JOBS]                              # built before the threads start: the cache is not what is tested
    shared = tig.Fact(cases[0][0])
    (n, rp, ci, va), f, _, r, z = cases[0]
    wants = [z] + [ref.apply(n, rp, ci, f, r * (k + 1.0)) for k in range(1, 4)]
    errors = []

    def own(k):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            mat, f, info, r, z = cases[k]
            with torch.cuda.stream(s):
                for it in range(4):
                    p = tig.Fact(mat, device=it % 2 == 0, no_chains=it == 3, stream=s)
                    tig._same_bits(p.factors(), f, (JOBS[k], it))
                    for alias in (False, True):
                        tig._same_bits(p.apply(r, alias), z, (JOBS[k], it, alias))
                    assert p.factor() == -1
                    tig._same_bits(p.apply(r), z, (JOBS[k], it, "behind factor"))
                    p.close()
        except BaseException as e:                                        # noqa: BLE001 - reported by the main thread
            errors.append((JOBS[k], repr(e)))

    def on_shared(k):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            rk = r * (k + 1.0)
            with torch.cuda.stream(s):
                for it in range(8):
                    tig._same_bits(shared.apply(rk, stream=s), wants[k], ("shared", k, it))
        except BaseException as e:                                        # noqa: BLE001
            errors.append(("shared", k, repr(e)))

    threads = [threading.Thread(target=own, args=(k,)) for k in range(len(JOBS))] + [threading.Thread(target=on_shared, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    shared.close()
    assert not errors, errors
