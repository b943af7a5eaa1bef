"""g4s_sptrsv_* from different host threads at the same time (include/g4s.h, "Threads and streams": different handles are independent, and a solve only
reads its handle): two threads, each with a stream and a handle of its own, analyse with device and with host pointers and solve repeatedly; a third
and a fourth thread solve on ONE shared handle on streams of their own. Every level array and every x is compared with tests/trsv_ref.py with ==, x bit
for bit — which is also what the single-threaded tests of test_trsv_gpu.py get."""
import threading

import numpy as np
import pytest
import torch

from tests import trsv_ref as ref
from tests import test_trsv_gpu as ttg

pytestmark = pytest.mark.gpu

JOBS = ("grid40", "blocks")


def test_two_threads_two_handles_two_streams():
    cases = [ref.case(name) for name in JOBS]                              # built before the threads start: the cache is not what is tested
    shared = ttg.Plan(cases[0][0])
    errors = []

    def own(k):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            mat, lev, info, b, x = cases[k]
            with torch.cuda.stream(s):
                for it in range(4):
                    p = ttg.Plan(mat, device=it % 2 == 0, no_chains=it == 3, stream=s)
                    assert np.array_equal(p.level, lev)
                    for alias in (False, True, False):
                        ttg._same_bits(p.solve(b, alias), x, (JOBS[k], it, alias))
                    p.close()
        except BaseException as e:                                        # noqa: BLE001 - reported by the main thread
            errors.append((JOBS[k], repr(e)))

    def on_shared(k):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            mat, _, _, b, x = cases[0]
            bk = b * (k + 1.0)
            want = x if k == 0 else ref.solve(*mat, bk)
            with torch.cuda.stream(s):
                for it in range(8):
                    ttg._same_bits(shared.solve(bk, stream=s), want, ("shared", k, it))
        except BaseException as e:                                        # noqa: BLE001
            errors.append(("shared", k, repr(e)))

    threads = [threading.Thread(target=own, args=(k,)) for k in range(len(JOBS))] + [threading.Thread(target=on_shared, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    shared.close()
    assert not errors, errors
