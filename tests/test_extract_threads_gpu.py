"""g4s_csr_extract_* from different host threads at the same time (include/g4s.h, "Different host threads may call at the same time"): each thread has a
stream of its own and a job of its own — one that sorts nothing, one that sorts rows in a wave and in LDS — and repeats both calls; every result is compared
with tests/extract_ref.py bit for bit. The scratch of a call is its own and the read-back ledger is per thread: nothing of one call may show in another."""
import threading

import numpy as np
import pytest
import torch

from tests import extract_ref as ref
from tests import test_extract_gpu as teg

pytestmark = pytest.mark.gpu


def test_host_threads_on_streams_of_their_own():
    jobs = []
    for k in range(3):
        rng = np.random.default_rng(30 + k)
        rows, cols = 50 + 7 * k, 300
        A = teg._rows_of(rng.integers(1, 200, rows).tolist(), cols, 30 + k, canonical=k != 2)
        I = rng.integers(0, rows, 80)
        J = (np.sort(rng.integers(0, cols, 500)), rng.permutation(cols), rng.integers(0, cols, 700))[k]   # nothing sorted | rows sorted | repeats, unsorted rows
        jobs.append((A, rows, cols, I, J, ref.extract(A[0], A[1], A[2], rows, cols, I, J)))
    errors = []

    def work(k):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            A, rows, cols, I, J, want = jobs[k]
            for _ in range(10):
                teg._exact(teg._raw(A, rows, cols, I, J, stream=s), want)
        except BaseException as e:                                        # noqa: BLE001 - reported by the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
