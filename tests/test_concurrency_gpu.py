"""Concurrent use of libg4s_hip.so: several handles on several streams from one thread, six host threads making synchronous calls, the process-wide
carried symbolic state taken apart by another thread, and g4s_last_error() staying with its thread. Each scenario of tests/concurrency_worker.py runs
in a fresh child process; the child compares every result with == (tests/concurrency_cases.py: integer values) and prints what differed.

A child that ends by signal or by its time limit sets a flag, and every later test of this module fails at once without starting a child:
nothing more is started on a card that may have faulted. One child at a time.

Time limits: ten times the measured duration of the worker's whole run, which contains the scenario's serial pass (MEASURED below, seconds on an
MI355X: serial pass / concurrent pass / the worker's main(): the expected results on the CPU, warm-up, device copies, both passes), plus START_UP for
what the worker cannot time itself (starting Python, importing torch and the cases). That is looser than ten times the serial pass alone: the child
cannot be given less than it needs before its first call. The limit only guards against a hang; it asserts nothing about speed. A thread that waits
at a barrier gives up after concurrency_cases.BARRIER_TIMEOUT, below every limit here, and the scenario then ends with a difference, not a kill.
carried_inplace is one thread: its two figures are the same run.

Overlap in threads_synchronous_calls (and the contended column scratch inside it) is attempted, not proven: from outside the library nothing
shows that two calls were in flight at once. The parts that cannot pass by luck are the barrier-ordered scenarios (carried_*, errors_*) and the
deterministic switch test test_spgemm_gpu.py::test_spgemm_without_column_scratch."""
import json
import os
import subprocess
import sys

import pytest

from tests import concurrency_cases as cc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "concurrency_worker.py")

START_UP = 60.0
# scenario: (serial pass, concurrent pass, the worker's main()) in seconds, measured once on an MI355X
MEASURED = {
    "handles_on_streams": (0.025, 0.003, 0.936),
    "threads_synchronous_calls": (5.159, 2.01, 16.928),
    "carried_product": (0.271, 0.388, 4.118),
    "carried_trim": (0.24, 0.219, 3.956),
    "carried_symbolic": (0.344, 0.273, 4.338),
    "carried_inplace": (0.411, 0.411, 3.902),
    "errors_stay_with_their_thread": (3.548, 0.752, 14.5),
}
_suspect = []                     # why no further child is started


def _limit(scenario):
    return 10.0 * MEASURED[scenario][2] + START_UP


assert cc.BARRIER_TIMEOUT < min(_limit(s) for s in MEASURED)


def _run(scenario):
    if _suspect:
        pytest.fail(f"not started: {_suspect[0]}")
    limit = _limit(scenario)
    try:
        r = subprocess.run([sys.executable, WORKER, scenario], cwd=ROOT, timeout=limit, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired as e:
        _suspect.append(f"the child of {scenario} was killed after {limit:.0f} s (a hang)")
        pytest.fail(f"{_suspect[0]}; stderr: {(e.stderr or b'')[-2000:]!r}")
    if r.returncode < 0:
        _suspect.append(f"the child of {scenario} ended by signal {-r.returncode}")
        pytest.fail(f"{_suspect[0]}; stderr: {r.stderr[-2000:]}")
    assert r.returncode == 0, f"exit status {r.returncode}; stderr: {r.stderr[-4000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, f"no result line; stdout: {r.stdout[-2000:]}"
    out = json.loads(lines[-1])
    print(f"{scenario}: {out['calls']} calls, serial {out['serial_s']} s, concurrent {out['concurrent_s']} s, child {out['total_s']} s")
    assert out["scenario"] == scenario and out["calls"] > 0
    assert out["n_differences"] == 0, "\n".join(out["differences"])
    return out


def test_handles_on_streams():
    """four handles (stream, blocked, diagonal, block-row), a stream each, g4s_spmv / g4s_spmm / g4s_spmv_semiring / g4s_spmv_transpose enqueued
    round-robin without a wait: every y equals the same call made alone, bit for bit, and the CPU reference"""
    assert _run("handles_on_streams")["calls"] == 2 * 8 * 4 * 4


def test_threads_synchronous_calls():
    """six threads, a stream each, different phase-shifted mixes of the synchronous entry points (concurrency_cases.schedule: every call on each of
    the three problems), outputs freed inside the loop; two of them also run the same large product behind a barrier, a third calls g4s_trim in
    the middle of each of its rounds"""
    _run("threads_synchronous_calls")


@pytest.mark.parametrize("variant", ["product", "trim", "symbolic", "inplace"])
def test_carried_symbolic_interleaved(variant):
    """A: symbolic(P1) — B: a one-call product of P2 / g4s_trim / symbolic(P2) — A: numeric(P1), then numeric(P1) with new values; "inplace": one thread,
    the same buffers rewritten with P2 and symbolic + numeric again"""
    _run(f"carried_{variant}")


def test_errors_stay_with_their_thread():
    """A's refusals (bad column id, unsorted mask, negative k) carry A's own message; B and C, in lock step, stay exact and never see A's text"""
    _run("errors_stay_with_their_thread")
