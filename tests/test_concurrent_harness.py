"""tests/concurrency.py on two toy functions that model DtFill.run_numpy's host race in plain numpy (no GPU): a staging array
that every caller shares, with time between the copy in and the copy out, as there is between the staging copy and the DMA.
The harness must report mismatches for the unlocked function and none for the same function behind a lock: the evidence that
tests/test_gpu_reentrancy.py can see this class of bug."""
import threading
import time

import numpy as np

import concurrency

WORKERS, ROUNDS, N = 4, 10, 4096


class Staged:
    """out = 2 * x through a shared staging array: copy in, a millisecond, copy out."""

    def __init__(self, lock=None):
        self.stage = np.zeros(N, np.float32)
        self.lock = lock

    def unsafe(self, x):
        np.copyto(self.stage, x)
        time.sleep(0.001)
        return 2 * self.stage

    def __call__(self, x):
        if self.lock is None:
            return self.unsafe(x)
        with self.lock:
            return self.unsafe(x)


def drive(f):
    xs = [np.full(N, k + 1, np.float32) for k in range(WORKERS)]  # every worker's frames differ in every element
    want = [2 * x for x in xs]

    def work(k, r):
        assert np.array_equal(f(xs[k]), want[k]), "worker %d got another worker's frames" % k

    return concurrency.run_rounds(work, WORKERS, ROUNDS, timeout=30.0)


def test_the_shared_staging_array_is_caught():
    failures = drive(Staged())
    # four workers copy in within the same millisecond: at most one of a round reads its own frames back
    assert len(failures) >= ROUNDS, concurrency.describe(failures)
    assert all(isinstance(e, AssertionError) and r is not None for _, r, e in failures), concurrency.describe(failures)
    assert len({k for k, _, _ in failures}) >= 2  # (it is not one unlucky worker)


def test_the_same_function_behind_a_lock_is_clean():
    failures = drive(Staged(threading.Lock()))
    assert not failures, concurrency.describe(failures)


def test_another_exception_ends_the_run():
    """Anything but an AssertionError (a device's runtime error, say) is reported and nothing is started after it."""
    started = []

    def work(k, r):
        started.append((k, r))
        if (k, r) == (1, 2):
            raise RuntimeError("boom")

    failures = concurrency.run_rounds(work, WORKERS, ROUNDS, timeout=30.0)
    assert [(k, r, str(e)) for k, r, e in failures] == [(1, 2, "boom")]
    assert max(r for _, r in started) == 2  # (round 3's barrier never fills: worker 1 is gone)


def test_a_worker_that_does_not_return_fails_the_run_instead_of_hanging_it():
    gate = threading.Event()

    def work(k, r):
        if k == 0:
            gate.wait(30.0)

    t0 = time.monotonic()
    try:
        failures = concurrency.run_rounds(work, 2, 2, timeout=0.05)
    finally:
        gate.set()
    assert time.monotonic() - t0 < 5.0
    assert any(k == 0 and str(e) == concurrency.STILL_ALIVE for k, _, e in failures), concurrency.describe(failures)
