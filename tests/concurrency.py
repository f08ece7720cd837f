"""Run the same code from several host threads at once, round by round (helpers only: no tests, no fixtures).

run_rounds() is the one helper: K daemon threads, R rounds, a threading.Barrier at the start of every round so that the K calls of
a round start together, every worker's exception collected.  It never hangs: the barrier and the joins have a time limit, and a
worker that is still alive after it is a failure of its own.

(Not named concurrent.py: the tests' directory is on sys.path, and a module of that name would stand in front of the standard
library's concurrent package, which the product's staging pool and torch import.)
"""
import threading
import time

STILL_ALIVE = "still alive"


def run_rounds(work, workers, rounds, timeout=120.0):
    """Call work(k, r) in thread k = 0 .. workers - 1 for r = 0 .. rounds - 1, all threads released together at the start of every
    round.  Returns the failures as a list of (k, r, exception), in no particular order; an empty list means every call returned.

    An AssertionError is a finding: it is recorded and the worker goes on with the next round, so that the list counts every
    mismatch.  Any other exception (a runtime error of the device, a broken barrier) is recorded and ends all workers at the next
    barrier: nothing more is started after it.  A worker that has not finished `timeout` seconds after the start is reported as
    (k, None, RuntimeError(STILL_ALIVE)); it is a daemon thread, so it cannot keep the process from ending."""
    failures = []
    calls = [0]
    lock = threading.Lock()
    barrier = threading.Barrier(workers)
    deadline = time.monotonic() + timeout

    def record(k, r, e):
        with lock:
            failures.append((k, r, e))

    def body(k):
        for r in range(rounds):
            try:
                barrier.wait(max(0.0, deadline - time.monotonic()))
            except threading.BrokenBarrierError:
                return  # another worker ended the run (its exception is in the list) or the time is up
            try:
                work(k, r)
                with lock:
                    calls[0] += 1
            except AssertionError as e:
                record(k, r, e)
            except BaseException as e:  # noqa: BLE001
                record(k, r, e)
                barrier.abort()
                return

    threads = [threading.Thread(target=body, args=(k,), daemon=True, name="worker-%d" % k) for k in range(workers)]
    for t in threads:
        t.start()
    for k, t in enumerate(threads):
        t.join(max(0.0, deadline - time.monotonic()))
        if t.is_alive():
            barrier.abort()
            record(k, None, RuntimeError(STILL_ALIVE))
    with lock:
        if not failures and calls[0] != workers * rounds:  # (a barrier that ran out of time ends the workers without a word)
            failures.append((None, None, RuntimeError("only %d of %d calls were made in %g s" % (calls[0], workers * rounds, timeout))))
        return list(failures)


def describe(failures, limit=4):
    """The failures as one line for an assertion message."""
    return "%d failure(s): %s" % (len(failures), "; ".join("worker %s round %s: %r" % f for f in failures[:limit]))
