"""Host-form isolation across threads on one handle (the SRS, PRACH and CSI-RS GPU tests share this).

The host form of a C-ABI object keeps one private device buffer and one private stream per handle, and ctypes releases
the GIL during the call: threads that use the host form of one handle at the same time must each get the result of
their own input.  This checks isolation only; correctness against the reference is the other tests' job.
"""
import threading

THREADS, REPEATS = 4, 8


def check_isolation(call, inputs, bits):
    """call(input) is the host form on the shared handle, bits(result) the result's exact bytes.  Each of the THREADS
    inputs is computed once single-threaded; then one thread per input calls REPEATS times, all started together, and
    every result must equal that thread's single-threaded one bit for bit."""
    assert len(inputs) == THREADS
    want = [bits(call(x)) for x in inputs]
    assert len(set(want)) == THREADS, "the inputs must give distinct results, or a mixed-up one would not show"
    got = [[] for _ in inputs]
    errors = []
    barrier = threading.Barrier(THREADS)

    def worker(i):
        try:
            barrier.wait(timeout=30)
            for _ in range(REPEATS):
                got[i].append(bits(call(inputs[i])))
        except Exception as e:  # reported by the main thread
            errors.append((i, e))
            barrier.abort()

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(THREADS)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(THREADS):
        wrong = [r for r, g in enumerate(got[i]) if g != want[i]]
        assert len(got[i]) == REPEATS and not wrong, "thread %d: calls %s differ from the single-threaded result" % (i, wrong)
