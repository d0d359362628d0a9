"""P virtual ranks of a loopback communicator on P host threads (not a test
file: shared by tests/test_gpu_loopback.py and
tests/test_gpu_exchange_edges.py)."""

import threading

import pytest

from okm import testing


@pytest.fixture(autouse=True)
def _loopback_timeout():
    """A rank that never arrives ends a collective after 60 s, not 300 (the
    conftest resets every knob after each test)."""
    testing.set_knob("loopback_timeout_ms", 60_000)
    yield


def run_ranks(P, fn):
    """fn(rank) on P threads (one per virtual rank); returns the results in
    rank order, re-raising the first exception."""
    out, err = [None] * P, [None] * P

    def body(r):
        try:
            out[r] = fn(r)
        except BaseException as e:  # surfaced below
            err[r] = e

    th = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
        assert not t.is_alive(), "a virtual rank hung"
    for e in err:
        if e is not None:
            raise e
    return out
