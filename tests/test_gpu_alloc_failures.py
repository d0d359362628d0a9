"""Every device allocation of a count, failed in turn (the test hook
fail_alloc: the n-th allocation from the context's arena returns OKM_E_NOMEM
before anything is taken or mapped -- a host-side status, no launch).

The arena holds nothing but runs, the result and its pending state between
calls, so after okm_reset it must be empty whatever failed: a step that
strands a block on an error path (okm_engine.hip Blocks) shows as
device_in_use > 0.  One long-lived context runs the whole sweep of a
configuration, since that is the case that matters: it keeps what a failed
attempt stranded until it is destroyed.

Per configuration: a clean run (exact against the oracle; it counts the
allocations, N <= 256), then for EVERY n in 1..N the same calls with the n-th
allocation failing.  Either every call returns OK -- the engine recovered (the
host tier of do_count, or a path with a fallback of its own: a batch's L1 run
taken again by l1_batch_or_spill, the dense copy made in host memory, the
pipelined groups' device word) and the table is exact -- or a call fails with
OKM_E_NOMEM / OKM_E_STATE.  In both cases the arena is empty after a reset,
no host table is left, and the same calls once more are exact.  Which
recoveries went without a spill is printed, not asserted: from here an
allocation is a number, and which path it belongs to is not visible."""

import numpy as np
import pytest

import okm
from okm import testing
from oracle import OracleCounter, OracleCounterWide

pytestmark = pytest.mark.gpu

BIG = 10**9


def _upload(arr):
    arr = np.ascontiguousarray(arr)
    buf = okm.DeviceBuffer(max(arr.nbytes, 8))
    if arr.nbytes:
        buf.upload(arr)
    return buf


@pytest.fixture(scope="module")
def batches():
    """Two small batches (~0.3 M windows each) in host and device memory, and
    a third whose L1 parts outgrow one count item (4096 instances), so that the
    partition passes run: ~3 M windows of a 2 kbp genome, a few hot keys per
    part, which one pass does not always separate (fan-out, host rounds)."""
    host = [okm.synth_reads(4_000, 100, genome_len=200_000, genome_seed=7, seed=s) for s in (7, 8)]
    host.append(okm.synth_reads(40_000, 100, genome_len=2_000, genome_seed=7, seed=9))
    dev = [_upload(h) for h in host]
    yield host, dev
    for b in dev:
        b.free()


_oracles = {}


def _oracle(k, host, which):
    """The oracle's table of the batches host[i], i in `which` (computed once)."""
    key = (k, tuple(which))
    if key not in _oracles:
        oc = OracleCounterWide(k) if k > 32 else OracleCounter(k)
        for i in which:
            oc.add_separated(host[i])
        _oracles[key] = oc.result(1)
    return _oracles[key]


def _same(got, expect):
    return np.array_equal(got[0], expect[0]) and np.array_equal(got[1], expect[1])


def _sweep(ctr, knobs, run, expect, min_levels=0):
    """run(ctr) -> (keys, counts) under `knobs`, with every allocation failed
    in turn; the clean run takes at least `min_levels` partition passes."""

    def attempt(fail):
        ctr.reset()
        for name, v in knobs.items():
            testing.set_knob(name, v)
        testing.set_knob("fail_alloc", fail)
        try:
            return run(ctr), None
        except okm.OkmError as e:
            return None, e
        finally:
            left[0] = testing.get_knob("fail_alloc")
            testing.set_knob("fail_alloc", -1)

    def assert_empty(what):
        ctr.reset()
        assert testing.device_in_use(ctr) == 0, what
        assert ctr.engine_info()["host_bytes"] == 0, what

    left = [0]
    got, err = attempt(BIG)
    assert err is None and _same(got, expect), "clean run"
    n_gets = BIG - left[0]
    assert ctr.engine_info()["levels"] >= min_levels, ctr.engine_info()
    print(f"clean run: {n_gets} allocations")
    assert_empty("clean run")
    assert 0 < n_gets <= 256, n_gets
    recovered, no_spill = [], []
    for n in range(1, n_gets + 1):
        got, err = attempt(n)
        spills = ctr.engine_info()["spills"]
        if err is None:
            assert left[0] == -1, f"allocation {n}: the failure did not fire"
            assert _same(got, expect), f"allocation {n}: recovered, but the table differs"
            recovered.append(n)
            if not spills:
                no_spill.append(n)
        else:
            assert err.status in (okm._lib.OKM_E_NOMEM, okm._lib.OKM_E_STATE), (n, err)
        assert_empty(f"after allocation {n} failed")
        got, err = attempt(-1)
        assert err is None and _same(got, expect), f"clean run after allocation {n} failed"
    print(f"recovered at {len(recovered)} of {n_gets}; without a spill (a fallback of the path's own) at {no_spill}")


def _one_batch(dev, host, i=0):
    def run(ctr):
        ctr.add_device_batch(dev[i].address, len(host[i]))
        return ctr.result(1)
    return run


def _two_counts(dev, host):
    # add -> count -> add -> count: the kept table becomes a folded run beside the new batch
    def run(ctr):
        ctr.add_device_batch(dev[0].address, len(host[0]))
        ctr.count()
        ctr.add_device_batch(dev[1].address, len(host[1]))
        return ctr.result(1)
    return run


# (k, knobs, batch, partition passes the clean run takes at least).  At the
# small batches' size no L1 part is split, so the partition passes (split_launch,
# the fan-out, the host rounds of count_parts) run on the third batch: 3-bit
# passes take host rounds there, 1-bit passes the fan-out and host rounds.
ONE_BATCH = [
    pytest.param(31, {}, 0, 0, id="k31-defaults"),
    pytest.param(31, {"group_keys": 100_000, "group_exact": 0}, 0, 0, id="k31-groups-bound-table"),
    pytest.param(31, {"group_keys": 100_000, "group_exact": 0, "group_over": 1}, 0, 0, id="k31-groups-over-the-run"),
    pytest.param(31, {"group_keys": 100_000, "group_exact": 1}, 0, 0, id="k31-groups-exact-tables"),
    pytest.param(27, {"part_max_bits": 3}, 0, 0, id="k27-small-passes-no-split"),
    pytest.param(27, {"part_max_bits": 3}, 2, 2, id="k27-host-rounds"),
    pytest.param(27, {"part_max_bits": 1}, 2, 2, id="k27-fan-out-host-rounds"),
    pytest.param(45, {"group_keys": 100_000}, 0, 0, id="k45-direct-count"),
]


@pytest.mark.parametrize("k,knobs,batch,min_levels", ONE_BATCH)
def test_one_batch_every_allocation_fails_in_turn(batches, k, knobs, batch, min_levels):
    host, dev = batches
    with okm.KmerCounter(k, wide=k > 32) as ctr:
        _sweep(ctr, knobs, _one_batch(dev, host, batch), _oracle(k, host, [batch]), min_levels)


@pytest.mark.parametrize("k", [31, 45])
def test_kept_table_and_new_batch_every_allocation_fails_in_turn(batches, k):
    host, dev = batches
    with okm.KmerCounter(k, wide=k > 32) as ctr:
        _sweep(ctr, {}, _two_counts(dev, host), _oracle(k, host, [0, 1]))


@pytest.mark.parametrize("sorted_path", [-1, 1, 2])
def test_sorted_runs_every_allocation_fails_in_turn(batches, sorted_path):
    # two halves counted separately; their device tables merged by a third
    # context (okm_add_sorted_pairs_device): staged count, merge kernel, two-pass count
    host, dev = batches
    k = 31
    halves, bufs = [], []
    for i in range(2):
        with okm.KmerCounter(k) as c:
            c.add_device_batch(dev[i].address, len(host[i]))
            tk, tc = c.result(1)
        halves.append((_upload(tk), _upload(tc), len(tc)))
        bufs += halves[-1][:2]

    def run(ctr):
        for bk, bc, n in halves:
            ctr.add_sorted_pairs_device(bk.address, bc.address, n)
        return ctr.result(1)

    with okm.KmerCounter(k) as ctr:
        _sweep(ctr, {"sorted_path": sorted_path}, run, _oracle(k, host, [0, 1]))
    for b in bufs:
        b.free()


def test_host_pairs_every_allocation_fails_in_turn(batches):
    # okm_add_pairs from host arrays with counts (partition_pairs), then the count
    host, _ = batches
    k = 31
    ek, ec = _oracle(k, host, [0])
    oc = OracleCounter(k)
    oc.add_pairs(ek, ec)
    oc.add_pairs(ek[::2], ec[::2])

    def run(ctr):
        ctr.add_pairs(ek, ec)
        ctr.add_pairs(ek[::2].copy(), ec[::2].copy())
        return ctr.result(1)

    with okm.KmerCounter(k) as ctr:
        _sweep(ctr, {}, run, oc.result(1))
