"""The multi-GPU exchange kernels (okm_dist.hip: k_pack_counts, k_pack_deltas,
k_widen_counts, k_widen_deltas, k_apply_escapes, k_apply_key_escapes, the
per-slice scans and the piece cutting) at their byte and slice edges, through
the product path: every rank's local table is given as exact (key, count)
pairs (add_pairs), merged by okm_merge_owned / okm_merge_owned_n over P
virtual ranks of a loopback communicator -- and, for a subset, over real RCCL
at one rank with owner == local -- and compared, exactly, with the numpy
restatement of tests/exchange_cases.py: each owner's table, n_owned, and the
(sent, received) bytes of Comm.last_bytes(), which show an escape that is sent
needlessly or dropped even where the final table would hide it.  The cases and
what each pins: tests/exchange_cases.py, self-checked on the CPU by
tests/test_exchange_cases.py."""

import numpy as np
import pytest

import exchange_cases as ec
import okm
from okm import testing
from loopback_ranks import _loopback_timeout, run_ranks  # noqa: F401  (the 60 s loopback timeout)

pytestmark = pytest.mark.gpu


def _merge_on(comm, case, r, made):
    """Rank r's side of the case on its communicator: (tables of every owner
    context, n_owned per table, last_bytes).  The contexts go to `made`: the
    caller closes them once EVERY rank has returned (known
    issue: a context torn down beside another context's count)."""
    sets = ec.table_sets(case)
    locals_, owners = [], []
    for ts in sets:
        local = okm.KmerCounter(case.k, case.mode, wide=case.wide)
        made.append(local)
        locals_.append(local)
        if case.owner_mode == "local":
            owners.append(local)
        else:
            owners.append(okm.KmerCounter(case.k, case.mode, wide=case.wide))
            made.append(owners[-1])
        keys, counts = ts[r]
        if len(keys):
            local.add_pairs(ec.to_pairs(keys) if case.wide else keys, counts)
    if len(sets) == 1:
        n_owned = [comm.merge_owned(locals_[0], owners[0])]
    else:
        n_owned = comm.merge_owned_n(locals_, owners)
    return [o.result(1) for o in owners], n_owned, comm.last_bytes()


def run_case(case, deltas):
    """The case over P loopback ranks; deltas: 0 / 1 forces the key wire
    format, None leaves the choice to the library."""
    for name, value in case.knobs.items():
        testing.set_knob(name, value)
    testing.set_knob("wire_deltas", -1 if deltas is None else deltas)
    comms = okm.Comm.init_loopback(case.P, 0)
    made = []
    try:
        return run_ranks(case.P, lambda r: _merge_on(comms[r], case, r, made))
    finally:
        for c in made:
            c.close()
        for c in comms:
            c.close()


def check_tables(case, res):
    """Every owner's keys and counts, n_owned, and the ranges in rank order."""
    for t in range(len(ec.table_sets(case))):
        want = ec.expected_tables(case, t)
        last = -1
        for r, (ek, ecnt) in enumerate(want):
            (gk, gc), n_owned = res[r][0][t], res[r][1][t]
            if case.wide:
                assert np.array_equal(gk.reshape(-1, 2), ec.to_pairs(ek)), (case.name, t, r)
                got = ec.from_pairs(gk)
            else:
                assert np.array_equal(gk, ek), (case.name, t, r)
                got = [int(v) for v in gk]
            if case.mode == "count":
                assert np.array_equal(gc, ecnt), (case.name, t, r)
            assert n_owned == len(ek), (case.name, t, r)
            if got:  # the ranges concatenated in rank order are strictly ascending
                assert last < got[0] and all(a < b for a, b in zip(got, got[1:]))
                last = got[-1]


def check(case, res, deltas):
    check_tables(case, res)
    assert [r[2] for r in res] == ec.expected_bytes(case, deltas), (case.name, deltas)


def same_tables(a, b):
    for ra, rb in zip(a, b):
        for (ka, ca), (kb, cb) in zip(ra[0], rb[0]):
            assert np.array_equal(ka, kb) and np.array_equal(ca, cb)
        assert ra[1] == rb[1]


@pytest.mark.parametrize("name", ec.names())
def test_exchange_case(name):
    """Groups 1 to 11: tables, n_owned and wire bytes exact in both key wire
    formats (K128 keys never travel as deltas: the knob must not change their
    bytes), and the two formats' tables identical."""
    case = ec.get(name)
    res = {}
    for deltas in (1, 0):
        res[deltas] = run_case(case, deltas)
        check(case, res[deltas], deltas)
    same_tables(res[0], res[1])


@pytest.mark.parametrize("name", ec.AUTO_FORMAT)
def test_exchange_automatic_format(name):
    """Group 12: no wire_deltas knob.  Which format the library picks is a
    tuning heuristic; every rank must pick the same, and report its bytes."""
    case = ec.get(name)
    res = run_case(case, None)
    check_tables(case, res)
    got = [r[2] for r in res]
    assert got in (ec.expected_bytes(case, 0), ec.expected_bytes(case, 1)), (case.name, got)


@pytest.fixture(scope="module")
def comm1():
    c = okm.Comm(1, 0, okm.comm_unique_id(), 0)
    assert c.rank == 0 and c.size == 1
    yield c
    c.close()


@pytest.mark.parametrize("name", ec.names("single"))
def test_exchange_single_rank_rccl(comm1, name):
    """One rank over real RCCL with owner == local: the general path with a
    self send/recv, so every pack, widen, escape and scan kernel runs with
    P = 1 and cut = [0, n] through the RCCL transport.  last_bytes() counts
    traffic with OTHER ranks only, so it is (0, 0) here whatever is sent: at
    one rank a needless or dropped escape can show in the table alone, and
    the byte counts are pinned by the loopback cases."""
    case = ec.get(name)
    assert comm1.info()["transport"] == "rccl"
    res = {}
    for deltas in (1, 0):
        for knob, value in case.knobs.items():
            testing.set_knob(knob, value)
        testing.set_knob("wire_deltas", deltas)
        made = []
        try:
            res[deltas] = [_merge_on(comm1, case, 0, made)]
        finally:
            for c in made:
                c.close()
        check(case, res[deltas], deltas)
    same_tables(res[0], res[1])
