"""okm_lookup_counts (the counts of given k-mers) on the device, exact against
a plain lookup in numpy's (or the oracle's) table: counts[i] = the count of
query i, 0 where it is absent, and n_found = the queries that were present.
The inputs are tests/lookup_cases.py's (self-checked on the CPU by
tests/test_lookup_cases.py).

The table is searched where it lies -- a count's pending per-item runs (u32 or
u64 counts), a dense device table, a host-resident table in slices -- and must
stay there: the run's own kernel statistics show no gather ("compact_items"),
and every later reader gives the exact table.  Every case is looked up twice,
with host queries and with device queries, and both check n_found."""

import ctypes
import gzip
import os
import subprocess
import threading
from functools import lru_cache

import numpy as np
import pytest

import hist_cases as hc
import lookup_cases as lc
import okm
from conftest import GOLDEN
from okm import _lib, testing
from oracle import OracleCounter, OracleCounterWide

pytestmark = pytest.mark.gpu

K = lc.K
BIG = 10**9


def _upload(arr):
    arr = np.ascontiguousarray(arr, dtype=np.uint64)
    buf = okm.DeviceBuffer(max(arr.nbytes, 8))
    if arr.nbytes:
        buf.upload(arr)
    return buf


def _same(got, expect):
    return np.array_equal(got[0], expect[0]) and np.array_equal(got[1], expect[1])


def _host(c, q):
    """(counts, n_found) of host queries q (one-word, or (n, 2) pairs)."""
    q = np.ascontiguousarray(q, dtype=np.uint64)
    n = q.size // 2 if c.wide else q.size
    out = np.full(n, 77, np.uint64)  # every entry is written, absent ones with 0
    found = ctypes.c_uint64(99)
    _lib.check(_lib.load().okm_lookup_counts(c.ctx, q.ctypes.data, n, out.ctypes.data, 0, ctypes.byref(found)),
               "okm_lookup_counts")
    assert np.array_equal(out, c.lookup(q))  # the Python wrapper, n_found = NULL
    return out, found.value


def _device(c, q):
    q = np.ascontiguousarray(q, dtype=np.uint64)
    n = q.size // 2 if c.wide else q.size
    dq, dc = _upload(q), _upload(np.full(max(n, 1), 77, np.uint64))
    try:
        found = c.lookup_device(dq.address, n, dc.address)
        out = np.empty(n, np.uint64)
        if n:
            dc.download(out)
        return out, found
    finally:
        dq.free()
        dc.free()


def _check(c, ek, ec, q):
    """Host and device lookups of q against the one-word table (ek, ec)."""
    exp, found = lc.expected(ek, ec, q)
    for got in (_host(c, q), _device(c, q)):
        assert got[0].dtype == np.uint64 and np.array_equal(got[0], exp)
        assert got[1] == found
    return exp


def _check_wide(c, table, queries):
    exp, found = lc.expected_wide(table, queries)
    q = lc.to_pairs(queries)
    for got in (_host(c, q), _device(c, q), _host(c, q.reshape(-1))):  # (n, 2) or flat 2n
        assert np.array_equal(got[0], exp) and got[1] == found
    return exp


def _launches(c, name):
    return c.kernel_stats().get(name, {"launches": 0})["launches"]


# ---------------------------------------------------------------------------
# pending table (the count's own runs), then the dense table
# ---------------------------------------------------------------------------

def _pending_then_dense(keys, q, k=K):
    ek, ec = hc.table_of(keys)
    with okm.KmerCounter(k) as c:
        c.set_timing(True)
        c.add_pairs(keys)
        assert c.count() == len(ek)
        first = _check(c, ek, ec, q)
        stats = c.kernel_stats()
        assert stats["lookup_counts"]["launches"] == 3, sorted(stats)  # _host looks up twice, _device once
        assert stats["lookup_counts"]["alg_bytes"] == 3 * 16.0 * len(q)  # the queries in, the counts out
        assert "compact_items" not in stats, sorted(stats)  # the pending table was not gathered
        assert _same(c.result(1), (ek, ec))  # the reader after it: exact, and it gathers
        assert _launches(c, "compact_items") == 1
        second = _check(c, ek, ec, q)  # now over the dense table
        assert np.array_equal(first, second)
        assert _launches(c, "lookup_counts") == 6 and _launches(c, "compact_items") == 1
        assert _same(c.result(1), (ek, ec))


def test_pending_item_edges():
    runs, inp = lc.items()
    q = lc.edge_queries(runs)
    _pending_then_dense(inp, q)
    every = np.concatenate(runs)
    _pending_then_dense(inp, np.concatenate([every, every + np.uint64(1), q]))  # every key, and beside every key


@pytest.mark.parametrize("m", hc.ITEM_SIZES)
def test_pending_one_item_between_two_ranges(m):
    """hist_cases.one_item: m keys under one prefix between two populated
    ranges; m = 0 is an empty key range that the queries fall into."""
    keys = hc.one_item(m)
    ek = np.unique(keys)
    mid = ek[(ek >> np.uint64(hc.LOW_BITS)) == (hc.PREFIX >> np.uint64(hc.LOW_BITS))]
    assert len(mid) == m
    q = [hc.PREFIX, hc.PREFIX | np.uint64((1 << hc.LOW_BITS) - 1), hc.PREFIX - np.uint64(1), hc.PREFIX_ABOVE,
         ek[0], ek[-1], ek[0] - np.uint64(1), ek[-1] + np.uint64(1)]
    if m:
        q += [mid[0], mid[-1], mid[0] - np.uint64(1), mid[-1] + np.uint64(1), mid[m // 2]]
    _pending_then_dense(keys, np.array(q, np.uint64))


def test_pending_many_items():
    keys = hc.many_items()
    ek = np.unique(keys)
    rng = np.random.default_rng(5)
    q = np.concatenate([ek, ek + np.uint64(1), ek - np.uint64(1), rng.integers(0, 1 << 62, 5000, dtype=np.uint64)])
    _pending_then_dense(keys, q)


@pytest.mark.parametrize("with_zero", [True, False])
def test_k32_zero_and_all_ones(with_zero):
    keys = lc.k32_table(with_zero)
    ek = np.unique(keys)
    q = np.array([0, lc.M64, 1, lc.M64 - 1, ek[0], ek[-1], ek[-1] + np.uint64(1), ek[1] - np.uint64(1)], np.uint64)
    _pending_then_dense(keys, q, k=32)
    exp, found = lc.expected(*hc.table_of(keys), q)
    assert exp[0] == (3 if with_zero else 0) and exp[1] == 0


def test_pending_u32_counts_from_reads():
    """A count from reads stages u32 counts."""
    batch = okm.synth_reads(20_000, 100, genome_len=300_000, genome_seed=5, seed=5)
    oc = OracleCounter(K)
    oc.add_separated(batch)
    ek, ec = oc.result(1)
    rng = np.random.default_rng(7)
    q = rng.permutation(np.concatenate([ek[::3], ek[::7] + np.uint64(1),
                                        rng.integers(0, 1 << 62, 3000, dtype=np.uint64)]))
    buf = okm.DeviceBuffer(len(batch), 0)
    buf.upload(batch)
    try:
        with okm.KmerCounter(K) as c:
            c.set_timing(True)
            c.add_device_batch(buf.address, len(batch))
            exp = _check(c, ek, ec, q)  # counts first, as okm_result_size does
            assert int(exp.max()) >= 2 and (exp == 0).sum() > 3000
            assert "compact_items" not in c.kernel_stats()
            assert _same(c.result(1), (ek, ec))
            _check(c, ek, ec, q)
    finally:
        buf.free()


# ---------------------------------------------------------------------------
# counts past 2^32
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("k", [31, 45])
def test_counts_past_u32(k):
    wide = k > 32
    runs, (ek, ec) = hc.past_u32_runs()
    big = ek[ec >= np.uint64(1 << 32)]
    assert sorted(int(x) for x in ec[ec >= np.uint64(1 << 32)]) == [5_000_000_000, 6_000_000_000]
    q = np.concatenate([big, big + np.uint64(1), ek[:2000], ek[-3:], [np.uint64(1 << 41)]]).astype(np.uint64)
    bufs = []
    try:
        with okm.KmerCounter(k, wide=wide) as m:
            for keys, counts in runs:
                kk = np.stack([keys, np.zeros_like(keys)], axis=1).reshape(-1) if wide else keys
                bk, bc = _upload(kk), _upload(counts)
                bufs += [bk, bc]
                m.add_sorted_pairs_device(bk.address, bc.address, len(keys))
            for _ in range(2):  # as the count leaves the table, then after a reader
                if wide:
                    exp = _check_wide(m, dict(zip((int(x) for x in ek), (int(x) for x in ec))), [int(x) for x in q])
                else:
                    exp = _check(m, ek, ec, q)
                assert sorted(int(x) for x in exp[:2]) == [5_000_000_000, 6_000_000_000]
                gk, gc = m.result(1)
                if wide:
                    gk = gk.reshape(-1, 2)[:, 0]
                assert _same((gk, gc), (ek, ec))
    finally:
        for b in bufs:
            b.free()


# ---------------------------------------------------------------------------
# query counts and orders
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def items_counter():
    runs, inp = lc.items()
    c = okm.KmerCounter(K)
    c.add_pairs(inp)
    ek, ec = hc.table_of(inp)
    assert c.count() == len(ek)
    yield c, ek, ec
    c.close()


@pytest.mark.parametrize("n", lc.QUERY_COUNTS + (lc.BLOCK_QUERIES - 1, lc.BLOCK_QUERIES, lc.BLOCK_QUERIES + 1))
def test_query_counts(items_counter, n):
    c, ek, ec = items_counter
    rng = np.random.default_rng(n)
    q = rng.permutation(np.concatenate([ek[: n // 2], ek[: n - n // 2] + np.uint64(1)]))[:n]
    assert len(q) == n
    exp = _check(c, ek, ec, q)
    assert len(exp) == n


def test_no_queries_touch_nothing(items_counter):
    c, ek, ec = items_counter
    lib = _lib.load()
    found = ctypes.c_uint64(5)
    assert lib.okm_lookup_counts(c.ctx, None, 0, None, 0, ctypes.byref(found)) == _lib.OKM_OK and found.value == 0
    assert lib.okm_lookup_counts(c.ctx, None, 0, None, 1, None) == _lib.OKM_OK
    assert len(c.lookup(np.zeros(0, np.uint64))) == 0


def test_host_queries_cross_the_upload_chunk(items_counter):
    c, ek, ec = items_counter
    n = lc.CHUNK + 300
    rng = np.random.default_rng(11)
    q = ek[rng.integers(0, len(ek), n)]
    q[::5] += np.uint64(1)
    q[lc.CHUNK - 2:lc.CHUNK + 2] = [ek[0], ek[-1], ek[0] - np.uint64(1), ek[1]]  # around the chunk's edge
    q[-1] = ek[-1]
    exp, found = lc.expected(ek, ec, q)
    got = _host(c, q)
    assert np.array_equal(got[0], exp) and got[1] == found and 0 < found < n
    got = _device(c, q)
    assert np.array_equal(got[0], exp) and got[1] == found


def test_query_orders(items_counter):
    c, ek, ec = items_counter
    rng = np.random.default_rng(13)
    some = np.sort(np.concatenate([ek[::9], ek[::9] + np.uint64(1)]))
    for q in (np.full(3000, ek[100]),                      # all the same present key
              np.full(3000, ek[100] + np.uint64(1)),       # ... and the same absent one
              some, some[::-1].copy(),                     # sorted, reversed
              np.repeat(some[:700], 3), rng.permutation(np.repeat(some[:700], 3))):  # duplicated
        exp = _check(c, ek, ec, q)
        assert len(exp) == len(q)
    assert lc.expected(ek, ec, np.full(3000, ek[100]))[1] == 3000


# ---------------------------------------------------------------------------
# wide keys (k in 33..64)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("k", lc.WIDE_KS)
def test_wide_word_neighbours(k):
    table, queries = lc.word_neighbours(k)
    keys = sorted(table)
    with okm.KmerCounter(k, wide=True) as c:
        c.set_timing(True)
        c.add_pairs(lc.table_input(table))
        assert c.count() == len(table)
        before = _launches(c, "compact_items")
        first = _check_wide(c, table, queries)
        assert _launches(c, "compact_items") == before  # the lookup itself gathered nothing
        gk, gc = c.result(1)
        assert lc.from_pairs(gk) == keys and [int(x) for x in gc] == [table[v] for v in keys]
        assert np.array_equal(_check_wide(c, table, queries), first)


@lru_cache(maxsize=None)
def _ont(k):
    batch, _lens = okm.synth_long_reads(0.0006, 100_000, genome_seed=6, seed=6, median_len=300.0, min_len=100,
                                        max_len=3000)
    oc = OracleCounterWide(k)
    oc.add_separated(batch)
    ek, ec = oc.result(1)
    ints = lc.from_pairs(ek)
    table = dict(zip(ints, (int(x) for x in ec)))
    queries = []
    for v in ints[::23]:
        queries += [v, (v - 1) & lc.M128, (v + 1) & lc.M128, (v - (1 << 64)) & lc.M128, (v + (1 << 64)) & lc.M128]
    queries += [0, lc.M128, ints[0], ints[-1], ints[0] - 1 if ints[0] else 0, ints[-1] + 1]
    return batch, (ek, ec), table, queries


WIDE_PATHS = {
    "direct": {},
    "groups_bound_table": {"group_keys": 50_000, "group_exact": 0},
    "groups_exact_tables": {"group_keys": 50_000, "group_exact": 1},
}


@pytest.mark.parametrize("path", list(WIDE_PATHS))
@pytest.mark.parametrize("k", lc.WIDE_KS)
def test_wide_paths(k, path):
    batch, expect, table, queries = _ont(k)
    assert 1000 < len(table) and max(table.values()) >= 3
    for name, v in WIDE_PATHS[path].items():
        testing.set_knob(name, v)
    buf = okm.DeviceBuffer(len(batch), 0)
    buf.upload(batch)
    try:
        with okm.KmerCounter(k, wide=True) as c:
            c.set_timing(True)
            c.add_device_batch(buf.address, len(batch))
            c.count()
            before = _launches(c, "compact_items")
            exp = _check_wide(c, table, queries)
            assert int(exp.max()) >= 2 and (exp == 0).sum() > len(queries) // 2
            assert _launches(c, "compact_items") == before  # the lookup itself gathered nothing
            if path != "direct":
                assert c.engine_info()["groups"] >= 3, c.engine_info()
            assert _same(c.result(1), expect)
    finally:
        buf.free()


# ---------------------------------------------------------------------------
# host-resident table: keys and counts go up in slices
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_batch():
    batch = okm.synth_reads(8_000, 100, genome_len=150_000, genome_seed=8, seed=8)
    oc = OracleCounter(K)
    oc.add_separated(batch)
    buf = okm.DeviceBuffer(len(batch), 0)
    buf.upload(batch)
    yield batch, buf, oc.result(1)
    buf.free()


def _to_host_table(c, expect):
    """The dense gather's first allocation fails: the table is gathered into
    mapped host memory and stays there."""
    testing.set_knob("fail_alloc", 1)
    assert _same(c.result(1), expect)
    assert testing.get_knob("fail_alloc") == -1, "the failure did not fire"
    assert c.engine_info()["host_bytes"] > 0


def _slice_queries(ek, sl):
    """The last key of every slice, the first key of the next and an absent key between them."""
    q = [ek[0], ek[-1], ek[0] - np.uint64(1), ek[-1] + np.uint64(1)]
    for e in range(sl, len(ek), sl):
        q += [ek[e - 1], ek[e], ek[e - 1] + (ek[e] - ek[e - 1]) // np.uint64(2)]  # (the gap's middle; the key itself if adjacent)
    return np.array(q, np.uint64)


def test_host_resident_table_in_slices(small_batch):
    batch, buf, (ek, ec) = small_batch
    assert len(ek) > 3 * 4096 and len(ek) % 1000 and len(ek) % 4096
    rng = np.random.default_rng(17)
    with okm.KmerCounter(K) as c:
        c.set_timing(True)
        c.add_device_batch(buf.address, len(batch))
        c.count()
        _to_host_table(c, (ek, ec))
        launches = 0
        for sl in (1000, 4096, len(ek)):  # a ragged last slice, several slices, exactly one
            testing.set_knob("hist_slice", sl)
            q = np.concatenate([_slice_queries(ek, sl), rng.permutation(ek)[:2000],
                                rng.integers(0, 1 << 62, 500, dtype=np.uint64)])
            exp = _check(c, ek, ec, q)
            assert (exp == 0).sum() >= 500
            launches += 3 * -(-len(ek) // sl)  # one per slice, for two host lookups and a device one
            assert _launches(c, "lookup_counts") == launches
            assert c.engine_info()["host_bytes"] > 0  # still host-resident
        testing.set_knob("hist_slice", -1)  # the product's slice: one here
        _check(c, ek, ec, _slice_queries(ek, 4096))
        assert "compact_items" in c.kernel_stats() and _launches(c, "compact_items") == 1  # _to_host_table's
        assert c.engine_info()["host_bytes"] > 0
        assert _same(c.result(1), (ek, ec))
        assert c.engine_info()["host_bytes"] > 0


# ---------------------------------------------------------------------------
# every allocation of the lookup fails in turn
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("state", ["pending", "dense", "host"])
def test_every_allocation_fails_in_turn(small_batch, state):
    batch, buf, expect = small_batch
    ek, ec = expect
    q = np.concatenate([ek[::11], ek[::13] + np.uint64(1)])
    exp, found = lc.expected(ek, ec, q)

    def prepare(c):
        c.reset()
        c.add_device_batch(buf.address, len(batch))
        c.count()
        if state == "dense":
            assert _same(c.result(1), expect)
        elif state == "host":
            _to_host_table(c, expect)
            testing.set_knob("hist_slice", 5000)

    def attempt(c, fail):
        testing.set_knob("fail_alloc", fail)
        try:
            return c.lookup(q), None
        except okm.OkmError as e:
            return None, e
        finally:
            left[0] = testing.get_knob("fail_alloc")
            testing.set_knob("fail_alloc", -1)

    left = [0]
    with okm.KmerCounter(K) as c:
        prepare(c)
        got, err = attempt(c, BIG)
        assert err is None and np.array_equal(got, exp)
        n_gets = BIG - left[0]
        print(f"{state}: {n_gets} allocations")
        # the found word, the host queries' two buffers; the pending index's four arrays / the slice's two
        assert n_gets == {"pending": 7, "dense": 3, "host": 5}[state]
        for n in range(1, n_gets + 1):
            prepare(c)
            in_use = testing.device_in_use(c)
            got, err = attempt(c, n)
            assert left[0] == -1, f"allocation {n}: the failure did not fire"
            if err is None:
                assert np.array_equal(got, exp)
            else:
                assert err.status == _lib.OKM_E_NOMEM, (n, err)
            assert testing.device_in_use(c) == in_use, f"allocation {n}: a block was stranded"
            if state == "host":
                assert c.engine_info()["host_bytes"] > 0
            again = _host(c, q)  # the table is intact: again, cleanly
            assert np.array_equal(again[0], exp) and again[1] == found
            assert _same(c.result(1), expect)
            c.reset()
            assert testing.device_in_use(c) == 0 and c.engine_info()["host_bytes"] == 0


# ---------------------------------------------------------------------------
# other states
# ---------------------------------------------------------------------------

def test_before_any_batch_is_all_zeros():
    q = np.array([0, 5, 1 << 61], np.uint64)
    with okm.KmerCounter(K) as c:
        for got in (_host(c, q), _device(c, q)):  # the caller's buffer is zeroed, whatever it held
            assert got[0].tolist() == [0, 0, 0] and got[1] == 0
    with okm.KmerCounter(40, wide=True) as c:
        got = _host(c, lc.to_pairs([0, 5, 1 << 70]))
        assert got[0].tolist() == [0, 0, 0] and got[1] == 0


def test_null_arguments(items_counter):
    c, ek, ec = items_counter
    lib = _lib.load()
    buf = np.zeros(4, np.uint64)
    assert lib.okm_lookup_counts(c.ctx, None, 4, buf.ctypes.data, 0, None) == _lib.OKM_E_ARG
    assert lib.okm_lookup_counts(c.ctx, buf.ctypes.data, 4, None, 0, None) == _lib.OKM_E_ARG
    assert lib.okm_lookup_counts(c.ctx, None, 4, None, 1, None) == _lib.OKM_E_ARG
    assert lib.okm_lookup_counts(None, buf.ctypes.data, 4, buf.ctypes.data, 0, None) == _lib.OKM_E_ARG
    with pytest.raises(ValueError):
        with okm.KmerCounter(40, wide=True) as w:
            w.lookup(np.zeros(3, np.uint64))
    _check(c, ek, ec, ek[:10])  # the table is as it was


def test_set_mode_has_no_counts():
    with okm.KmerCounter(K, "set") as c:
        c.add_pairs(np.arange(1, 100, dtype=np.uint64))
        with pytest.raises(okm.OkmError) as ei:
            c.lookup(np.arange(1, 5, dtype=np.uint64))
        assert ei.value.status == _lib.OKM_E_STATE
        keys, _ = c.result(1)
        assert np.array_equal(keys, np.arange(1, 100, dtype=np.uint64))


def test_folded_table():
    """count, then add: the first table becomes a weighted run of the second count."""
    a, b = hc.fold_pairs()
    ek, ec = hc.table_of(np.concatenate([a, b]))
    ak, ac = hc.table_of(a)
    q = np.concatenate([ek[::5], ek[::7] + np.uint64(1)])
    with okm.KmerCounter(K) as c:
        c.add_pairs(a)
        c.count()
        exp_a = _check(c, ak, ac, q)
        c.add_pairs(b)
        exp = _check(c, ek, ec, q)  # counts the pending batch first
        assert not np.array_equal(exp_a, exp)
        assert _same(c.result(1), (ek, ec))


def test_count_add_records_count():
    rng = np.random.default_rng(41)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rng.integers(0, 4, 5000)]
    reads = [genome[o:o + 90].tobytes() for o in rng.integers(0, 4900, 1500)]
    oc = OracleCounter(K)
    with okm.KmerCounter(K) as c:
        c.add_records(reads[:700])
        oc.add_records(reads[:700])
        c.count()
        ek, ec = oc.result(1)
        q = np.concatenate([ek, ek[::3] + np.uint64(1)])
        _check(c, ek, ec, q)
        c.add_records(reads[700:])
        oc.add_records(reads[700:])
        c.count()
        ek, ec = oc.result(1)
        _check(c, ek, ec, np.concatenate([q, ek[::2]]))
        assert _same(c.result(1), (ek, ec))


# ---------------------------------------------------------------------------
# groups and owners
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def group_reads():
    n, read_len = 12_000, 100
    batch = okm.synth_reads(n, read_len, genome_len=200_000, genome_seed=9, seed=9)
    recs = batch.reshape(n, read_len + 1)
    recs[::50, :read_len] = ord("A")  # a hot key
    batch = np.ascontiguousarray(recs).reshape(-1)
    oc = OracleCounter(K)
    oc.add_separated(batch)
    ek, ec = oc.result(1)
    rng = np.random.default_rng(19)
    q = rng.permutation(np.concatenate([ek[::4], ek[::9] + np.uint64(1), [np.uint64(0)],
                                        rng.integers(0, 1 << 62, 2000, dtype=np.uint64)]))
    with okm.KmerCounter(K) as c:  # the one-context answer for the same reads
        buf = okm.DeviceBuffer(len(batch), 0)
        buf.upload(batch)
        c.add_device_batch(buf.address, len(batch))
        one = _check(c, ek, ec, q)
        buf.free()
    assert one[np.flatnonzero(q == 0)[0]] == ec[0] > 100  # poly-A, the hot key
    return recs, q, one, lc.expected(ek, ec, q)[1]


def test_group_of_one_gpu(group_reads):
    """okm_group_lookup_counts through a real group (one context per GPU; this
    test has one GPU: more ranks are covered through the loopback owners
    below, since a group of N needs N devices)."""
    recs, q, one, found = group_reads
    lib = _lib.load()
    g = ctypes.c_void_p()
    _lib.check(lib.okm_group_create(ctypes.byref(g), K, 0, 1, None, 0), "okm_group_create")
    try:
        for part in np.array_split(recs, 3):
            seqs = [bytes(r[:-1]) for r in part]
            data, offs = okm.pack_records(seqs)
            _lib.check(lib.okm_group_add_batch(g, data.ctypes.data, offs.ctypes.data, len(offs) - 1, 0),
                       "okm_group_add_batch")
        out = np.full(len(q), 77, np.uint64)
        nf = ctypes.c_uint64(99)
        _lib.check(lib.okm_group_lookup_counts(g, q.ctypes.data, len(q), out.ctypes.data, ctypes.byref(nf)),  # counts first
                   "okm_group_lookup_counts")
        assert np.array_equal(out, one) and nf.value == found
        assert lib.okm_group_lookup_counts(g, None, 4, out.ctypes.data, None) == _lib.OKM_E_ARG
        assert lib.okm_group_lookup_counts(g, q.ctypes.data, 4, None, None) == _lib.OKM_E_ARG
        assert lib.okm_group_lookup_counts(g, None, 0, None, ctypes.byref(nf)) == _lib.OKM_OK and nf.value == 0
        _lib.check(lib.okm_group_lookup_counts(g, q.ctypes.data, len(q), out.ctypes.data, None),
                   "okm_group_lookup_counts")
        assert np.array_equal(out, one)
    finally:
        lib.okm_group_destroy(g)


def test_set_mode_group_has_no_counts():
    lib = _lib.load()
    g = ctypes.c_void_p()
    _lib.check(lib.okm_group_create(ctypes.byref(g), K, _lib.OKM_MODE_SET, 1, None, 0), "okm_group_create")
    try:
        q, out = np.arange(1, 5, dtype=np.uint64), np.zeros(4, np.uint64)
        assert lib.okm_group_lookup_counts(g, q.ctypes.data, 4, out.ctypes.data, None) == _lib.OKM_E_STATE
    finally:
        lib.okm_group_destroy(g)


@pytest.mark.parametrize("P", [2, 3])
def test_owners_of_a_loopback_merge_sum_to_the_whole(group_reads, P):
    """What okm_group_lookup_counts does over N GPUs, on one: the owners of a
    P-rank merge hold disjoint key ranges, so every query is found on exactly
    one owner, or on none, and the per-owner arrays and n_found add."""
    recs, q, one, found = group_reads
    testing.set_knob("loopback_timeout_ms", 60_000)
    shards = [np.ascontiguousarray(p).reshape(-1) for p in np.array_split(recs, P)]
    comms = okm.Comm.init_loopback(P, 0)
    out, err = [None] * P, [None] * P

    def rank(r):
        local, owner = okm.KmerCounter(K), okm.KmerCounter(K)
        buf = okm.DeviceBuffer(len(shards[r]))
        try:
            buf.upload(shards[r])
            local.add_device_batch(buf.address, len(shards[r]))
            comms[r].merge_owned(local, owner)
            out[r] = _host(owner, q)
        except BaseException as e:  # surfaced below
            err[r] = e
        finally:
            buf.free()
            local.close()
            owner.close()

    th = [threading.Thread(target=rank, args=(r,), daemon=True) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
        assert not t.is_alive(), "a virtual rank hung"
    for c in comms:
        c.close()
    for e in err:
        if e is not None:
            raise e
    assert np.array_equal(sum(o for o, _ in out), one)
    assert sum(f for _, f in out) == found
    owners_with = sum((o > 0).astype(np.int64) for o, _ in out)
    assert np.array_equal(owners_with, (one > 0).astype(np.int64))  # exactly one owner, or none
    assert all(f > 0 for _, f in out)


# ---------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------

def _cli(*args):
    return subprocess.run([_lib.CLI_PATH, *args], capture_output=True, text=True, timeout=120)


def _text_of(v, k):
    return "".join("ACGT"[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))


@pytest.mark.parametrize("extra", [[], ["--gpus", "1"], ["-m", "2"]])
def test_cli_lookup(tmp_path, extra):
    fa = os.path.join(GOLDEN, "data", "test_input1.fasta.gz")
    recs = okm.read_fastx_file(fa, True)
    oc = OracleCounter(5)
    oc.add_records(recs, normalized=True)
    ek, ec = oc.result(1)
    table = {_text_of(int(v), 5): int(n) for v, n in zip(ek, ec)}
    record = next(r.decode() for r in recs if set(r) <= set(b"ACGT"))  # (the others hold N runs)
    assert len(record) >= 12
    absent = [m for m in ("AAAAA", "CCCCC", "GATCA", "ttttt", "TGATC") if lc.canonical_text(m) not in table]
    assert len(absent) >= 2
    text, kmers = lc.lookup_file_lines(record, 5, absent)
    look, plain, out, lo = tmp_path / "look.fa", tmp_path / "plain.tsv", tmp_path / "out.tsv", tmp_path / "l.tsv"
    look.write_bytes(text.encode())
    r = _cli("count", "-k", "5", "-i", fa, "-o", str(plain), *extra)
    assert r.returncode == 0, r.stderr
    r = _cli("count", "-k", "5", "-i", fa, "-o", str(out), "--lookup", str(look), "--lookup-output", str(lo), *extra)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == plain.read_bytes() and len(plain.read_bytes()) > 0
    exp = lc.render_lookup(kmers, table)  # the whole table, whatever --min-count
    assert lo.read_text() == exp
    assert any(line.endswith("\t0") for line in exp.splitlines()) and any(not line.endswith("\t0") for line in exp.splitlines())


def test_cli_lookup_wide_and_gz(tmp_path):
    k = 35
    rng = np.random.default_rng(43)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    read = acgt[rng.integers(0, 4, 80)].tobytes().decode()
    other = acgt[rng.integers(0, 4, 60)].tobytes().decode()
    fa = tmp_path / "in.fa"
    fa.write_text("".join(f">r{i}\n{read}\n" for i in range(4)) + ">other\n" + other + "\n")
    oc = OracleCounterWide(k)
    oc.add_records(okm.read_fastx_file(str(fa), True), normalized=True)
    ek, ec = oc.result(1)
    table = {_text_of(v, k): int(n) for v, n in zip(lc.from_pairs(ek), ec)}
    assert set(table.values()) == {1, 4}
    absent = ["A" * k, "ACGT" * 8 + "ACG", ("ACGT" * 8 + "ACG").lower()]
    assert all(lc.canonical_text(m) not in table for m in absent)
    text, kmers = lc.lookup_file_lines(read[:50] + other[:40], k, absent)  # (the k-mers across the joint are absent too)
    look, plain, out, lo = tmp_path / "look.txt.gz", tmp_path / "plain.tsv", tmp_path / "out.tsv", tmp_path / "l.tsv.gz"
    look.write_bytes(gzip.compress(text.encode()))
    assert _cli("count", "-k", str(k), "-i", str(fa), "-o", str(plain), "--wide").returncode == 0
    r = _cli("count", "-k", str(k), "-i", str(fa), "-o", str(out), "--wide", "--lookup", str(look), "--lookup-output",
             str(lo))
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == plain.read_bytes()
    exp = lc.render_lookup(kmers, table)
    assert {line.split("\t")[1] for line in exp.splitlines()} == {"0", "1", "4"}
    assert gzip.decompress(lo.read_bytes()).decode() == exp
