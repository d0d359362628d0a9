"""Item shapes of the LDS count kernels (okm_count.hip), exact against numpy.

One item is a key range of at most 4,096 instances; the tag kernel takes its
instances in rows of 512, gives every one of its 2,048 homes (the 11 key bits
below the item's common prefix) a tag key, and counting-sorts the other
("rest") instances; an item with more rest instances than the rest buffer
holds (896), a dense item (few remaining key bits) or, in the single-segment
kernel, an item of several segments goes to the slow kernel.  The cases pin
the edges of those shapes: row and capacity boundaries, the packed 16-bit tag
count at its largest value, crowded homes, deferral, the dense limit, and
items that span several sorted runs (the generic loaders).  They state
behaviour, not an implementation: every expectation is numpy's or the
oracle's.
"""

import numpy as np
import pytest

import okm
from oracle import OracleCounter

pytestmark = pytest.mark.gpu

K = 31
# keys of one item share their top bits: here the 10 bits above bit 52 (the
# L1 bins take 9 or 10), everything below is free
PREFIX = np.uint64(0x2A5) << np.uint64(52)
LOW_BITS = 52


def _count_pairs(keys, k=K):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    with okm.KmerCounter(k) as c:
        c.set_timing(True)
        c.add_pairs(keys)
        gk, gc = c.result(1)
        stats = c.kernel_stats()
    assert "count_items" in stats and stats["count_items"]["launches"] >= 1
    return gk, gc


def _check_pairs(keys, k=K):
    gk, gc = _count_pairs(keys, k)
    ek, ec = np.unique(np.asarray(keys, dtype=np.uint64), return_counts=True)
    assert np.array_equal(gk, ek)
    assert np.array_equal(gc, ec.astype(np.uint64))


def _low(rng, n, bits=LOW_BITS):
    return rng.integers(0, 1 << bits, n, dtype=np.uint64)


EDGES = [1, 2, 511, 512, 513, 4095, 4096, 4097]


@pytest.mark.parametrize("n", EDGES)
def test_one_item_rows_with_repeats(n):
    """n instances drawn from n/4 keys (the tag path's usual mix); 4,097 is one
    past an item's capacity and must still count exactly."""
    rng = np.random.default_rng(n)
    pool = PREFIX | _low(rng, max(1, n // 4))
    _check_pairs(pool[rng.integers(0, len(pool), n)])


@pytest.mark.parametrize("n", EDGES)
def test_one_item_all_distinct(n):
    rng = np.random.default_rng(100 + n)
    keys = PREFIX | np.unique(_low(rng, 2 * n))[:n]
    assert len(keys) == n
    _check_pairs(rng.permutation(keys))


@pytest.mark.parametrize("n", [4095, 4096])
def test_one_key_fills_the_item(n):
    """The packed 16-bit tag count at its largest value."""
    _check_pairs(np.full(n, PREFIX | np.uint64(0x1234_5678_9ABC), dtype=np.uint64))


@pytest.mark.parametrize("order", ["tag_low", "tag_high", "tag_middle"])
@pytest.mark.parametrize("crowd", [2, 3, 40])
def test_keys_sharing_a_home(order, crowd):
    """Keys that differ only below the home field: one becomes the home's tag
    (most likely the one in the first row), the others are rest keys below and
    above it.  Around them, an ordinary mix."""
    rng = np.random.default_rng(crowd)
    home = PREFIX | (np.uint64(0x155) << np.uint64(41))
    crowd_keys = home | np.unique(_low(rng, 4 * crowd, 18))[:crowd]
    first = {"tag_low": crowd_keys[0], "tag_high": crowd_keys[-1], "tag_middle": crowd_keys[crowd // 2]}[order]
    pool = PREFIX | _low(rng, 400)
    body = np.concatenate([pool[rng.integers(0, len(pool), 1600)], np.repeat(crowd_keys, 5)])
    keys = np.concatenate([np.full(3, first, dtype=np.uint64), rng.permutation(body)])
    _check_pairs(keys)


def test_item_with_too_many_rest_instances():
    """3,000 distinct keys sharing everything above their lowest 18 bits: one
    home, one tag, 2,999 rest instances -- more than the rest buffer holds, so
    the item is deferred, and still exact."""
    rng = np.random.default_rng(7)
    keys = PREFIX | (np.uint64(0x3C1) << np.uint64(41)) | np.unique(_low(rng, 8000, 18))[:3000]
    assert len(keys) == 3000
    _check_pairs(rng.permutation(keys))


def test_hot_key_beside_sparse_keys():
    rng = np.random.default_rng(9)
    hot = np.uint64(0x0123_4567_89AB_CDEF) >> np.uint64(2)
    sparse = rng.integers(0, 1 << 62, 60_000, dtype=np.uint64)
    keys = rng.permutation(np.concatenate([np.full(100_000, hot, dtype=np.uint64), sparse]))
    _check_pairs(keys)


def _random_reads(rng, n, length):
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [acgt[rng.integers(0, 4, length)].tobytes() for _ in range(n)]


def _check_records(seqs, k):
    with okm.KmerCounter(k) as c:
        c.set_timing(True)
        c.add_records(seqs)
        gk, gc = c.result(1)
        stats = c.kernel_stats()
    assert "count_items" in stats
    oc = OracleCounter(k)
    oc.add_records(seqs)
    ek, ec = oc.result(1)
    assert np.array_equal(gk, ek) and np.array_equal(gc, ec)


@pytest.mark.parametrize("k", [5, 6, 7, 8, 9, 10])
def test_small_k_around_the_dense_limit(k):
    """2k key bits less the L1 bits leave 11 remaining bits (the dense limit) or
    a few more or fewer at these k."""
    rng = np.random.default_rng(k)
    _check_records(_random_reads(rng, 300, 120), k)


@pytest.mark.parametrize("n", EDGES)
def test_row_edges_from_bytes(n):
    """One read n times: each of its k-mers has n instances (end to end from
    bytes), beside a few reads that occur once."""
    rng = np.random.default_rng(200 + n)
    read = _random_reads(rng, 1, 60)[0]
    _check_records([read] * n + _random_reads(rng, 20, 80), K)


def test_crowded_home_from_bytes():
    """Reads that differ in their last bases only: k-mers that share all but
    their lowest bits."""
    rng = np.random.default_rng(11)
    stem = _random_reads(rng, 1, 40)[0]
    tails = _random_reads(rng, 3000, 6)
    _check_records([stem + t for t in tails], K)


def _upload(arr):
    arr = np.ascontiguousarray(arr, dtype=np.uint64)
    buf = okm.DeviceBuffer(max(arr.nbytes, 8))
    buf.upload(arr)
    return buf


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nruns", [2, 4, 5, 65])
def test_items_spanning_sorted_runs(nruns, weighted):
    """Strictly ascending runs spread over the whole key space: every key-range
    item holds a slice of each run (the 2..4-run, staged and generic loaders)."""
    rng = np.random.default_rng(nruns)
    shared = rng.integers(0, 1 << 62, 1500, dtype=np.uint64)  # keys that every run holds
    runs = []
    for _ in range(nruns):
        keys = np.unique(np.concatenate([rng.integers(0, 1 << 62, 3000, dtype=np.uint64), shared]))
        runs.append((keys, rng.integers(1, 1000, len(keys)).astype(np.uint64)))
    allk = np.concatenate([r[0] for r in runs])
    allw = np.concatenate([r[1] if weighted else np.ones(len(r[0]), np.uint64) for r in runs])
    ek, inv = np.unique(allk, return_inverse=True)
    ec = np.zeros(len(ek), np.uint64)
    np.add.at(ec, inv, allw)
    bufs = []
    with okm.KmerCounter(K) as c:
        c.set_timing(True)
        for keys, counts in runs:
            bk = _upload(keys)
            bc = _upload(counts) if weighted else None
            bufs += [bk, bc]
            c.add_sorted_pairs_device(bk.address, bc.address if bc else None, len(keys))
        gk, gc = c.result(1)
        stats = c.kernel_stats()
    assert "count_items" in stats
    assert np.array_equal(gk, ek) and np.array_equal(gc, ec)


@pytest.mark.parametrize("k", [17, 31, 32])
def test_batch_against_oracle(k):
    batch = okm.synth_reads(30_000, 150, genome_len=1_000_000, genome_seed=3, seed=3)
    buf = okm.DeviceBuffer(len(batch), 0)
    buf.upload(batch)
    with okm.KmerCounter(k) as c:
        c.set_timing(True)
        c.add_device_batch(buf.address, len(batch))
        gk, gc = c.result(1)
        stats = c.kernel_stats()
    buf.free()
    assert "count_items" in stats
    oc = OracleCounter(k)
    oc.add_separated(batch)
    ek, ec = oc.result(1)
    assert np.array_equal(gk, ek) and np.array_equal(gc, ec)
