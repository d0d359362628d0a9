"""Inputs and numpy expectations of the count-histogram tests (not a test
file: tests/test_hist_cases.py checks on the CPU that every case has the
property its name claims; tests/test_gpu_count_histogram.py runs them).

The expectation is always numpy's: for the table's count array C,
    hist    = bincount(minimum(C, n_bins - 1), minlength=n_bins)
    summary = {len(C), sum(C) mod 2^64, max(C)}
Everything is an exact integer."""

from functools import lru_cache

import numpy as np

K = 31
N_BINS_MIN, N_BINS_MAX = 2, (1 << 20) + 1

# keys of one count item share their top bits (the 10 bits above bit 52; the L1
# bins take 9 or 10), as in tests/test_gpu_count_item_shapes.py
LOW_BITS = 52
PREFIX_BELOW = np.uint64(0x2A4) << np.uint64(LOW_BITS)
PREFIX = np.uint64(0x2A5) << np.uint64(LOW_BITS)
PREFIX_ABOVE = np.uint64(0x2A6) << np.uint64(LOW_BITS)

ITEM_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4096]
BIN_EDGE_NBINS = [2, 3, 257, 1000, 4097, 65536, 65537, 70001, 70002, (1 << 20) + 1]
BIN_EDGE_TOP = 70_000


def expected_hist(counts, n_bins):
    c = np.asarray(counts, dtype=np.uint64)
    return np.bincount(np.minimum(c, np.uint64(n_bins - 1)).astype(np.int64), minlength=n_bins).astype(np.uint64)


def expected_summary(counts):
    c = np.asarray(counts, dtype=np.uint64)
    if not len(c):
        return {"n_distinct": 0, "n_instances": 0, "max_count": 0}
    return {"n_distinct": len(c), "n_instances": int(c.sum(dtype=np.uint64)), "max_count": int(c.max())}  # uint64 sums wrap


def render_tsv(hist):
    """okm_write_histogram_tsv restated: COUNT<TAB>KMERS, zero bins omitted."""
    return "".join(f"{b}\t{int(h)}\n" for b, h in enumerate(hist) if int(h))


def table_of(keys, weights=None):
    """numpy's table of an add_pairs input: (sorted distinct keys, counts)."""
    keys = np.asarray(keys, dtype=np.uint64)
    if weights is None:
        ek, ec = np.unique(keys, return_counts=True)
        return ek, ec.astype(np.uint64)
    ek, inv = np.unique(keys, return_inverse=True)
    ec = np.zeros(len(ek), np.uint64)
    np.add.at(ec, inv, np.asarray(weights, dtype=np.uint64))
    return ek, ec


def _distinct_low(rng, n, bits=LOW_BITS):
    out = np.unique(rng.integers(0, 1 << bits, 2 * n + 8, dtype=np.uint64))[:n]
    assert len(out) == n
    return out


@lru_cache(maxsize=None)
def one_item(m):
    """Unweighted keys: m distinct keys under one item's prefix (each once, so
    they fit one item of 4096 instances) between two populated key ranges of
    100 keys, key i of which occurs (i mod 7) + 1 times.  m == 0: an empty key
    range between two populated ones."""
    rng = np.random.default_rng(1000 + m)
    flank = np.concatenate([PREFIX_BELOW | _distinct_low(rng, 100), PREFIX_ABOVE | _distinct_low(rng, 100)])
    flank = np.repeat(flank, (np.arange(len(flank)) % 7) + 1)
    mid = PREFIX | _distinct_low(rng, m) if m else np.zeros(0, np.uint64)
    return rng.permutation(np.concatenate([flank, mid]))


@lru_cache(maxsize=None)
def many_items():
    """Unweighted keys over the whole key space (many items): key i occurs
    (i mod 300) + 1 times; 3,000 keys, 451,500 instances."""
    rng = np.random.default_rng(17)
    keys = np.unique(rng.integers(0, 1 << 62, 3100, dtype=np.uint64))[:3000]
    assert len(keys) == 3000
    return rng.permutation(np.repeat(keys, (np.arange(3000) % 300) + 1))


@lru_cache(maxsize=None)
def all_one_count(count):
    """200,000 distinct keys, every one `count` times (unweighted)."""
    rng = np.random.default_rng(23)
    keys = np.unique(rng.integers(0, 1 << 62, 201_000, dtype=np.uint64))[:200_000]
    assert len(keys) == 200_000
    return rng.permutation(np.repeat(keys, count))


@lru_cache(maxsize=None)
def hot_among_singletons():
    """One key 4,096 times among 50,000 keys that occur once (unweighted)."""
    rng = np.random.default_rng(29)
    keys = np.unique(rng.integers(0, 1 << 62, 50_100, dtype=np.uint64))[:50_001]
    assert len(keys) == 50_001
    return rng.permutation(np.concatenate([np.full(4096, keys[25_000], np.uint64), np.delete(keys, 25_000)]))


@lru_cache(maxsize=None)
def count_equals_index():
    """Weighted pairs: 70,000 keys, the i-th (in input order) with count i for
    i in 1..70,000 -- for every n_bins of BIN_EDGE_NBINS up to 70,002 the table
    holds the counts n_bins - 2, n_bins - 1 and n_bins (where >= 1)."""
    rng = np.random.default_rng(31)
    keys = np.unique(rng.integers(0, 1 << 62, 70_500, dtype=np.uint64))[:BIN_EDGE_TOP]
    assert len(keys) == BIN_EDGE_TOP
    keys = rng.permutation(keys)
    return keys, np.arange(1, BIN_EDGE_TOP + 1, dtype=np.uint64)


@lru_cache(maxsize=None)
def past_u32_runs():
    """Three strictly ascending weighted runs (the shape of
    tests/test_gpu_merge.py::test_merge_counts_past_u32): one key holds 3e9 in
    two runs (6e9 merged), another a lone 5e9.  Returns (runs, (keys, counts))."""
    rng = np.random.default_rng(5)
    runs = []
    for _ in range(3):
        keys = np.unique(rng.integers(0, 1 << 40, 60_000, dtype=np.uint64))
        runs.append([keys, rng.integers(1, 1000, len(keys)).astype(np.uint64)])
    big = np.uint64(3_000_000_000)
    shared = runs[0][0][len(runs[0][0]) // 2]
    runs[0][1][len(runs[0][0]) // 2] = big
    k1 = np.unique(np.append(runs[1][0], shared))
    c1 = rng.integers(1, 1000, len(k1)).astype(np.uint64)
    c1[np.searchsorted(k1, shared)] = big
    runs[1] = [k1, c1]
    lone = runs[2][0][0]
    assert lone not in set(runs[0][0].tolist()) | set(k1.tolist())
    runs[2][1][0] = np.uint64(5_000_000_000)
    table = table_of(np.concatenate([r[0] for r in runs]), np.concatenate([r[1] for r in runs]))
    return [tuple(r) for r in runs], table


def fold_pairs():
    """Two unweighted add_pairs inputs that share half their keys (counted,
    then added to: the first table is folded into the second count)."""
    rng = np.random.default_rng(37)
    pool = np.unique(rng.integers(0, 1 << 62, 40_000, dtype=np.uint64))
    a = pool[rng.integers(0, len(pool) // 2, 120_000)]
    b = pool[rng.integers(len(pool) // 4, len(pool), 120_000)]
    return a, b
