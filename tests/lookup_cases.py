"""Inputs and expectations of the count-lookup tests (not a test file:
tests/test_lookup_cases.py checks on the CPU that every case has the property
its name claims; tests/test_gpu_lookup_counts.py runs them).

The expectation is always a plain table lookup: for the table (keys, counts),
    counts_of(q) = counts[keys == q], 0 where q is not a key
    n_found      = the number of queries that are keys (duplicates count)
by numpy's searchsorted for one-word keys and by a Python dict of integers for
two-word keys.  Everything is an exact integer."""

from functools import lru_cache

import numpy as np

import hist_cases as hc

K = hc.K
M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
CHUNK = 1 << 22          # okm_engine.hip kLookupChunk: host queries uploaded per launch
BLOCK_QUERIES = 256      # okm_lookup.hip kLookBlock * kLookFly: queries of one workgroup

# the runs a count leaves: sizes of one item's run around the wave (64) and at
# the item capacity (4096), each under its own 10-bit prefix (hist_cases.py),
# with empty key ranges between them
ITEM_SIZES = (1, 2, 63, 64, 65, 4096)
ITEM_PREFIXES = (0x011, 0x0A0, 0x150, 0x2A5, 0x300, 0x3F0)
QUERY_COUNTS = (0, 1, 63, 64, 65)
WIDE_KS = (33, 37, 63, 64)   # 37: the 12 home bits of an item straddle bit 64 (tests/wide_cases.py)


def expected(keys, counts, queries):
    """(counts of the queries, n_found) in a sorted one-word table."""
    keys = np.asarray(keys, dtype=np.uint64)
    counts = np.asarray(counts, dtype=np.uint64)
    q = np.asarray(queries, dtype=np.uint64)
    if not len(keys):
        return np.zeros(len(q), np.uint64), 0
    at = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
    hit = keys[at] == q
    return np.where(hit, counts[at], np.uint64(0)).astype(np.uint64), int(hit.sum())


def expected_wide(table, queries):
    """The same for Python integers: table is a dict key -> count."""
    out = np.array([table.get(int(q), 0) for q in queries], dtype=np.uint64)
    return out, sum(1 for q in queries if int(q) in table)


def to_pairs(ints):
    """Python ints -> (n, 2) uint64 [lo, hi]."""
    out = np.empty((len(ints), 2), dtype=np.uint64)
    out[:, 0] = np.fromiter((v & M64 for v in ints), dtype=np.uint64, count=len(ints))
    out[:, 1] = np.fromiter((v >> 64 for v in ints), dtype=np.uint64, count=len(ints))
    return out


def from_pairs(pairs):
    pairs = np.asarray(pairs, dtype=np.uint64).reshape(-1, 2)
    return [(int(h) << 64) | int(l) for l, h in pairs]


@lru_cache(maxsize=None)
def items():
    """One run of keys per entry of ITEM_SIZES, run i under ITEM_PREFIXES[i]
    (ascending, so the runs are in key order and every other prefix is an empty
    key range).  Returns (runs, pairs input): key j of a run occurs (j mod 3)
    + 1 times, the 4096-key run's keys once each (one item holds 4096
    instances)."""
    rng = np.random.default_rng(71)
    runs, inp = [], []
    for m, p in zip(ITEM_SIZES, ITEM_PREFIXES):
        keys = np.sort((np.uint64(p) << np.uint64(hc.LOW_BITS)) | hc._distinct_low(rng, m))
        runs.append(keys)
        inp.append(keys if m == 4096 else np.repeat(keys, (np.arange(m) % 3) + 1))
    return runs, rng.permutation(np.concatenate(inp))


def edge_queries(runs, top=(1 << 62) - 1):
    """The first and the last key of every run, the key one below the first and
    one above the last (absent: in the gap, or a neighbour's), one key below
    the table's first and one above its last."""
    q = []
    for r in runs:
        q += [r[0], r[-1], r[0] - np.uint64(1), r[-1] + np.uint64(1)]
    q += [np.uint64(0), runs[0][0] // np.uint64(2), np.uint64(top)]
    return np.array(q, dtype=np.uint64)


@lru_cache(maxsize=None)
def k32_table(with_zero):
    """k = 32 keys over all 64 bits, key 0 (all A) among them or not; 2^64 - 1
    never is one (all T: its canonical form is all A)."""
    rng = np.random.default_rng(73)
    keys = np.unique(rng.integers(1, M64, 5000, dtype=np.uint64))
    if with_zero:
        keys = np.concatenate([np.zeros(3, np.uint64), keys])
    return rng.permutation(keys)


@lru_cache(maxsize=None)
def word_neighbours(k):
    """Two-word keys that a comparison dropping a word confuses.  Returns
    (table dict, queries): the table holds keys equal in hi that differ in lo
    and keys equal in lo that differ in hi, among them lo = 0 and lo = 2^64 -
    1; the queries are every key, and one lo below, one lo above, one hi below
    and one hi above it (as 128-bit integers, so +-1 carries across bit 64)."""
    rng = np.random.default_rng(100 + k)
    top = (1 << (2 * k - 64)) - 1  # the largest hi word
    his = [0, 1, 3] if k == 33 else [0, top // 2 - 1, top // 2 + 1, top]  # (k = 33: hi has two bits)
    los = [0, 5, 7, 1 << 63, M64 - 2, M64] + [int(x) for x in rng.integers(1 << 20, 1 << 62, 40, dtype=np.uint64)]
    table = {}
    for i, h in enumerate(his):
        for j, l in enumerate(los):
            if (i + j) % 4 == 3:
                continue  # some (hi, lo) combinations stay absent
            table[(h << 64) | l] = 1 + (i * 7 + j) % 5
    table.pop((1 << (2 * k)) - 1, None)  # all T is never canonical (and is the engine's padding key)
    queries = []
    for v in sorted(table):
        queries += [v, (v - 1) & M128, (v + 1) & M128, (v - (1 << 64)) & M128, (v + (1 << 64)) & M128]
    return table, queries


def table_input(table):
    """add_pairs input of a dict table: every key count times, shuffled."""
    keys = sorted(table)
    pairs = to_pairs([v for v in keys for _ in range(table[v])])
    return pairs[np.random.default_rng(3).permutation(len(pairs))]


def kmers_of(seq, k):
    return [seq[i:i + k] for i in range(len(seq) - k + 1)]


def canonical_text(kmer):
    rc = kmer.upper()[::-1].translate(str.maketrans("ACGT", "TGCA"))
    return min(kmer.upper(), rc)


def lookup_file_lines(record, k, absent):
    """A --lookup file over one record: a '>' line, every k-mer of the record
    in alternating case, a blank line, the absent k-mers; (text, k-mers in
    file order as written)."""
    kmers = [m.lower() if i % 2 else m for i, m in enumerate(kmers_of(record, k))] + list(absent)
    n = len(kmers) - len(absent)
    text = ">kmers of one record\n" + "\n".join(kmers[:n]) + "\n\n" + "\r\n".join(kmers[n:]) + "\n"
    return text, kmers


def render_lookup(kmers, table):
    """The --lookup-output file: KMER<TAB>COUNT per listed k-mer, as written;
    table: canonical upper-case text -> count."""
    return "".join(f"{m}\t{table.get(canonical_text(m), 0)}\n" for m in kmers)
